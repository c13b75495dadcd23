// s3d_ssfid.hip — the activation statistics of the reference's evaluation/ssfid.py on the device: the first two layers of the 3-D
// voxel classifier (evaluation/classifier3D.py: Conv3d k4 s2 p1 + InstanceNorm3d + leaky_relu 0.01, twice), then the mean and the
// ddof = 1 covariance of the activations' rows.  DESIGN.md §21.
//
//   k_ssfid_l1      occupancy -> pre-activations [R1][32] (binary input: bias + the occupied taps' weights, fixed tap order) and
//                   per-block {sum d, sum d^2} per channel, d = x - bias, in float64
//   k_ssfid_mr      partials -> {mean, rstd} per channel (float64), parts added in index order
//   k_ssfid_l2      implicit GEMM on mfma_f32_32x32x2f32: M = 4 x 4 x 8 output voxels per block, N = 64, K = 64 taps x 32 channels in
//                   four 8-channel halo chunks; normalise + leaky_relu applied while staging the halo, out-of-range positions
//                   staged as exact zeros; the epilogue leaves the second norm's partials
//   SfRows          normalise + leaky_relu of the rows and their activations (optional), as the load of k_rows_gram: the column
//                   sums, the C x C Gram and k_rows_cov's mu, sigma are s3d_rowstats.h's, 128 rows per block
//
// No float atomics; every sum has a fixed order that depends on the volume's shape alone, so the same input gives the same bits.
// Statistics are taken about the channel's bias: a constant channel (an empty volume) has variance exactly 0 and normalises to
// exactly 0, as in exact arithmetic.
#include "s3d_rowstats.h"

namespace s3d {

constexpr int kSfThreads = 256;
constexpr int kSfC1 = 32, kSfC2 = 64, kSfTaps = 64;
constexpr float kSfSlope = 0.01f;
constexpr double kSfEps = 1e-5;
constexpr int kSfMaxDim = 1024;                       // per axis; indices below are 64-bit where a product can pass 2^31
// layer 2 tile: 4 x 4 x 8 output voxels, halo 10 x 10 x 18 input positions, 8 input channels per chunk
constexpr int kSfTx = 4, kSfTy = 4, kSfTz = 8;
constexpr int kSfHx = 2 * kSfTx + 2, kSfHy = 2 * kSfTy + 2, kSfHz = 2 * kSfTz + 2;
constexpr int kSfChunk = 8, kSfChunks = kSfC1 / kSfChunk;
constexpr int kSfHalo = kSfHx * kSfHy * kSfHz;        // 1800 positions
constexpr int kSfStageBatch = 5;                      // halo loads in flight per thread while staging (15 per chunk)
constexpr int kSfFlushTaps = 2;                       // taps per float32 MFMA chain of layer 2 (1, 2 or 4)
constexpr int kSfGramSpan = 128;                      // rows per block of k_rows_gram: 256 blocks at 128^3, one per CU

__device__ static inline float sf_act(float x, double mean, double rstd) {
    const float v = float((double(x) - mean) * rstd);
    return v > 0.f ? v : v * kSfSlope;
}

// ------------------------------------------------------------------ layer 1
// One thread per output voxel (row r = (ox * Y1 + oy) * Z1 + oz), all 32 channels in registers; the weights wT [64 taps][32] are
// staged in LDS and read at wave-uniform addresses.  The block's 256 x 32 outputs go through LDS (row stride 33) for the statistics (thread t sums
// channel t % 32 over rows t / 32 * 32 ...) and for stores in the output's own order.
__global__ void __launch_bounds__(kSfThreads) k_ssfid_l1(const unsigned char* __restrict__ vox, int X, int Y, int Z, int Y1, int Z1,
                                                         long long R1, const float* __restrict__ wT, const float* __restrict__ bias,
                                                         float* __restrict__ raw, double* __restrict__ part) {
    __shared__ float tile[kSfThreads * (kSfC1 + 1)];
    __shared__ double red[8][kSfC1][2];
    __shared__ f32x4 wl[kSfTaps * kSfC1 / 4];
    const int t = threadIdx.x;
    for (int i = t; i < kSfTaps * kSfC1 / 4; i += kSfThreads) wl[i] = reinterpret_cast<const f32x4*>(wT)[i];
    __syncthreads();
    const long long r0 = (long long)blockIdx.x * kSfThreads, r = r0 + t;
    const bool live = r < R1;
    const long long rr = live ? r : R1 - 1;
    const int oz = int(rr % Z1), oy = int((rr / Z1) % Y1), ox = int(rr / ((long long)Z1 * Y1));
    float acc[kSfC1];
#pragma unroll
    for (int c = 0; c < kSfC1; ++c) acc[c] = 0.f;
#pragma unroll 1
    for (int kx = 0; kx < 4; ++kx) {
        const int ix = 2 * ox - 1 + kx;
#pragma unroll 1
        for (int ky = 0; ky < 4; ++ky) {
            const int iy = 2 * oy - 1 + ky;
            const bool rowin = (unsigned)ix < (unsigned)X && (unsigned)iy < (unsigned)Y;
            const unsigned char* row = vox + ((long long)(rowin ? ix : 0) * Y + (rowin ? iy : 0)) * Z;
#pragma unroll
            for (int kz = 0; kz < 4; ++kz) {
                const int iz = 2 * oz - 1 + kz;
                const bool in = rowin && (unsigned)iz < (unsigned)Z;
                const float o = (in && row[in ? iz : 0] != 0) ? 1.f : 0.f;
                const f32x4* w = wl + ((kx * 4 + ky) * 4 + kz) * (kSfC1 / 4);
#pragma unroll
                for (int c4 = 0; c4 < kSfC1 / 4; ++c4) {
                    const f32x4 w4 = w[c4];                                // one address for the wave: a broadcast read
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc[c4 * 4 + e] = fmaf(o, w4[e], acc[c4 * 4 + e]);
                }
            }
        }
    }
#pragma unroll
    for (int c = 0; c < kSfC1; ++c) tile[t * (kSfC1 + 1) + c] = acc[c] + bias[c];
    __syncthreads();
    {
        const int c = t & 31, g = t >> 5;
        const double b = double(bias[c]);
        double s = 0.0, q = 0.0;
        for (int i = 0; i < 32; ++i) {
            const int row = g * 32 + i;
            if (r0 + row < R1) {
                const double d = double(tile[row * (kSfC1 + 1) + c]) - b;
                s += d;
                q = fma(d, d, q);
            }
        }
        red[g][c][0] = s;
        red[g][c][1] = q;
    }
    const long long n = min((long long)kSfThreads, R1 - r0) * kSfC1;
    for (int e = t; e < n; e += kSfThreads) raw[r0 * kSfC1 + e] = tile[(e >> 5) * (kSfC1 + 1) + (e & 31)];
    __syncthreads();
    if (t < kSfC1 * 2) {
        const int c = t >> 1, k = t & 1;
        double s = 0.0;
#pragma unroll
        for (int g = 0; g < 8; ++g) s += red[g][c][k];
        part[((long long)blockIdx.x * kSfC1 + c) * 2 + k] = s;
    }
}

// ------------------------------------------------------------------ partials -> {mean, rstd}
// One wave per channel: lane l adds parts l, l + 64, ... in order, then a fixed xor tree.  mean = bias + S1 / n,
// var = S2 / n - (S1 / n)^2 (biased), rstd = 1 / sqrt(var + 1e-5).
__global__ void __launch_bounds__(64) k_ssfid_mr(const double* __restrict__ part, int nparts, int C, const float* __restrict__ bias, double count,
                                                 double* __restrict__ mr) {
    const int c = blockIdx.x, l = threadIdx.x;
    double s = 0.0, q = 0.0;
    for (int p = l; p < nparts; p += 64) {
        s += part[((long long)p * C + c) * 2 + 0];
        q += part[((long long)p * C + c) * 2 + 1];
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        s += __shfl_xor(s, off);
        q += __shfl_xor(q, off);
    }
    if (l == 0) {
        const double m = s / count;
        double var = q / count - m * m;
        var = var > 0.0 ? var : 0.0;
        mr[c * 2 + 0] = double(bias[c]) + m;
        mr[c * 2 + 1] = 1.0 / sqrt(var + kSfEps);
    }
}

// ------------------------------------------------------------------ layer 2
// wp: the weights in fragment order, float4 at (((q * 64 + tap) * 2 + nb) * 64 + lane): element e = w[co = nb * 32 + lane % 32]
// [ci = q * 8 + lane / 32 * 4 + e][tap].  Wave w owns the tile's x = w plane (32 voxels: m = y * 8 + z) and both halves of the
// output channels.  Per tap and chunk: one 16-byte LDS read of A, two 16-byte weight reads, eight MFMAs.  A float32 MFMA chain runs
// over kSfFlushTaps taps of one chunk (k order: tap, e, lane half, i.e. channel q * 8 + {0, 4, 1, 5, 2, 6, 3, 7} inside a tap) and
// is then added to the float64 accumulator, in (chunk, tap) order: a 2048-term float32 chain leaves 5e-7 rms in the activations
// and 2e-7 in a distance of 0.36, twenty times the reference's own float32 error there; 16-term chains leave the
// float32 rounding of the stored values.
__device__ static inline void sf_load_w(const f32x4* __restrict__ wp, int grp, int lane, f32x4 (&b)[8]) {
#pragma unroll
    for (int i = 0; i < 8; ++i) b[i] = wp[(grp * 8 + i) * 64 + lane];     // grp = q * 16 + kx * 4 + ky; i = kz * 2 + nb
}

// One (chunk, kx, ky) group: four taps, 32 MFMAs.  A chain runs over kSfFlushTaps taps; between its MFMAs the chain before (p0, p1,
// complete by then) is added to the float64 accumulators.
__device__ __forceinline__ void sf_group(const f32x4* halo, int apos, int half, const f32x4 (&bc)[8], double (&acc)[2][16], f32x16& p0,
                                         f32x16& p1) {
#pragma unroll
    for (int u = 0; u < 4 / kSfFlushTaps; ++u) {
        f32x16 c0, c1;
#pragma unroll
        for (int i = 0; i < 16; ++i) { c0[i] = 0.f; c1[i] = 0.f; }
#pragma unroll
        for (int kk = 0; kk < kSfFlushTaps; ++kk) {
            const int kz = u * kSfFlushTaps + kk;
            const f32x4 a4 = halo[(apos + kz) * 2 + half];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                c0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[e], bc[kz * 2 + 0][e], c0, 0, 0, 0);
                c1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[e], bc[kz * 2 + 1][e], c1, 0, 0, 0);
                constexpr int per = 16 / (4 * kSfFlushTaps);              // elements of the previous chain per step
#pragma unroll
                for (int j = 0; j < per; ++j) {
                    const int i = (kk * 4 + e) * per + j;
                    acc[0][i] += double(p0[i]);
                    acc[1][i] += double(p1[i]);
                }
                __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
                __builtin_amdgcn_sched_group_barrier(0x002, 4 * per, 0);
            }
        }
        p0 = c0;
        p1 = c1;
    }
}

__global__ void __launch_bounds__(kSfThreads) k_ssfid_l2(const float* __restrict__ raw1, int X1, int Y1, int Z1, const double* __restrict__ mr1,
                                                         const f32x4* __restrict__ wp, const float* __restrict__ bias, int X2, int Y2, int Z2,
                                                         int nty, int ntz, float* __restrict__ raw2, double* __restrict__ part) {
    __shared__ f32x4 halo[kSfHalo * 2];                                   // [hx][hy][hz][8 channels]
    __shared__ double red[4][kSfC2][2];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, half = lane >> 5, m = lane & 31;
    const int bz = blockIdx.x % ntz, by = (blockIdx.x / ntz) % nty, bx = blockIdx.x / (ntz * nty);
    const int ox0 = bx * kSfTx, oy0 = by * kSfTy, oz0 = bz * kSfTz;
    const int ix0 = 2 * ox0 - 1, iy0 = 2 * oy0 - 1, iz0 = 2 * oz0 - 1;
    double acc[2][16];
    f32x16 p0, p1;                                                        // the chain that waits to be added (zeros before the first)
#pragma unroll
    for (int i = 0; i < 16; ++i) { acc[0][i] = 0.0; acc[1][i] = 0.0; p0[i] = 0.f; p1[i] = 0.f; }
    const int abase = ((2 * wave) * kSfHy + 2 * (m >> 3)) * kSfHz + 2 * (m & 7);       // halo position of tap (0, 0, 0)
    f32x4 b0[8], b1[8];
    sf_load_w(wp, 0, lane, b0);
    for (int q = 0; q < kSfChunks; ++q) {
        if (q) __syncthreads();                                           // the previous chunk's reads are done
        {
            const int sub = t & 1;                                        // kSfThreads is even: a thread keeps its four channels
            double mean[4], rstd[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                mean[e] = mr1[(q * kSfChunk + sub * 4 + e) * 2];
                rstd[e] = mr1[(q * kSfChunk + sub * 4 + e) * 2 + 1];
            }
            // loads in batches of kSfStageBatch so that their latencies overlap; normalise and store afterwards
            constexpr int kIters = (kSfHalo * 2 + kSfThreads - 1) / kSfThreads;
#pragma unroll 1
            for (int it0 = 0; it0 < kIters; it0 += kSfStageBatch) {
                f32x4 x[kSfStageBatch];
                bool in[kSfStageBatch];
#pragma unroll
                for (int k = 0; k < kSfStageBatch; ++k) {
                    const int i = t + (it0 + k) * kSfThreads, pos = i >> 1;
                    const int hz = pos % kSfHz, hy = (pos / kSfHz) % kSfHy, hx = pos / (kSfHz * kSfHy);
                    const int ix = ix0 + hx, iy = iy0 + hy, iz = iz0 + hz;
                    in[k] = i < kSfHalo * 2 && (unsigned)ix < (unsigned)X1 && (unsigned)iy < (unsigned)Y1 && (unsigned)iz < (unsigned)Z1;
                    x[k] = f32x4{0.f, 0.f, 0.f, 0.f};
                    if (in[k]) x[k] = *reinterpret_cast<const f32x4*>(raw1 + (((long long)ix * Y1 + iy) * Z1 + iz) * kSfC1 + q * kSfChunk + sub * 4);
                }
#pragma unroll
                for (int k = 0; k < kSfStageBatch; ++k) {
                    const int i = t + (it0 + k) * kSfThreads;
                    f32x4 v = {0.f, 0.f, 0.f, 0.f};
                    if (in[k]) {
#pragma unroll
                        for (int e = 0; e < 4; ++e) v[e] = sf_act(x[k][e], mean[e], rstd[e]);
                    }
                    if (i < kSfHalo * 2) halo[i] = v;
                }
            }
        }
        __syncthreads();
#pragma unroll 1
        for (int g2 = 0; g2 < 16; g2 += 2) {
            // two groups per trip, two weight register sets: each set is refilled one whole group (32 MFMAs) before it is used,
            // and the scheduling barriers keep the loads where they are written
            const int grp = q * 16 + g2;
            sf_load_w(wp, grp + 1, lane, b1);
            __builtin_amdgcn_sched_barrier(0);
            sf_group(halo, abase + ((g2 >> 2) * kSfHy + (g2 & 3)) * kSfHz, half, b0, acc, p0, p1);
            __builtin_amdgcn_sched_barrier(0);
            sf_load_w(wp, grp + 2 < kSfChunks * 16 ? grp + 2 : grp, lane, b0);         // the last trip re-fetches a group
            __builtin_amdgcn_sched_barrier(0);
            sf_group(halo, abase + ((g2 >> 2) * kSfHy + (g2 & 3) + 1) * kSfHz, half, b1, acc, p0, p1);
            __builtin_amdgcn_sched_barrier(0);
        }
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) { acc[0][i] += double(p0[i]); acc[1][i] += double(p1[i]); }
    // epilogue: register i of lane (m, half) is voxel (x = wave, y = i / 4, z = half * 4 + i % 4), channel nb * 32 + m
    const int ox = ox0 + wave;
#pragma unroll
    for (int nb = 0; nb < 2; ++nb) {
        const int co = nb * 32 + m;
        const double bd = double(bias[co]);
        double s = 0.0, qq = 0.0;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int oy = oy0 + (i >> 2), oz = oz0 + half * 4 + (i & 3);
            if (ox < X2 && oy < Y2 && oz < Z2) {
                const float x = float(acc[nb][i] + bd);
                raw2[(((long long)ox * Y2 + oy) * Z2 + oz) * kSfC2 + co] = x;
                const double d = double(x) - bd;
                s += d;
                qq = fma(d, d, qq);
            }
        }
        s += __shfl_xor(s, 32);
        qq += __shfl_xor(qq, 32);
        if (half == 0) { red[wave][co][0] = s; red[wave][co][1] = qq; }
    }
    __syncthreads();
    if (t < kSfC2 * 2) {
        const int c = t >> 1, k = t & 1;
        part[((long long)blockIdx.x * kSfC2 + c) * 2 + k] = ((red[0][c][k] + red[1][c][k]) + red[2][c][k]) + red[3][c][k];
    }
}

// ------------------------------------------------------------------ rows -> activations: the Load of k_rows_gram
// a = leaky_relu((x - mean) * rstd) as float32 (what the reference hands to np.cov), written to `act` when asked for.  A thread
// keeps its channel quad (kRsThreads is a multiple of C / 4), so bind fetches its four {mean, rstd} pairs once.
template <int C>
struct SfRows {
    static_assert(kRsThreads % (C / 4) == 0, "a thread keeps its channel quad");
    const float* raw;
    const double* mr;
    float* act;
    double mean[4] = {}, rstd[4] = {};
    __device__ void bind(int cq) {
#pragma unroll
        for (int e = 0; e < 4; ++e) { mean[e] = mr[(cq * 4 + e) * 2]; rstd[e] = mr[(cq * 4 + e) * 2 + 1]; }
    }
    __device__ f32x4 operator()(long long, long long row, int cq) const {
        const f32x4 x = *reinterpret_cast<const f32x4*>(raw + row * C + cq * 4);
        f32x4 v;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = sf_act(x[e], mean[e], rstd[e]);
        if (act) *reinterpret_cast<f32x4*>(act + row * C + cq * 4) = v;
        return v;
    }
};

}  // namespace s3d

using namespace s3d;

struct s3d_ssfid {
    std::vector<float> host[4];          // conv_1.weight, conv_1.bias, conv_2.weight, conv_2.bias as given
    bool have[4] = {false, false, false, false};
    bool packed = false;
    DevBuf w1T, b1, w2p, b2;             // [64][32]; [32]; fragment order (k_ssfid_l2); [64]
    DevBuf raw1, raw2, part1, part2, mr1, mr2, gpart, mpart;
    StageTimer<5> timer;                 // s3d_ssfid_profile: layer 1, its statistics, layer 2, its statistics, the covariance
    int last_layer = 0;
};

static const struct { const char* name; int ndim; int64_t shape[5]; } kSfParams[4] = {
    {"conv_1.weight", 5, {kSfC1, 1, 4, 4, 4}},
    {"conv_1.bias", 1, {kSfC1, 0, 0, 0, 0}},
    {"conv_2.weight", 5, {kSfC2, kSfC1, 4, 4, 4}},
    {"conv_2.bias", 1, {kSfC2, 0, 0, 0, 0}},
};

static int ssfid_pack(s3d_ssfid* h) {
    std::vector<float> w1T(size_t(kSfTaps) * kSfC1), w2p(size_t(kSfChunks) * kSfTaps * 2 * 64 * 4);
    for (int c = 0; c < kSfC1; ++c)
        for (int tap = 0; tap < kSfTaps; ++tap) w1T[size_t(tap) * kSfC1 + c] = h->host[0][size_t(c) * kSfTaps + tap];
    for (int q = 0; q < kSfChunks; ++q)
        for (int tap = 0; tap < kSfTaps; ++tap)
            for (int nb = 0; nb < 2; ++nb)
                for (int lane = 0; lane < 64; ++lane)
                    for (int e = 0; e < 4; ++e) {
                        const int co = nb * 32 + (lane & 31), ci = q * kSfChunk + (lane >> 5) * 4 + e;
                        w2p[((((size_t(q) * kSfTaps + tap) * 2 + nb) * 64) + lane) * 4 + e] = h->host[2][(size_t(co) * kSfC1 + ci) * kSfTaps + tap];
                    }
    S3D_TRY(upload(h->w1T, w1T.data(), w1T.size() * sizeof(float)));
    S3D_TRY(upload(h->b1, h->host[1].data(), kSfC1 * sizeof(float)));
    S3D_TRY(upload(h->w2p, w2p.data(), w2p.size() * sizeof(float)));
    S3D_TRY(upload(h->b2, h->host[3].data(), kSfC2 * sizeof(float)));
    h->packed = true;
    return 0;
}

extern "C" {

int s3d_ssfid_create(s3d_ssfid** out) {
    S3D_CHECK(out, S3D_ERR_INVALID, "ssfid_create: null argument");
    *out = new s3d_ssfid();
    return 0;
}
void s3d_ssfid_destroy(s3d_ssfid* h) { delete h; }

int s3d_ssfid_set_param(s3d_ssfid* h, const char* name, const float* data, const int64_t* shape, int ndim) {
    S3D_CHECK(h && name && data && shape, S3D_ERR_INVALID, "ssfid set_param: null argument");
    for (int p = 0; p < 4; ++p) {
        if (strcmp(kSfParams[p].name, name) != 0) continue;
        size_t n;
        S3D_TRY(check_param_shape("ssfid", name, shape, ndim, kSfParams[p].shape, kSfParams[p].ndim,
                                  "the classifier of ef_dim = 32 is the one supported", n));
        h->host[p].assign(data, data + n);
        h->have[p] = true;
        h->packed = false;
        return 0;
    }
    set_error("ssfid set_param: unexpected key '%s' (conv_1.weight, conv_1.bias, conv_2.weight, conv_2.bias are taken)", name);
    return S3D_ERR_INVALID;
}

int s3d_ssfid_out_dims(const int dims[3], int out_layer, int out_dims[3], int* channels) {
    S3D_CHECK(dims && out_dims, S3D_ERR_INVALID, "ssfid_out_dims: null argument");
    S3D_CHECK(out_layer >= 1 && out_layer <= 4, S3D_ERR_INVALID, "ssfid: out_layer %d, the classifier has layers 1..4", out_layer);
    S3D_CHECK(out_layer <= 2, S3D_ERR_UNSUPPORTED, "ssfid: out_layer %d is not built; 1 and 2 (the reference's choice) are", out_layer);
    for (int k = 0; k < 3; ++k) {
        S3D_CHECK(dims[k] >= 1, S3D_ERR_INVALID, "ssfid: axis %d has %d voxels", k, dims[k]);
        S3D_CHECK(dims[k] <= kSfMaxDim, S3D_ERR_UNSUPPORTED, "ssfid: axis %d has %d voxels, %d at most", k, dims[k], kSfMaxDim);
        out_dims[k] = dims[k] >> out_layer;
        S3D_CHECK(out_dims[k] >= 1, S3D_ERR_INVALID, "ssfid: axis %d of %d voxels leaves no output at layer %d", k, dims[k], out_layer);
    }
    if (channels) *channels = out_layer == 1 ? kSfC1 : kSfC2;
    return 0;
}

int s3d_ssfid_features(s3d_ssfid* h, const uint8_t* vox, const int dims[3], int out_layer, float* act, double* mu, double* sigma, void* stream) {
    S3D_CHECK(h && vox && dims && mu && sigma, S3D_ERR_INVALID, "ssfid_features: null argument");
    int od[3];
    S3D_TRY(s3d_ssfid_out_dims(dims, out_layer, od, nullptr));
    for (int p = 0; p < 4; ++p) S3D_CHECK(h->have[p], S3D_ERR_INVALID, "ssfid_features: %s has not been set", kSfParams[p].name);
    if (!h->packed) S3D_TRY(ssfid_pack(h));
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int X = dims[0], Y = dims[1], Z = dims[2];
    const int X1 = X / 2, Y1 = Y / 2, Z1 = Z / 2, X2 = X1 / 2, Y2 = Y1 / 2, Z2 = Z1 / 2;
    const long long R1 = (long long)X1 * Y1 * Z1, R2 = (long long)X2 * Y2 * Z2;
    const long long nb1 = (R1 + kSfThreads - 1) / kSfThreads;
    S3D_CHECK(nb1 < (1LL << 31), S3D_ERR_UNSUPPORTED, "ssfid_features: volume too large");

    const int ntx = (X2 + kSfTx - 1) / kSfTx, nty = (Y2 + kSfTy - 1) / kSfTy, ntz = (Z2 + kSfTz - 1) / kSfTz;
    const long long nb2 = (long long)ntx * nty * ntz;
    // every allocation comes before the first launch
    S3D_TRY(h->raw1.reserve(size_t(R1) * kSfC1 * sizeof(float)));
    S3D_TRY(h->part1.reserve(size_t(nb1) * kSfC1 * 2 * sizeof(double)));
    S3D_TRY(h->mr1.reserve(kSfC1 * 2 * sizeof(double)));
    if (out_layer == 2) {
        S3D_TRY(h->raw2.reserve(size_t(R2) * kSfC2 * sizeof(float)));
        S3D_TRY(h->part2.reserve(size_t(nb2) * kSfC2 * 2 * sizeof(double)));
        S3D_TRY(h->mr2.reserve(kSfC2 * 2 * sizeof(double)));
    }
    S3D_TRY(reserve_rows_stats(out_layer == 2 ? kSfC2 : kSfC1, out_layer == 2 ? R2 : R1, 1, kSfGramSpan, h->gpart, h->mpart));
    StageTimer<5>& tm = h->timer;
    tm.timed = false;
    S3D_TRY(tm.mark(0, st));
    const float* raw1 = static_cast<const float*>(h->raw1.p);
    const double* mr1 = static_cast<const double*>(h->mr1.p);
    hipLaunchKernelGGL(k_ssfid_l1, dim3((unsigned)nb1), dim3(kSfThreads), 0, st, vox, X, Y, Z, Y1, Z1, R1, static_cast<const float*>(h->w1T.p),
                       static_cast<const float*>(h->b1.p), static_cast<float*>(h->raw1.p), static_cast<double*>(h->part1.p));
    S3D_HIP(hipGetLastError());
    S3D_TRY(tm.mark(1, st));
    hipLaunchKernelGGL(k_ssfid_mr, dim3(kSfC1), dim3(64), 0, st, static_cast<const double*>(h->part1.p), int(nb1), kSfC1,
                       static_cast<const float*>(h->b1.p), double(R1), static_cast<double*>(h->mr1.p));
    S3D_HIP(hipGetLastError());
    for (int i = 2; i <= 4; ++i) S3D_TRY(tm.mark(i, st));                  // layer 1 alone: stages 2 and 3 are empty
    if (out_layer == 2) {
        hipLaunchKernelGGL(k_ssfid_l2, dim3((unsigned)nb2), dim3(kSfThreads), 0, st, raw1, X1, Y1, Z1, mr1, static_cast<const f32x4*>(h->w2p.p),
                           static_cast<const float*>(h->b2.p), X2, Y2, Z2, nty, ntz, static_cast<float*>(h->raw2.p),
                           static_cast<double*>(h->part2.p));
        S3D_HIP(hipGetLastError());
        S3D_TRY(tm.mark(3, st));
        hipLaunchKernelGGL(k_ssfid_mr, dim3(kSfC2), dim3(64), 0, st, static_cast<const double*>(h->part2.p), int(nb2), kSfC2,
                           static_cast<const float*>(h->b2.p), double(R2), static_cast<double*>(h->mr2.p));
        S3D_HIP(hipGetLastError());
        S3D_TRY(tm.mark(4, st));
        const SfRows<kSfC2> rows{static_cast<const float*>(h->raw2.p), static_cast<const double*>(h->mr2.p), act};
        S3D_TRY(launch_rows_stats<kSfC2>(rows, R2, 1, kSfGramSpan, h->gpart, h->mpart, mu, sigma, st));
    } else {
        const SfRows<kSfC1> rows{raw1, mr1, act};
        S3D_TRY(launch_rows_stats<kSfC1>(rows, R1, 1, kSfGramSpan, h->gpart, h->mpart, mu, sigma, st));
    }
    S3D_TRY(tm.mark(5, st));
    tm.timed = tm.on;
    h->last_layer = out_layer;
    return 0;
}

int s3d_ssfid_profile(s3d_ssfid* h, int on) {
    S3D_CHECK(h, S3D_ERR_INVALID, "ssfid_profile: null handle");
    return h->timer.enable(on != 0);
}

int s3d_ssfid_profile_read(s3d_ssfid* h, double ms[5]) {
    S3D_CHECK(h && ms, S3D_ERR_INVALID, "ssfid_profile_read: null argument");
    S3D_TRY(h->timer.read("ssfid", ms));
    if (h->last_layer == 1) ms[2] = ms[3] = 0.0;
    return 0;
}

}  // extern "C"
