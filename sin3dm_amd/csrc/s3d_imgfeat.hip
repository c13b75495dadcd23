// s3d_imgfeat.hip — the image features of the reference's evaluation/sifid.py and evaluation/lpips.py on the device: the stem of
// Inception-v3 (three or five BasicConv2d units) with the mean and ddof = 1 covariance of its rows, and AlexNet's `features` with
// the unit-normalised maps and the weighted squared differences of every pair of images.  DESIGN.md §23.
//
//   k_if_conv<MODE>  implicit GEMM on mfma_f32_32x32x2f32, channels-last, run-time (KH, KW, stride, pad, Cin, Cout): M = 128 output
//                    pixels of ONE image per block (4 waves x 32), N = 64 output channels, K = taps x Cin in chunks of 16.  A chunk
//                    is one float32 MFMA chain; chains are added in float64 in chunk order.  MODE 1 / 2 form the input from the
//                    uint8 sample with the roundings of sifid.py / lpips.py; out-of-range taps are staged as exact zeros.  The
//                    epilogue applies scale * x + shift (BatchNorm folded in float64, or 1 and the bias), ReLU, and stores once.
//   k_if_pool        MaxPool2d(3, 2), floor mode, no padding
//   IfRows           the last unit's rows as the load of k_rows_gram: the column sums, the C x C Gram and k_rows_cov's mu, sigma
//                    are s3d_rowstats.h's, 1024 rows per block
//   k_if_unit        x * rsqrt(sum_c x^2 + 1e-10) per pixel
//   k_if_pairs       sum over pixels and channels of w_c (xh - yh)^2 for every ordered pair of images of the batch, float64
//   k_if_lpips       partials -> per-layer means and their sum over the five layers
//
// No float atomics; every sum has a fixed order that depends on the shapes alone, so the same input gives the same bits.
#include "s3d_rowstats.h"

#include <algorithm>
#include <cmath>

namespace s3d {

constexpr int kIfThreads = 256;
constexpr int kIfTileM = 128;                         // output pixels per block: 4 waves x 32
constexpr int kIfTileN = 64;                          // output channels per block: two 32-wide MFMA columns per wave
constexpr int kIfChunk = 16;                          // k values per float32 MFMA chain and per LDS stage
constexpr int kIfLd = 20;                             // floats per staged pixel row (16 + 4: 16-byte aligned, rows 20 banks apart)
constexpr int kIfLayers = 5;
constexpr int kIfGramSpan = 1024;                     // rows per block of k_rows_gram
constexpr int kIfPairSlices = 4;                      // blocks per pair of k_if_pairs
constexpr double kIfBnEps = 1e-3;                     // torchvision BasicConv2d: BatchNorm2d(eps = 0.001)
constexpr double kIfUnitEps = 1e-10;                  // lpips.py normalize()
constexpr int kIfMaxDim = 8192;                       // image extent per axis

struct IfConv {
    int H, W, Cin, KH, KW, stride, pad, Ho, Wo, Cout, K, nchunks, nbtot, src_ch, tiles;
};

// The uint8 sample as the first layer's float32 input.  MODE 1, sifid.py: imread gives float32 u / 255, InceptionV3 takes 2 x - 1
// (2 x is exact, one rounding).  MODE 2, lpips.py: u / 255. and (v - 0.5) / 0.5 in float64, the cast to float32, then
// (x - mu) / sigma in float32.
template <int MODE>
__device__ static inline float if_sample(unsigned char u, int ci) {
    if (MODE == 1) {
        const float x = float(u) / 255.0f;
        return 2.0f * x - 1.0f;
    }
    const double v = (double(u) / 255.0 - 0.5) / 0.5;
    const float mu = ci == 0 ? -0.03f : ci == 1 ? -0.088f : -0.188f;
    const float sg = ci == 0 ? 0.458f : ci == 1 ? 0.448f : 0.450f;
    return (float(v) - mu) / sg;
}

// Eight k values (k0 + half * 8 + e) of output pixel (oy, ox) of image `img`; k = (ky * KW + kx) * Cin + ci.
template <int MODE>
__device__ static inline void if_fetch(const void* __restrict__ in, const IfConv& c, long long img, int oy, int ox, bool live, int k0, int half,
                                       float (&v)[8]) {
    if (MODE == 0 && (c.Cin & 15) == 0) {                 // a chunk lies inside one tap: two 16-byte loads
        const int tap = k0 / c.Cin, ci = k0 - tap * c.Cin + half * 8;
        const int ky = tap / c.KW, kx = tap - ky * c.KW;
        const int iy = oy * c.stride - c.pad + ky, ix = ox * c.stride - c.pad + kx;
        const bool ok = live && (unsigned)iy < (unsigned)c.H && (unsigned)ix < (unsigned)c.W;
        f32x4 a = {0.f, 0.f, 0.f, 0.f}, b = {0.f, 0.f, 0.f, 0.f};
        if (ok) {
            const f32x4* p = reinterpret_cast<const f32x4*>(static_cast<const float*>(in) + ((img * c.H + iy) * c.W + ix) * c.Cin + ci);
            a = p[0];
            b = p[1];
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) { v[e] = a[e]; v[4 + e] = b[e]; }
        return;
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int k = k0 + half * 8 + e;
        const int tap = k / c.Cin, ci = k - tap * c.Cin;
        const int ky = tap / c.KW, kx = tap - ky * c.KW;
        const int iy = oy * c.stride - c.pad + ky, ix = ox * c.stride - c.pad + kx;
        const bool ok = live && k < c.K && (unsigned)iy < (unsigned)c.H && (unsigned)ix < (unsigned)c.W;
        float x = 0.f;
        if (ok) {
            const long long pix = (img * c.H + iy) * c.W + ix;
            if (MODE == 0) x = static_cast<const float*>(in)[pix * c.Cin + ci];
            else x = if_sample<MODE>(static_cast<const unsigned char*>(in)[pix * c.src_ch + ci], ci);
        }
        v[e] = x;
    }
}

// wp: the weights in fragment order, eight floats at ((q * nbtot + nbg) * 64 + lane) * 8: element j = w[co = nbg * 32 + lane % 32]
// [k = q * 16 + lane / 32 * 8 + j], zero past K or Cout.  MFMA step j of a chunk contracts k = {j, 8 + j} in that order, so a chain
// runs over k = 0, 8, 1, 9, ... 7, 15 of its chunk whatever the launch shape.  The chain of chunk q - 1 is added to the float64
// accumulators while the MFMAs of chunk q run.  The next chunk's loads are issued before the current chunk's MFMAs; the staged
// pixels are double-buffered in LDS, one barrier per chunk.
template <int MODE>
__global__ void __launch_bounds__(kIfThreads) k_if_conv(const void* __restrict__ in, IfConv c, const f32x4* __restrict__ wp,
                                                        const double* __restrict__ scale, const double* __restrict__ shift,
                                                        float* __restrict__ out) {
    __shared__ float stage[2][kIfTileM * kIfLd];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, half = lane >> 5, m = lane & 31;
    const long long img = blockIdx.x / c.tiles;
    const int p0 = int(blockIdx.x % c.tiles) * kIfTileM;
    const int npix = c.Ho * c.Wo;
    const int n0 = blockIdx.y * kIfTileN;
    const bool two = c.Cout - n0 > 32;
    // staging: thread t brings k = half_s * 8 .. + 7 of pixel p0 + t / 2
    const int sp = t >> 1, half_s = t & 1;
    const int p = p0 + sp;
    const bool live = p < npix;
    const int oy = live ? p / c.Wo : 0, ox = live ? p - oy * c.Wo : 0;
    double acc[2][16];
    f32x16 prev0, prev1;
#pragma unroll
    for (int i = 0; i < 16; ++i) { acc[0][i] = 0.0; acc[1][i] = 0.0; prev0[i] = 0.f; prev1[i] = 0.f; }
    float v[8];
    f32x4 b[4];
    const f32x4* wq = wp + ((size_t)(blockIdx.y * 2) * 64 + lane) * 2;
    const size_t wstep = (size_t)c.nbtot * 64 * 2;
    if_fetch<MODE>(in, c, img, oy, ox, live, 0, half_s, v);
    b[0] = wq[0]; b[1] = wq[1]; b[2] = wq[128]; b[3] = wq[129];
    for (int q = 0; q < c.nchunks; ++q) {
        float* s = stage[q & 1];
        *reinterpret_cast<f32x4*>(s + sp * kIfLd + half_s * 8) = f32x4{v[0], v[1], v[2], v[3]};
        *reinterpret_cast<f32x4*>(s + sp * kIfLd + half_s * 8 + 4) = f32x4{v[4], v[5], v[6], v[7]};
        f32x4 bc[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) bc[i] = b[i];
        __syncthreads();
        if (q + 1 < c.nchunks) {
            if_fetch<MODE>(in, c, img, oy, ox, live, (q + 1) * kIfChunk, half_s, v);
            const f32x4* w1 = wq + (size_t)(q + 1) * wstep;
            b[0] = w1[0]; b[1] = w1[1]; b[2] = w1[128]; b[3] = w1[129];
        }
        const float* ar = s + (wave * 32 + m) * kIfLd + half * 8;
        const f32x4 a0 = *reinterpret_cast<const f32x4*>(ar), a1 = *reinterpret_cast<const f32x4*>(ar + 4);
        f32x16 c0, c1;
#pragma unroll
        for (int i = 0; i < 16; ++i) { c0[i] = 0.f; c1[i] = 0.f; }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float a = j < 4 ? a0[j & 3] : a1[j & 3];
            c0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, j < 4 ? bc[0][j & 3] : bc[1][j & 3], c0, 0, 0, 0);
            if (two) c1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, j < 4 ? bc[2][j & 3] : bc[3][j & 3], c1, 0, 0, 0);
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) { acc[0][i] += double(prev0[i]); acc[1][i] += double(prev1[i]); }
        prev0 = c0;
        prev1 = c1;
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) { acc[0][i] += double(prev0[i]); acc[1][i] += double(prev1[i]); }
    // register i of lane (m, half) is pixel p0 + wave * 32 + (i % 4) + 8 * (i / 4) + 4 * half, channel n0 + nb * 32 + m
#pragma unroll
    for (int nb = 0; nb < 2; ++nb) {
        const int co = n0 + nb * 32 + m;
        if (co >= c.Cout) continue;
        const double sc = scale[co], sh = shift[co];
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int po = p0 + wave * 32 + (i & 3) + 8 * (i >> 2) + 4 * half;
            if (po < npix) {
                const float y = float(fma(acc[nb][i], sc, sh));
                out[(img * npix + po) * c.Cout + co] = y > 0.f ? y : 0.f;
            }
        }
    }
}

// ------------------------------------------------------------------ MaxPool2d(3, 2)
// One thread per output pixel and four channels; total = n * Ho * Wo * C / 4.
__global__ void __launch_bounds__(kIfThreads) k_if_pool(const float* __restrict__ in, int H, int W, int C, int Ho, int Wo, long long total,
                                                        float* __restrict__ out) {
    const long long i = (long long)blockIdx.x * kIfThreads + threadIdx.x;
    if (i >= total) return;
    const int cq = C / 4;
    const int c4 = int(i % cq);
    const long long pix = i / cq;
    const int ox = int(pix % Wo), oy = int((pix / Wo) % Ho);
    const long long img = pix / ((long long)Wo * Ho);
    f32x4 best = *reinterpret_cast<const f32x4*>(in + ((img * H + 2 * oy) * W + 2 * ox) * C + c4 * 4);
#pragma unroll
    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
            const f32x4 x = *reinterpret_cast<const f32x4*>(in + ((img * H + 2 * oy + ky) * W + 2 * ox + kx) * C + c4 * 4);
#pragma unroll
            for (int e = 0; e < 4; ++e) best[e] = x[e] > best[e] ? x[e] : best[e];
        }
    *reinterpret_cast<f32x4*>(out + pix * C + c4 * 4) = best;
}

// ------------------------------------------------------------------ the rows of the last unit: the Load of k_rows_gram
template <int C>
struct IfRows {
    const float* act;                                     // [n][R][C]
    long long R;
    __device__ void bind(int) {}
    __device__ f32x4 operator()(long long img, long long row, int cq) const {
        return *reinterpret_cast<const f32x4*>(act + (img * R + row) * C + cq * 4);
    }
};

// ------------------------------------------------------------------ LPIPS head
// One wave per pixel: lane l adds x_c^2 for c = l, l + 64, ... in float64, a fixed xor tree, then x * (s + 1e-10)^(-1/2).
__global__ void __launch_bounds__(kIfThreads) k_if_unit(const float* __restrict__ x, long long npix, int C, float* __restrict__ u) {
    const long long pix = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (pix >= npix) return;
    double s = 0.0;
    for (int c = lane; c < C; c += 64) {
        const double v = double(x[pix * C + c]);
        s = fma(v, v, s);
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off);
    const double r = 1.0 / sqrt(s + kIfUnitEps);
    for (int c = lane; c < C; c += 64) u[pix * C + c] = float(double(x[pix * C + c]) * r);
}

// Block (pair = i * n + j, slice): thread t adds w_c d^2, d = xh_i - xh_j in float32 as the reference subtracts, over the float4
// lo + t, lo + t + 256, ... of its slice in float64 (per_img is a multiple of 4 and below 2^31); then a fixed tree over the block.
// i == j gives exactly 0, and (i, j) and (j, i) the same bits.
__global__ void __launch_bounds__(kIfThreads) k_if_pairs(const float* __restrict__ u, int n, long long per_img, int C, const float* __restrict__ w,
                                                         double* __restrict__ part) {
    __shared__ double red[kIfThreads];
    const int t = threadIdx.x;
    const int i = blockIdx.x / n, j = blockIdx.x % n;
    const unsigned n4 = unsigned(per_img / 4), len = (n4 + kIfPairSlices - 1) / kIfPairSlices;
    const unsigned lo = blockIdx.y * len, hi = min(n4, lo + len);
    const f32x4* a = reinterpret_cast<const f32x4*>(u + i * per_img);
    const f32x4* b = reinterpret_cast<const f32x4*>(u + j * per_img);
    double s = 0.0;
    for (unsigned e = lo + t; e < hi; e += kIfThreads) {
        const f32x4 x = a[e], y = b[e];
        const f32x4 w4 = *reinterpret_cast<const f32x4*>(w + (e * 4u) % unsigned(C));
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float d = x[k] - y[k];
            s = fma(double(w4[k]), double(d) * double(d), s);
        }
    }
    red[t] = s;
    __syncthreads();
    for (int off = kIfThreads / 2; off >= 1; off >>= 1) {
        if (t < off) red[t] += red[t + off];
        __syncthreads();
    }
    if (t == 0) part[(long long)blockIdx.x * kIfPairSlices + blockIdx.y] = red[0];
}

// One thread per pair: the slices in order, the mean over the layer's pixels, the five layers in order.
struct IfLpipsFin { double npix[kIfLayers]; };
__global__ void __launch_bounds__(kIfThreads) k_if_lpips(const double* __restrict__ part, int npairs, IfLpipsFin f, double* __restrict__ layers,
                                                         double* __restrict__ total) {
    const int pr = blockIdx.x * kIfThreads + threadIdx.x;
    if (pr >= npairs) return;
    double sum = 0.0;
    for (int l = 0; l < kIfLayers; ++l) {
        double s = 0.0;
        for (int k = 0; k < kIfPairSlices; ++k) s += part[((long long)l * npairs + pr) * kIfPairSlices + k];
        s /= f.npix[l];
        if (layers) layers[(long long)l * npairs + pr] = s;
        sum += s;
    }
    total[pr] = sum;
}

struct IfLayerDef { const char* name; int cin, cout, k, stride, pad; bool pool_before; };
static const IfLayerDef kIfNets[2][kIfLayers] = {
    {{"Conv2d_1a_3x3", 3, 32, 3, 2, 0, false}, {"Conv2d_2a_3x3", 32, 32, 3, 1, 0, false}, {"Conv2d_2b_3x3", 32, 64, 3, 1, 1, false},
     {"Conv2d_3b_1x1", 64, 80, 1, 1, 0, true}, {"Conv2d_4a_3x3", 80, 192, 3, 1, 0, false}},
    {{"features.0", 3, 64, 11, 4, 2, false}, {"features.3", 64, 192, 5, 1, 2, true}, {"features.6", 192, 384, 3, 1, 1, true},
     {"features.8", 384, 256, 3, 1, 1, false}, {"features.10", 256, 256, 3, 1, 1, false}},
};
// the parameters of a layer: the Inception units' {conv.weight, bn.weight, bn.bias, bn.running_mean, bn.running_var}, AlexNet's
// {weight, bias} and the LPIPS linear layer of that map
static const char* const kIfSuffix[2][5] = {{".conv.weight", ".bn.weight", ".bn.bias", ".bn.running_mean", ".bn.running_var"},
                                            {".weight", ".bias", nullptr, nullptr, nullptr}};
constexpr int kIfNumParams[2] = {5, 2};

}  // namespace s3d

using namespace s3d;

struct s3d_imgfeat {
    int net = 0;
    std::vector<float> host[kIfLayers][5], lin[kIfLayers];
    bool have[kIfLayers][5] = {}, have_lin[kIfLayers] = {};
    bool packed = false, lin_packed = false;
    DevBuf wp[kIfLayers], scale[kIfLayers], shift[kIfLayers], linw[kIfLayers];
    DevBuf out[kIfLayers], unit[kIfLayers], pool, gpart, mpart, ppart;
    // the last s3d_imgfeat_features call: what the statistics and the pairs are taken of
    int n = 0, nlayers = 0, hw[kIfLayers][2] = {};
    StageTimer<kIfLayers + 1> timer;     // s3d_imgfeat_profile: the five units, the unit normalisation
};

static int imgfeat_pack(s3d_imgfeat* h) {
    for (int l = 0; l < kIfLayers; ++l) {
        const IfLayerDef& d = kIfNets[h->net][l];
        const int K = d.k * d.k * d.cin, nchunks = (K + kIfChunk - 1) / kIfChunk, nbtot = 2 * ((d.cout + kIfTileN - 1) / kIfTileN);
        std::vector<float> wp(size_t(nchunks) * nbtot * 64 * 8, 0.f);
        const std::vector<float>& w = h->host[l][0];
        for (int q = 0; q < nchunks; ++q)
            for (int nbg = 0; nbg < nbtot; ++nbg)
                for (int lane = 0; lane < 64; ++lane)
                    for (int j = 0; j < 8; ++j) {
                        const int k = q * kIfChunk + (lane >> 5) * 8 + j, co = nbg * 32 + (lane & 31);
                        if (k >= K || co >= d.cout) continue;
                        const int tap = k / d.cin, ci = k % d.cin;
                        wp[((size_t(q) * nbtot + nbg) * 64 + lane) * 8 + j] = w[(size_t(co) * d.cin + ci) * d.k * d.k + tap];
                    }
        std::vector<double> sc(d.cout), sh(d.cout);
        for (int c = 0; c < d.cout; ++c) {
            if (h->net == S3D_IMGFEAT_INCEPTION) {
                sc[c] = double(h->host[l][1][c]) / sqrt(double(h->host[l][4][c]) + kIfBnEps);
                sh[c] = double(h->host[l][2][c]) - double(h->host[l][3][c]) * sc[c];
            } else {
                sc[c] = 1.0;
                sh[c] = double(h->host[l][1][c]);
            }
        }
        S3D_TRY(upload(h->wp[l], wp.data(), wp.size() * sizeof(float)));
        S3D_TRY(upload(h->scale[l], sc.data(), sc.size() * sizeof(double)));
        S3D_TRY(upload(h->shift[l], sh.data(), sh.size() * sizeof(double)));
    }
    h->packed = true;
    return 0;
}

extern "C" {

int s3d_imgfeat_create(int net, s3d_imgfeat** out) {
    S3D_CHECK(out, S3D_ERR_INVALID, "imgfeat_create: null argument");
    S3D_CHECK(net == S3D_IMGFEAT_INCEPTION || net == S3D_IMGFEAT_ALEXNET, S3D_ERR_UNSUPPORTED,
              "imgfeat_create: network %d; 0 (the Inception-v3 stem) and 1 (AlexNet features) are built", net);
    *out = new s3d_imgfeat();
    (*out)->net = net;
    return 0;
}
void s3d_imgfeat_destroy(s3d_imgfeat* h) { delete h; }

int s3d_imgfeat_set_param(s3d_imgfeat* h, const char* name, const float* data, const int64_t* shape, int ndim) {
    S3D_CHECK(h && name && data && shape, S3D_ERR_INVALID, "imgfeat set_param: null argument");
    for (int l = 0; l < kIfLayers; ++l) {
        const IfLayerDef& d = kIfNets[h->net][l];
        int64_t want[4] = {0, 0, 0, 0};
        int wdim = 0, slot = -1;
        const size_t len = strlen(d.name);
        if (strncmp(name, d.name, len) == 0) {
            for (int p = 0; p < kIfNumParams[h->net]; ++p)
                if (strcmp(name + len, kIfSuffix[h->net][p]) == 0) slot = p;
        }
        if (slot == 0) { wdim = 4; want[0] = d.cout; want[1] = d.cin; want[2] = want[3] = d.k; }
        if (slot > 0) { wdim = 1; want[0] = d.cout; }
        if (slot < 0 && h->net == S3D_IMGFEAT_ALEXNET) {
            char lname[64];
            snprintf(lname, sizeof lname, "lpips_weights.%d.main.1.weight", l);
            if (strcmp(name, lname) == 0) { slot = 5; wdim = 4; want[0] = 1; want[1] = d.cout; want[2] = want[3] = 1; }
        }
        if (slot < 0) continue;
        size_t n;
        S3D_TRY(check_param_shape("imgfeat", name, shape, ndim, want, wdim,
                                  h->net == S3D_IMGFEAT_INCEPTION ? "torchvision's inception_v3 is the network supported"
                                                                  : "torchvision's alexnet is the network supported", n));
        if (slot == 5) {
            h->lin[l].assign(data, data + n);
            h->have_lin[l] = true;
            h->lin_packed = false;
        } else {
            h->host[l][slot].assign(data, data + n);
            h->have[l][slot] = true;
            h->packed = false;
        }
        return 0;
    }
    set_error("imgfeat set_param: unexpected key '%s'", name);
    return S3D_ERR_INVALID;
}

int s3d_imgfeat_out_dims(int net, int H, int W, int dims, int* nlayers, int hw[5][2], int channels[5]) {
    S3D_CHECK(net == S3D_IMGFEAT_INCEPTION || net == S3D_IMGFEAT_ALEXNET, S3D_ERR_UNSUPPORTED, "imgfeat: network %d is not built", net);
    S3D_CHECK(nlayers, S3D_ERR_INVALID, "imgfeat_out_dims: null argument");
    int nl = kIfLayers;
    if (net == S3D_IMGFEAT_INCEPTION) {
        S3D_CHECK(dims == 64 || dims == 192, S3D_ERR_UNSUPPORTED,
                  "sifid: dims %d is not built; 64 and 192 (the two the reference's eval_full.py takes) are", dims);
        nl = dims == 64 ? 3 : 5;
    }
    S3D_CHECK(H >= 1 && W >= 1, S3D_ERR_INVALID, "imgfeat: an image of %d x %d", H, W);
    S3D_CHECK(H <= kIfMaxDim && W <= kIfMaxDim, S3D_ERR_UNSUPPORTED, "imgfeat: an image of %d x %d, %d per axis at most", H, W, kIfMaxDim);
    int e[2] = {H, W};
    for (int l = 0; l < nl; ++l) {
        const IfLayerDef& d = kIfNets[net][l];
        for (int a = 0; a < 2; ++a) {
            if (d.pool_before) e[a] = e[a] >= 3 ? (e[a] - 3) / 2 + 1 : 0;
            e[a] = e[a] >= 1 && e[a] + 2 * d.pad >= d.k ? (e[a] + 2 * d.pad - d.k) / d.stride + 1 : 0;
            S3D_CHECK(e[a] >= 1, S3D_ERR_INVALID, "imgfeat: an image of %d x %d is too small: nothing is left at %s", H, W, d.name);
            if (hw) hw[l][a] = e[a];
        }
        if (channels) channels[l] = d.cout;
    }
    // AlexNet's features end in MaxPool2d(3, 2); its output is unused, but the reference raises where it would be empty
    if (net == S3D_IMGFEAT_ALEXNET)
        S3D_CHECK(e[0] >= 3 && e[1] >= 3, S3D_ERR_INVALID,
                  "lpips: an image of %d x %d is too small: AlexNet's last feature map is %d x %d and its final MaxPool2d(3, 2) needs 3 x 3", H,
                  W, e[0], e[1]);
    *nlayers = nl;
    return 0;
}

int s3d_imgfeat_features(s3d_imgfeat* h, const uint8_t* img, int n, int H, int W, int ch, int dims, float* const* acts, void* stream) {
    S3D_CHECK(h && img, S3D_ERR_INVALID, "imgfeat_features: null argument");
    S3D_CHECK(n >= 1 && n <= 4096, S3D_ERR_INVALID, "imgfeat_features: a batch of %d images", n);
    S3D_CHECK(ch == 3 || ch == 4, S3D_ERR_INVALID, "imgfeat_features: %d channels per sample; RGB or RGBA", ch);
    int nl = 0, hw[kIfLayers][2];
    S3D_TRY(s3d_imgfeat_out_dims(h->net, H, W, dims, &nl, hw, nullptr));
    for (int l = 0; l < nl; ++l)
        for (int p = 0; p < kIfNumParams[h->net]; ++p)
            S3D_CHECK(h->have[l][p], S3D_ERR_INVALID, "imgfeat_features: %s%s has not been set", kIfNets[h->net][l].name, kIfSuffix[h->net][p]);
    if (!h->packed) S3D_TRY(imgfeat_pack(h));
    hipStream_t st = static_cast<hipStream_t>(stream);
    // every allocation comes before the first launch
    size_t pool_bytes = 0;
    {
        int e[2] = {H, W};
        for (int l = 0; l < nl; ++l) {
            const IfLayerDef& d = kIfNets[h->net][l];
            if (d.pool_before) pool_bytes = std::max(pool_bytes, size_t(n) * ((e[0] - 3) / 2 + 1) * ((e[1] - 3) / 2 + 1) * d.cin * sizeof(float));
            e[0] = hw[l][0];
            e[1] = hw[l][1];
            const size_t bytes = size_t(n) * hw[l][0] * hw[l][1] * d.cout * sizeof(float);
            S3D_TRY(h->out[l].reserve(bytes));
            if (h->net == S3D_IMGFEAT_ALEXNET) S3D_TRY(h->unit[l].reserve(bytes));
        }
        if (pool_bytes) S3D_TRY(h->pool.reserve(pool_bytes));
    }
    StageTimer<kIfLayers + 1>& tm = h->timer;
    tm.timed = false;
    h->nlayers = 0;
    const void* cur = img;
    int e[2] = {H, W};
    S3D_TRY(tm.mark(0, st));
    for (int l = 0; l < nl; ++l) {
        const IfLayerDef& d = kIfNets[h->net][l];
        if (d.pool_before) {
            const int ho = (e[0] - 3) / 2 + 1, wo = (e[1] - 3) / 2 + 1;
            const long long total = (long long)n * ho * wo * (d.cin / 4);
            hipLaunchKernelGGL(k_if_pool, dim3((unsigned)((total + kIfThreads - 1) / kIfThreads)), dim3(kIfThreads), 0, st,
                               static_cast<const float*>(cur), e[0], e[1], d.cin, ho, wo, total, static_cast<float*>(h->pool.p));
            S3D_HIP(hipGetLastError());
            cur = h->pool.p;
            e[0] = ho;
            e[1] = wo;
        }
        IfConv c;
        c.H = e[0]; c.W = e[1]; c.Cin = d.cin; c.KH = c.KW = d.k; c.stride = d.stride; c.pad = d.pad;
        c.Ho = hw[l][0]; c.Wo = hw[l][1]; c.Cout = d.cout; c.K = d.k * d.k * d.cin;
        c.nchunks = (c.K + kIfChunk - 1) / kIfChunk;
        c.nbtot = 2 * ((d.cout + kIfTileN - 1) / kIfTileN);
        c.src_ch = ch;
        c.tiles = (c.Ho * c.Wo + kIfTileM - 1) / kIfTileM;
        const dim3 grid((unsigned)(n * c.tiles), (unsigned)((d.cout + kIfTileN - 1) / kIfTileN));
        const f32x4* wp = static_cast<const f32x4*>(h->wp[l].p);
        const double* sc = static_cast<const double*>(h->scale[l].p);
        const double* sh = static_cast<const double*>(h->shift[l].p);
        float* o = static_cast<float*>(h->out[l].p);
        if (l > 0) hipLaunchKernelGGL(k_if_conv<0>, grid, dim3(kIfThreads), 0, st, cur, c, wp, sc, sh, o);
        else if (h->net == S3D_IMGFEAT_INCEPTION) hipLaunchKernelGGL(k_if_conv<1>, grid, dim3(kIfThreads), 0, st, cur, c, wp, sc, sh, o);
        else hipLaunchKernelGGL(k_if_conv<2>, grid, dim3(kIfThreads), 0, st, cur, c, wp, sc, sh, o);
        S3D_HIP(hipGetLastError());
        S3D_TRY(tm.mark(l + 1, st));
        cur = o;
        e[0] = hw[l][0];
        e[1] = hw[l][1];
        if (acts && acts[l])
            S3D_HIP(hipMemcpyAsync(acts[l], o, size_t(n) * e[0] * e[1] * d.cout * sizeof(float), hipMemcpyDeviceToDevice, st));
    }
    for (int l = nl; l < kIfLayers; ++l) S3D_TRY(tm.mark(l + 1, st));
    if (h->net == S3D_IMGFEAT_ALEXNET)
        for (int l = 0; l < nl; ++l) {
            const long long npix = (long long)n * hw[l][0] * hw[l][1];
            hipLaunchKernelGGL(k_if_unit, dim3((unsigned)((npix + 3) / 4)), dim3(kIfThreads), 0, st, static_cast<const float*>(h->out[l].p), npix,
                               kIfNets[h->net][l].cout, static_cast<float*>(h->unit[l].p));
            S3D_HIP(hipGetLastError());
        }
    S3D_TRY(tm.mark(kIfLayers + 1, st));
    tm.timed = tm.on;
    h->n = n;
    h->nlayers = nl;
    memcpy(h->hw, hw, sizeof hw);
    return 0;
}

int s3d_imgfeat_stats(s3d_imgfeat* h, double* mu, double* sigma, void* stream) {
    S3D_CHECK(h && mu && sigma, S3D_ERR_INVALID, "imgfeat_stats: null argument");
    S3D_CHECK(h->net == S3D_IMGFEAT_INCEPTION, S3D_ERR_INVALID, "imgfeat_stats: the statistics are taken of the Inception stem");
    S3D_CHECK(h->nlayers > 0, S3D_ERR_INVALID, "imgfeat_stats: no features have been computed (s3d_imgfeat_features first)");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int l = h->nlayers - 1, C = kIfNets[h->net][l].cout;
    const long long R = (long long)h->hw[l][0] * h->hw[l][1];
    const float* act = static_cast<const float*>(h->out[l].p);
    if (C == 64) return launch_rows_stats<64>(IfRows<64>{act, R}, R, h->n, kIfGramSpan, h->gpart, h->mpart, mu, sigma, st);
    return launch_rows_stats<192>(IfRows<192>{act, R}, R, h->n, kIfGramSpan, h->gpart, h->mpart, mu, sigma, st);
}

int s3d_imgfeat_pairs(s3d_imgfeat* h, double* layers, double* total, void* stream) {
    S3D_CHECK(h && total, S3D_ERR_INVALID, "imgfeat_pairs: null argument");
    S3D_CHECK(h->net == S3D_IMGFEAT_ALEXNET, S3D_ERR_INVALID, "imgfeat_pairs: the pair distances are taken of AlexNet's features");
    S3D_CHECK(h->nlayers == kIfLayers, S3D_ERR_INVALID, "imgfeat_pairs: no features have been computed (s3d_imgfeat_features first)");
    for (int l = 0; l < kIfLayers; ++l) S3D_CHECK(h->have_lin[l], S3D_ERR_INVALID, "imgfeat_pairs: lpips_weights.%d.main.1.weight has not been set", l);
    if (!h->lin_packed) {
        for (int l = 0; l < kIfLayers; ++l) S3D_TRY(upload(h->linw[l], h->lin[l].data(), h->lin[l].size() * sizeof(float)));
        h->lin_packed = true;
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int n = h->n, npairs = n * n;
    S3D_TRY(h->ppart.reserve(size_t(kIfLayers) * npairs * kIfPairSlices * sizeof(double)));
    double* part = static_cast<double*>(h->ppart.p);
    IfLpipsFin fin;
    for (int l = 0; l < kIfLayers; ++l) {
        const int C = kIfNets[h->net][l].cout;
        const long long npix = (long long)h->hw[l][0] * h->hw[l][1];
        fin.npix[l] = double(npix);
        S3D_CHECK(npix * C < (1LL << 31), S3D_ERR_UNSUPPORTED, "imgfeat_pairs: a feature map of %lld values", npix * C);
        hipLaunchKernelGGL(k_if_pairs, dim3((unsigned)npairs, kIfPairSlices), dim3(kIfThreads), 0, st, static_cast<const float*>(h->unit[l].p), n,
                           npix * C, C, static_cast<const float*>(h->linw[l].p), part + (size_t)l * npairs * kIfPairSlices);
        S3D_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(k_if_lpips, dim3((unsigned)((npairs + kIfThreads - 1) / kIfThreads)), dim3(kIfThreads), 0, st, part, npairs, fin, layers,
                       total);
    S3D_HIP(hipGetLastError());
    return 0;
}

int s3d_imgfeat_profile(s3d_imgfeat* h, int on) {
    S3D_CHECK(h, S3D_ERR_INVALID, "imgfeat_profile: null handle");
    return h->timer.enable(on != 0);
}

int s3d_imgfeat_profile_read(s3d_imgfeat* h, double ms[6]) {
    S3D_CHECK(h && ms, S3D_ERR_INVALID, "imgfeat_profile_read: null argument");
    return h->timer.read("imgfeat", ms);
}

}  // extern "C"
