// s3d_decoder.hip — AutoEncoderGroupSkip.decode on MI355X (src/encoding/networks.py:192-220).
//
// Two stages:
//  (1) prepare_triplane: the per-plane TriplaneGroupResnetBlock (conv5x5 -> InstanceNorm -> SiLU -> conv5x5 + 1x1
//      shortcut, src/encoding/blocks.py:189-256) for the geo and tex feature groups, run ONCE per triplane on the
//      MFMA convolution of s3d_conv.hip (the reference recomputes it for every 16 384-point chunk,
//      src/encoding/model.py:327-330; the result does not depend on the points).
//  (2) decode: one fused kernel per 128 points — bilinear border-clamped gather of the three feature planes
//      (F.grid_sample semantics, networks.py:182-190) straight into MFMA operand registers, then every
//      head's DecoderMLPSkipConcat chain (blocks.py:65-91) on the fp32 matrix cores without the activations ever
//      leaving the register file:
//        * the GEMM is evaluated transposed, D[hidden unit][point] = W · Xᵀ, so a layer's accumulator (lane =
//          point, registers = 16 hidden rows of a 32-row tile) IS the next layer's B operand: row order
//          (r&3) + 8(r>>2) + 4(lane>>5) is exactly the k-permutation "lane half 0 takes k0..3, half 1 k4..7" that
//          lets the weight operand be fetched with one ds_read_b128 per 4 MFMAs;
//        * weights stream through LDS in [rows][32 k] slabs shared by the block's 4 waves (each wave = 32 points),
//          register-prefetched one slab ahead, one barrier per slab.
//      Bound: fp32 MFMA (1.18 MFLOP per point, 16 B written per point).
// Every network runs the same point kernel (s3d_decoder_create_variant: geometry only, AutoEncoderGroupPBR, up to 8 texture
// channels): the chains are organised as feature groups that each carry a list of heads (DecodeArgs), and the skip net with
// texture is the table {geo: [sdf]}, {tex: [tex_channels, sigmoid]}.
#include <algorithm>
#include <cmath>
#include <memory>

#include "s3d_ae.h"
#include "s3d_aenet.h"

namespace s3d {

static inline int rup32(int v) { return (v + 31) / 32 * 32; }

// ------------------------------------------------------------------ small kernels of the plane block
// channels [c0, c0+cin) of an NCHW [1][Ctot][h][w] plane -> NHWC [h][w][32] zero-padded
__global__ void k_slice_pad(const float* __restrict__ in, float* __restrict__ out, int hw, int c0, int cin) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)hw * 32) return;
    const int c = int(i & 31);
    const long long pix = i >> 5;
    out[i] = c < cin ? in[size_t(c0 + c) * hw + pix] : 0.f;
}
// channels [0, up) of an NHWC [h][w][C] plane -> NCHW [up][h][w]  (s3d_decoder_plane_features)
__global__ void k_plane_to_nchw(const float* __restrict__ in, float* __restrict__ out, long long hw, int C, int up) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= hw * up) return;
    const long long pix = i % hw;
    const int c = int(i / hw);
    out[i] = in[pix * C + c];
}

// InstanceNorm2d(C, eps=1e-6, affine) + SiLU over one NHWC plane [hw][C]  (src/encoding/blocks.py:219-221, 94-96), in two
// launches: per-chunk partial sums in double (kInNormChunks chunks of pixels), then statistics + apply.
// block: C/4 quads x pl pixel lanes, chunk = blockIdx.x; part[chunk][C][2] = {sum, sum of squares}; sm: pl*C*2 doubles of LDS
__device__ __forceinline__ void chan_partials(const float* __restrict__ x, double* __restrict__ part, int hw, int C, double* sm) {
    const int cq = C / 4, pl = blockDim.x / cq;
    const int q = threadIdx.x % cq, l = threadIdx.x / cq;
    const int per = (hw + kInNormChunks - 1) / kInNormChunks;
    const int p0 = blockIdx.x * per, p1 = min(hw, p0 + per);
    double s[4] = {0, 0, 0, 0}, ss[4] = {0, 0, 0, 0};
    for (int pix = p0 + l; pix < p1; pix += pl) {
        const float4 v = reinterpret_cast<const float4*>(x)[size_t(pix) * cq + q];
        s[0] += v.x; ss[0] += double(v.x) * v.x; s[1] += v.y; ss[1] += double(v.y) * v.y;
        s[2] += v.z; ss[2] += double(v.z) * v.z; s[3] += v.w; ss[3] += double(v.w) * v.w;
    }
    for (int k = 0; k < 4; ++k) { sm[(size_t(l) * C + 4 * q + k) * 2] = s[k]; sm[(size_t(l) * C + 4 * q + k) * 2 + 1] = ss[k]; }
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += blockDim.x) {
        double S = 0, SS = 0;
        for (int ll = 0; ll < pl; ++ll) { S += sm[(size_t(ll) * C + c) * 2]; SS += sm[(size_t(ll) * C + c) * 2 + 1]; }
        part[(size_t(blockIdx.x) * C + c) * 2] = S; part[(size_t(blockIdx.x) * C + c) * 2 + 1] = SS;
    }
}
// per-channel scale = gamma * rstd and shift = beta - scale * mean from the chunk partials, in double
__device__ __forceinline__ void scale_shift_from_partials(const double* __restrict__ part, const float* __restrict__ gamma,
                                                          const float* __restrict__ beta, float* A, float* Bc, int hw, int C, float eps) {
    for (int c = threadIdx.x; c < C; c += blockDim.x) {
        double S = 0, SS = 0;
        for (int k = 0; k < kInNormChunks; ++k) { S += part[(size_t(k) * C + c) * 2]; SS += part[(size_t(k) * C + c) * 2 + 1]; }
        const double m = S / hw;
        double var = SS / hw - m * m; if (var < 0) var = 0;
        const float scale = float(1.0 / sqrt(var + double(eps))) * gamma[c];
        A[c] = scale; Bc[c] = beta[c] - scale * float(m);
    }
}
// xn = x * A + Bc per channel and y = SiLU(xn) over the blocks of grid dimension x; xn is stored only when KEEP
template <bool KEEP>
__device__ __forceinline__ void inorm_apply(const float* __restrict__ x, const float* A, const float* Bc, float* __restrict__ xn,
                                            float* __restrict__ y, int hw, int C) {
    const int cq = C / 4;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < (long long)hw * cq; i += (long long)gridDim.x * blockDim.x) {
        const int q = int(i % cq);
        const float4 v = reinterpret_cast<const float4*>(x)[i];
        const float4 a = reinterpret_cast<const float4*>(A)[q], b = reinterpret_cast<const float4*>(Bc)[q];
        float4 n, o;
        n.x = fmaf(v.x, a.x, b.x); n.y = fmaf(v.y, a.y, b.y); n.z = fmaf(v.z, a.z, b.z); n.w = fmaf(v.w, a.w, b.w);
        o.x = n.x / (1.f + expf(-n.x)); o.y = n.y / (1.f + expf(-n.y)); o.z = n.z / (1.f + expf(-n.z)); o.w = n.w / (1.f + expf(-n.w));
        if (KEEP) reinterpret_cast<float4*>(xn)[i] = n;
        reinterpret_cast<float4*>(y)[i] = o;
    }
}
template <bool KEEP>
__device__ __forceinline__ void inorm_silu(const float* __restrict__ x, const double* __restrict__ part, const float* __restrict__ gamma,
                                           const float* __restrict__ beta, float* __restrict__ xn, float* __restrict__ y, int hw, int C,
                                           float eps, float* A) {
    scale_shift_from_partials(part, gamma, beta, A, A + C, hw, C, eps);
    __syncthreads();
    inorm_apply<KEEP>(x, A, A + C, xn, y, hw, C);
}

__global__ void k_chan_partials(const float* __restrict__ x, double* __restrict__ part, int hw, int C) {      // grid (kInNormChunks)
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    chan_partials(x, part, hw, C, reinterpret_cast<double*>(smem_raw));
}
__global__ void k_inorm_silu(const float* __restrict__ x, const double* __restrict__ part, const float* __restrict__ gamma,
                             const float* __restrict__ beta, float* __restrict__ y, int hw, int C, float eps) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    inorm_silu<false>(x, part, gamma, beta, nullptr, y, hw, C, eps, reinterpret_cast<float*>(smem_raw));
}
// The PBR texture branch's second block normalises its INPUT (blocks.py:238-239) and adds that normalised input back as the
// residual: k_inorm_silu with both results kept, xn = IN(x) and y = SiLU(xn).
__global__ void k_inorm_keep(const float* __restrict__ x, const double* __restrict__ part, const float* __restrict__ gamma,
                             const float* __restrict__ beta, float* __restrict__ xn, float* __restrict__ y, int hw, int C, float eps) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    inorm_silu<true>(x, part, gamma, beta, xn, y, hw, C, eps, reinterpret_cast<float*>(smem_raw));
}

// The auto-encoder training tier's form (round 5): three planes per launch (blockIdx.y), the statistics finished by their own
// small launch between the two (launch_mr_from_partials3, s3d_ae_kernels.hip — every block of the apply pass used to walk the 64
// chunk records of its channels itself, 10 of its 18 us); scale and shift are formed in float from those {mean, rstd}
struct InNorm3Args { const float* x[3]; float* y[3]; double* part[3]; const float* gamma[3]; const float* beta[3]; const float* mr; int hw[3]; int C; };
__global__ void k_chan_partials3(InNorm3Args a) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const int p = blockIdx.y;
    chan_partials(a.x[p], a.part[p], a.hw[p], a.C, reinterpret_cast<double*>(smem_raw));
}
__global__ void k_inorm_silu3(InNorm3Args a) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const int p = blockIdx.y, C = a.C;
    float* A = reinterpret_cast<float*>(smem_raw); float* Bc = A + C;
    for (int c = threadIdx.x; c < C; c += blockDim.x) {
        const float m = a.mr[(size_t(p) * C + c) * 2], scale = a.mr[(size_t(p) * C + c) * 2 + 1] * a.gamma[p][c];
        A[c] = scale; Bc[c] = a.beta[p][c] - scale * m;
    }
    __syncthreads();
    inorm_apply<false>(a.x[p], A, Bc, nullptr, a.y[p], a.hw[p], C);
}
// ... and k_inorm_keep's: the normalised maps stored beside their SiLU (the training tier's tex_convs.1 of the PBR net).  (The
// scale / shift loop is written out in both kernels: as a shared __device__ helper it compiled to other instructions in both.)
struct InNormKeep3Args { InNorm3Args n; float* xn[3]; };
__global__ __launch_bounds__(256) void k_inorm_keep3(InNormKeep3Args k) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const InNorm3Args& a = k.n;
    const int p = blockIdx.y, C = a.C;
    float* A = reinterpret_cast<float*>(smem_raw); float* Bc = A + C;
    for (int c = threadIdx.x; c < C; c += blockDim.x) {
        const float m = a.mr[(size_t(p) * C + c) * 2], scale = a.mr[(size_t(p) * C + c) * 2 + 1] * a.gamma[p][c];
        A[c] = scale; Bc[c] = a.beta[p][c] - scale * m;
    }
    __syncthreads();
    inorm_apply<true>(a.x[p], A, Bc, k.xn[p], a.y[p], a.hw[p], C);
}
// xn null: the normalised maps are not kept (k_inorm_silu3)
int launch_inorm_keep3(float* const x[3], double* const part[3], const float* const gamma[3], const float* const beta[3], float* const xn[3],
                       float* const y[3], const size_t hw[3], int C, float eps, float* mr, hipStream_t st) {
    InNormKeep3Args k; InNorm3Args& a = k.n; a.C = C; a.mr = mr;
    int mx = 0;
    for (int p = 0; p < 3; ++p) {
        a.x[p] = x[p]; a.y[p] = y[p]; a.part[p] = part[p]; a.gamma[p] = gamma[p]; a.beta[p] = beta[p]; a.hw[p] = int(hw[p]);
        k.xn[p] = xn ? xn[p] : nullptr;
        mx = std::max(mx, a.hw[p]);
    }
    const int cq = C / 4, pl = std::max(1, 256 / cq);
    hipLaunchKernelGGL(k_chan_partials3, dim3(kInNormChunks, 3), dim3(cq * pl), size_t(pl) * C * 2 * sizeof(double), st, a);
    S3D_HIP(hipGetLastError());
    S3D_TRY(launch_mr_from_partials3(part, kInNormChunks, C, hw, eps, mr, st));
    const dim3 grid(std::min(1024, (mx * cq + 255) / 256), 3);
    if (xn) hipLaunchKernelGGL(k_inorm_keep3, grid, dim3(256), size_t(2) * C * sizeof(float), st, k);
    else hipLaunchKernelGGL(k_inorm_silu3, grid, dim3(256), size_t(2) * C * sizeof(float), st, a);
    S3D_HIP(hipGetLastError());
    return 0;
}
int launch_inorm_silu3(float* const x[3], double* const part[3], const float* const gamma[3], const float* const beta[3], float* const y[3],
                       const size_t hw[3], int C, float eps, float* mr, hipStream_t st) {
    return launch_inorm_keep3(x, part, gamma, beta, nullptr, y, hw, C, eps, mr, st);
}

// ------------------------------------------------------------------ fused gather + MLP
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef const f32x4 __attribute__((address_space(1)))* gf4p;
__device__ __forceinline__ gf4p g4(const float* p) { return (gf4p)(uintptr_t)p; }

struct MlpW {                 // device pointers of one DecoderMLPSkipConcat, padded to multiples of 32
    const float* w[6]; const float* b[6];
};

constexpr int kSlabLd = 36;   // padded slab row (floats)

// One layer on the matrix cores: hout[m] (MT tiles of 32 rows) = W[MT*32][K] x [in0 | in1] + bias, optional ReLU.
// in0 has KT0 tiles of 32 rows, in1 KT1.  All four waves run it in lockstep (they share the LDS weight slabs).
// BIAS = false starts the accumulators at zero and never reads `bias` (the transposed layers of k_decode_grad).  GRAD only tells
// k_decode_grad's instances from k_decode's: sharing them reordered k_decode's instructions, and k_decode is to compile as it did.
template <int KT0, int KT1, int MT, bool BIAS = true, bool GRAD = false>
__device__ __forceinline__ void mlp_layer(const float* __restrict__ Wg, const float* __restrict__ bias,
                                          const f32x16* in0, const f32x16* in1, f32x16* hout, float* lds, bool relu) {
    constexpr int KT = KT0 + KT1, K = KT * 32, M = MT * 32;
    constexpr int ITEMS = M * 8, NI = (ITEMS + 255) / 256;
    const int tid = threadIdx.x, lane = tid & 63, j = lane & 31, half = lane >> 5;
    // accumulators start at the bias of their rows
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int r = 0; r < 16; ++r) hout[m][r] = BIAS ? bias[m * 32 + (r & 3) + 8 * (r >> 2) + 4 * half] : 0.f;
    // slab staging descriptors: item -> (row, float4 q)
    gf4p src[NI]; int dst[NI];
#pragma unroll
    for (int it = 0; it < NI; ++it) {
        const int idx = min(it * 256 + tid, ITEMS - 1);
        const int row = idx >> 3, q = idx & 7;
        src[it] = g4(Wg + size_t(row) * K + q * 4);
        dst[it] = row * kSlabLd + q * 4;
    }
    f32x4 rg[NI];
    __syncthreads();                                   // previous layer's last slab reads are done
#pragma unroll
    for (int it = 0; it < NI; ++it) rg[it] = src[it][0];
#pragma unroll
    for (int it = 0; it < NI; ++it) *reinterpret_cast<f32x4*>(lds + dst[it]) = rg[it];
    __syncthreads();
#pragma unroll
    for (int t = 0; t < KT; ++t) {
        constexpr int kLastT = KT - 1;
        const int nt = t == kLastT ? t : t + 1;        // last slab re-fetches itself (harmless)
#pragma unroll
        for (int it = 0; it < NI; ++it) rg[it] = src[it][nt * 8];
        __builtin_amdgcn_sched_barrier(0);
        const float* slab = lds + (t & 1) * (M * kSlabLd);
        const f32x16& hin = t < KT0 ? in0[t < KT0 ? t : 0] : in1[t >= KT0 ? t - KT0 : 0];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            f32x4 a4[MT];
#pragma unroll
            for (int m = 0; m < MT; ++m) a4[m] = *reinterpret_cast<const f32x4*>(slab + (m * 32 + j) * kSlabLd + q * 8 + half * 4);
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int m = 0; m < MT; ++m)
                    hout[m] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[m][e], hin[q * 4 + e], hout[m], 0, 0, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
        float* nxt = lds + ((t + 1) & 1) * (M * kSlabLd);
#pragma unroll
        for (int it = 0; it < NI; ++it) *reinterpret_cast<f32x4*>(nxt + dst[it]) = rg[it];
        __syncthreads();
    }
    if (relu) {
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int r = 0; r < 16; ++r) hout[m][r] = fmaxf(hout[m][r], 0.f);
    }
}

// bilinear, padding_mode='border', align_corners=False sample of plane `fm` [h][w][UPT*32] at (u -> rows, v -> cols),
// accumulated into the lane's operand registers: x[t][4q+e] is channel 32t + 8q + 4*half + e.
template <int UPT>
__device__ __forceinline__ void gather_plane(const float* __restrict__ fm, int h, int w, float u, float v, int half,
                                             f32x16* x) {
    constexpr int C = UPT * 32;
    float fy = ((u + 1.f) * float(h) - 1.f) * 0.5f, fx = ((v + 1.f) * float(w) - 1.f) * 0.5f;
    fy = fminf(fmaxf(fy, 0.f), float(h - 1)); fx = fminf(fmaxf(fx, 0.f), float(w - 1));
    const int y0 = int(floorf(fy)), x0 = int(floorf(fx));
    const float ty = fy - float(y0), tx = fx - float(x0);
    const float w00 = (1.f - ty) * (1.f - tx), w01 = (1.f - ty) * tx, w10 = ty * (1.f - tx), w11 = ty * tx;
    const int y1 = min(y0 + 1, h - 1), x1 = min(x0 + 1, w - 1);
    const float* p00 = fm + (size_t(y0) * w + x0) * C + half * 4;
    const float* p01 = fm + (size_t(y0) * w + x1) * C + half * 4;
    const float* p10 = fm + (size_t(y1) * w + x0) * C + half * 4;
    const float* p11 = fm + (size_t(y1) * w + x1) * C + half * 4;
#pragma unroll
    for (int t = 0; t < UPT; ++t)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int c = t * 32 + q * 8;
            const f32x4 a = g4(p00 + c)[0], b = g4(p01 + c)[0], cc = g4(p10 + c)[0], d = g4(p11 + c)[0];
#pragma unroll
            for (int e = 0; e < 4; ++e) x[t][q * 4 + e] += w00 * a[e] + w01 * b[e] + w10 * cc[e] + w11 * d[e];
        }
}

// Feature groups that each carry a list of heads: a group's three planes are gathered ONCE into operand registers and every head
// of the group (its own DecoderMLPSkipConcat) runs on them, one after the other, so two heads' hidden tiles are never live
// together and nothing goes to memory between layers or heads.
//   skip net with texture  {geo: [sdf]}, {tex: [tex_channels 1..8, sigmoid]}
//   geometry only          {geo: [sdf]}
//   AutoEncoderGroupPBR    {geo: [sdf]}, {tex: [rgb 3, mr 2, normal 3]}      (no sigmoid, networks.py:311-315)
constexpr int kMaxHeads = 4;
struct DecodeArgs {
    const float* pts;         // [N][3] or null -> cell-centred grid points generated on the fly
    long long N;
    float amin[3];
    int gdim[3]; float gsize[3];
    const float* feat[2][3];  // [group][plane] NHWC [h][w][UP]
    int ph[3], pw[3];
    int ngroups;
    int hbeg[3];              // heads [hbeg[g], hbeg[g+1]) belong to group g
    MlpW mlp[kMaxHeads];
    int col0[kMaxHeads], ncol[kMaxHeads], sigm[kMaxHeads];   // output columns [col0, col0+ncol) (ncol <= 8), sigmoid flag
    int clamp_color;          // clamp columns >= 1 to [0,1] (never the sdf)
    float* out;               // [N][out_stride]
    int out_stride;
};

template <int UPT, int HIDT>
__global__ __launch_bounds__(256, 1) void k_decode(DecodeArgs a) {
    __shared__ __attribute__((aligned(16))) float lds[2 * HIDT * 32 * kSlabLd];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, j = lane & 31, half = lane >> 5;
    const long long pt = (long long)blockIdx.x * 128 + wave * 32 + j;
    const bool live = pt < a.N;
    float p[3] = {0.f, 0.f, 0.f};
    if (live) {
        if (a.pts) { p[0] = a.pts[pt * 3]; p[1] = a.pts[pt * 3 + 1]; p[2] = a.pts[pt * 3 + 2]; }
        else {        // sample_grid_points_aabb (src/encoding/utils3d.py:13-25): cell centres, 'ij' order
            // linspace(0.5, r-0.5, r) / r * size + min, one rounding per torch op (no fma contraction)
            const long long iz = pt % a.gdim[2], iy = (pt / a.gdim[2]) % a.gdim[1], ix = pt / ((long long)a.gdim[2] * a.gdim[1]);
            p[0] = __fadd_rn(__fmul_rn(__fdiv_rn(0.5f + float(ix), float(a.gdim[0])), a.gsize[0]), a.amin[0]);
            p[1] = __fadd_rn(__fmul_rn(__fdiv_rn(0.5f + float(iy), float(a.gdim[1])), a.gsize[1]), a.amin[1]);
            p[2] = __fadd_rn(__fmul_rn(__fdiv_rn(0.5f + float(iz), float(a.gdim[2])), a.gsize[2]), a.amin[2]);
        }
    }
    float qn[3];
#pragma unroll
    for (int k = 0; k < 3; ++k)                                                    // x = 2 * (x - min) / (max - min) - 1  (:196)
        qn[k] = __fsub_rn(__fdiv_rn(2.f * __fsub_rn(p[k], a.amin[k]), a.gsize[k]), 1.f);
    const float uu[3] = {qn[0], qn[0], qn[1]}, vv[3] = {qn[1], qn[2], qn[2]};      // coords_list [[0,1],[0,2],[1,2]] (:201)
    // rows are out_stride floats (36 B for the PBR net): no 16-byte alignment to rely on, so the lane writes its columns one by one
    float* orow = a.out + (live ? pt : 0) * a.out_stride;

#pragma unroll
    for (int g = 0; g < 2; ++g) {
        if (g < a.ngroups) {
            f32x16 x[UPT];
#pragma unroll
            for (int t = 0; t < UPT; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) x[t][r] = 0.f;
#pragma unroll
            for (int pl = 0; pl < 3; ++pl) gather_plane<UPT>(a.feat[g][pl], a.ph[pl], a.pw[pl], uu[pl], vv[pl], half, x);
            for (int hd = a.hbeg[g]; hd < a.hbeg[g + 1]; ++hd) {                 // block-uniform trip count (barriers inside)
                const MlpW& M = a.mlp[hd];
                f32x16 hA[HIDT], hB[HIDT], ho[1];
                mlp_layer<UPT, 0, HIDT>(M.w[0], M.b[0], x, x, hA, lds, true);
                mlp_layer<HIDT, 0, HIDT>(M.w[1], M.b[1], hA, hA, hB, lds, true);
                mlp_layer<HIDT, 0, HIDT>(M.w[2], M.b[2], hB, hB, hA, lds, true);
                mlp_layer<UPT, HIDT, HIDT>(M.w[3], M.b[3], x, hA, hB, lds, true);
                mlp_layer<HIDT, 0, HIDT>(M.w[4], M.b[4], hB, hB, hA, lds, true);
                mlp_layer<HIDT, 0, 1>(M.w[5], M.b[5], hA, hA, ho, lds, false);
                // rows 0..3 of the output tile are registers 0..3 of lane half 0, rows 4..7 those of half 1
                const int col0 = a.col0[hd], ncol = a.ncol[hd], sg = a.sigm[hd];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int row = e + 4 * half;
                    if (live && row < ncol) {
                        float c = ho[0][e];
                        if (sg) c = 1.f / (1.f + expf(-c));
                        if (a.clamp_color && col0 + row >= 1) c = fminf(fmaxf(c, 0.f), 1.f);
                        orow[col0 + row] = c;
                    }
                }
            }
        }
    }
}

// ------------------------------------------------------------------ sdf and its gradient with respect to the point
// k_decode_grad: the geometry group's chain of k_decode with each hidden layer's ReLU pattern kept as bit words, then the chain in
// reverse mode on transposed weight packs: the accumulator of G_prev = W^T G is again the next B operand, so mlp_layer runs it
// with zero-started accumulators and no ReLU.  dL/dx (UPT tiles) is dotted with the planes' bilinear derivative.
// The sdf it reports is NOT its own forward's: gather_plane's sums are left to the compiler's contraction, which picks other
// fused products in this kernel than in k_decode (1..4 units in the last place of the sdf, measured), so k_decode itself, run
// on the geometry head alone, writes sdf[N] first and this kernel reads it.  That is what makes the sdf bit-identical to
// decode_points' column 0.  A Newton step (step != 0) moves the point with that sdf and this gradient.
struct GradArgs {
    const float* pts;                               // [N][3] the points to evaluate (pts0 or pts_out of the previous step)
    const float* pts0;                              // [N][3] the start points (the total move is clamped around them)
    long long N;
    float amin[3], gsize[3];
    const float* feat[3]; int ph[3], pw[3];
    const float* w[6]; const float* b[6];           // the geometry head's forward packs
    const float* wt4; const float* wt3x; const float* wt3h; const float* wt2; const float* wt1; const float* wt0;   // transposed
    int step; float max_step, max_move;
    const float* sdf;                               // [N] k_decode's sdf at pts
    float* pts_out; float* grad;                    // pts_out: written when step != 0 (may alias pts), or a copy when non-null
};

// bit (m & 1) * 16 + r of word m >> 1: unit r of tile m is active
template <int HIDT>
__device__ __forceinline__ void relu_pattern(const f32x16* h, unsigned* mk) {
#pragma unroll
    for (int w = 0; w < (HIDT + 1) / 2; ++w) mk[w] = 0u;
#pragma unroll
    for (int m = 0; m < HIDT; ++m)
#pragma unroll
        for (int r = 0; r < 16; ++r) mk[m >> 1] |= (h[m][r] > 0.f ? 1u : 0u) << ((m & 1) * 16 + r);
    // the words are opaque from here on: seen through, relu_mask would select on the compares themselves, one lane mask in a
    // scalar register pair per unit and layer
#pragma unroll
    for (int w = 0; w < (HIDT + 1) / 2; ++w) asm volatile("" : "+v"(mk[w]));
}
template <int HIDT>
__device__ __forceinline__ void relu_mask(f32x16* g, const unsigned* mk) {
#pragma unroll
    for (int m = 0; m < HIDT; ++m)
#pragma unroll
        for (int r = 0; r < 16; ++r) g[m][r] = ((mk[m >> 1] >> ((m & 1) * 16 + r)) & 1u) ? g[m][r] : 0.f;
}

// d(sum over channels of dx * sample)/d(fy, fx) of one plane at gather_plane's cell, over the channels this lane half holds.
// F.grid_sample's backward for padding_mode='border': the factor of a clamped coordinate is 0 (on = false), the cell at an
// integer position is the one floor selects.  One deviation, on a set of measure zero: exactly ON the last texel centre (fy == h - 1, not
// clamped) floor selects a cell whose second row is clamped onto the first, so the factor is 0, where autograd keeps the in-bounds
// corners' term -(c00 (1 - tx) + c01 tx).
template <int UPT>
__device__ __forceinline__ void plane_grad(const float* __restrict__ fm, int h, int w, float u, float v, int half,
                                           const f32x16* dx, float& dfy, float& dfx, bool& on_y, bool& on_x) {
    constexpr int C = UPT * 32;
    float fy = __fmul_rn(__fmaf_rn(__fadd_rn(u, 1.f), float(h), -1.f), 0.5f), fx = __fmul_rn(__fmaf_rn(__fadd_rn(v, 1.f), float(w), -1.f), 0.5f);
    on_y = !(fy < 0.f) && !(fy > float(h - 1)); on_x = !(fx < 0.f) && !(fx > float(w - 1));
    fy = fminf(fmaxf(fy, 0.f), float(h - 1)); fx = fminf(fmaxf(fx, 0.f), float(w - 1));
    const int y0 = int(floorf(fy)), x0 = int(floorf(fx));
    const float ty = fy - float(y0), tx = fx - float(x0);
    const int y1 = min(y0 + 1, h - 1), x1 = min(x0 + 1, w - 1);
    const float* p00 = fm + (size_t(y0) * w + x0) * C + half * 4;
    const float* p01 = fm + (size_t(y0) * w + x1) * C + half * 4;
    const float* p10 = fm + (size_t(y1) * w + x0) * C + half * 4;
    const float* p11 = fm + (size_t(y1) * w + x1) * C + half * 4;
    float sy = 0.f, sx = 0.f;
#pragma unroll
    for (int t = 0; t < UPT; ++t)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int c = t * 32 + q * 8;
            const f32x4 a = g4(p00 + c)[0], b = g4(p01 + c)[0], cc = g4(p10 + c)[0], d = g4(p11 + c)[0];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float g = dx[t][q * 4 + e];
                sy += g * ((cc[e] - a[e]) * (1.f - tx) + (d[e] - b[e]) * tx);
                sx += g * ((b[e] - a[e]) * (1.f - ty) + (d[e] - cc[e]) * ty);
            }
        }
    dfy = sy + __shfl_xor(sy, 32);                  // lanes j and j + 32 hold the two halves of a point's channels
    dfx = sx + __shfl_xor(sx, 32);
}

template <int UPT, int HIDT>
__global__ __launch_bounds__(256, 1) void k_decode_grad(GradArgs a) {
    __shared__ __attribute__((aligned(16))) float lds[2 * HIDT * 32 * kSlabLd];
    constexpr int MW = (HIDT + 1) / 2;
    static_assert(UPT <= HIDT, "the slabs of the dL/dx layers (UPT * 32 rows) must fit the hidden layers' LDS");
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, j = lane & 31, half = lane >> 5;
    const long long pt = (long long)blockIdx.x * 128 + wave * 32 + j;
    const bool live = pt < a.N;
    float p[3] = {0.f, 0.f, 0.f};
    if (live) { p[0] = a.pts[pt * 3]; p[1] = a.pts[pt * 3 + 1]; p[2] = a.pts[pt * 3 + 2]; }
    float qn[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) qn[k] = __fsub_rn(__fdiv_rn(2.f * __fsub_rn(p[k], a.amin[k]), a.gsize[k]), 1.f);
    const float uu[3] = {qn[0], qn[0], qn[1]}, vv[3] = {qn[1], qn[2], qn[2]};
    unsigned mk[5][MW];
    f32x16 hA[HIDT], hB[HIDT], dx[UPT];
    {   // forward, for the ReLU patterns
        f32x16 x[UPT];
#pragma unroll
        for (int t = 0; t < UPT; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) x[t][r] = 0.f;
#pragma unroll
        for (int pl = 0; pl < 3; ++pl) gather_plane<UPT>(a.feat[pl], a.ph[pl], a.pw[pl], uu[pl], vv[pl], half, x);
        mlp_layer<UPT, 0, HIDT, true, true>(a.w[0], a.b[0], x, x, hA, lds, true);      relu_pattern<HIDT>(hA, mk[0]);
        mlp_layer<HIDT, 0, HIDT, true, true>(a.w[1], a.b[1], hA, hA, hB, lds, true);   relu_pattern<HIDT>(hB, mk[1]);
        mlp_layer<HIDT, 0, HIDT, true, true>(a.w[2], a.b[2], hB, hB, hA, lds, true);   relu_pattern<HIDT>(hA, mk[2]);
        mlp_layer<UPT, HIDT, HIDT, true, true>(a.w[3], a.b[3], x, hA, hB, lds, true);  relu_pattern<HIDT>(hB, mk[3]);
        mlp_layer<HIDT, 0, HIDT, true, true>(a.w[4], a.b[4], hB, hB, hA, lds, true);   relu_pattern<HIDT>(hA, mk[4]);
    }
    // backward: seed = the sdf row of the last layer, then the hidden layers transposed
#pragma unroll
    for (int m = 0; m < HIDT; ++m)
#pragma unroll
        for (int r = 0; r < 16; ++r) hA[m][r] = a.w[5][m * 32 + (r & 3) + 8 * (r >> 2) + 4 * half];
    relu_mask<HIDT>(hA, mk[4]);
    mlp_layer<HIDT, 0, HIDT, false, true>(a.wt4, nullptr, hA, hA, hB, lds, false);       relu_mask<HIDT>(hB, mk[3]);
    mlp_layer<HIDT, 0, UPT, false, true>(a.wt3x, nullptr, hB, hB, dx, lds, false);       // layer 3 takes [x | h]: dL/dx ...
    mlp_layer<HIDT, 0, HIDT, false, true>(a.wt3h, nullptr, hB, hB, hA, lds, false);      relu_mask<HIDT>(hA, mk[2]);   // ... and dL/dh
    mlp_layer<HIDT, 0, HIDT, false, true>(a.wt2, nullptr, hA, hA, hB, lds, false);       relu_mask<HIDT>(hB, mk[1]);
    mlp_layer<HIDT, 0, HIDT, false, true>(a.wt1, nullptr, hB, hB, hA, lds, false);       relu_mask<HIDT>(hA, mk[0]);
    {
        f32x16 dx0[UPT];
        mlp_layer<HIDT, 0, UPT, false, true>(a.wt0, nullptr, hA, hA, dx0, lds, false);
#pragma unroll
        for (int t = 0; t < UPT; ++t) dx[t] += dx0[t];
    }
    // planes: coords_list [[0,1],[0,2],[1,2]]; d fy / d u = h / 2, d u / d p_k = 2 / gsize[k]
    float gn[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int pl = 0; pl < 3; ++pl) {
        const int au = pl == 2 ? 1 : 0, av = pl == 0 ? 1 : 2;
        float dfy, dfx; bool on_y, on_x;
        plane_grad<UPT>(a.feat[pl], a.ph[pl], a.pw[pl], uu[pl], vv[pl], half, dx, dfy, dfx, on_y, on_x);
        gn[au] += on_y ? dfy * (0.5f * float(a.ph[pl])) : 0.f;
        gn[av] += on_x ? dfx * (0.5f * float(a.pw[pl])) : 0.f;
    }
    if (!live || half) return;
    float gr[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) { gr[k] = gn[k] * (2.f / a.gsize[k]); a.grad[pt * 3 + k] = gr[k]; }
    if (a.step) {
        // Newton step onto the level set, every operation rounded once (a float32 restatement reproduces it)
        const float sdf = a.sdf[pt];
        const float g2 = __fadd_rn(__fadd_rn(__fmul_rn(gr[0], gr[0]), __fmul_rn(gr[1], gr[1])), __fmul_rn(gr[2], gr[2]));
        if (g2 >= 1e-20f) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const float p0 = a.pts0[pt * 3 + k];
                float s = __fdiv_rn(__fmul_rn(sdf, gr[k]), g2);
                s = fminf(fmaxf(s, -a.max_step), a.max_step);
                float dm = __fsub_rn(__fsub_rn(p[k], s), p0);
                dm = fminf(fmaxf(dm, -a.max_move), a.max_move);
                p[k] = __fadd_rn(p0, dm);
            }
        }
    }
    if (a.pts_out) {
#pragma unroll
        for (int k = 0; k < 3; ++k) a.pts_out[pt * 3 + k] = p[k];
    }
}

}  // namespace s3d

using namespace s3d;

struct s3d_decoder {
    s3d_decoder_cfg cfg;
    int variant = 0;          // 0 skip net with texture, 1 geometry only, 2 AutoEncoderGroupPBR (include/sin3dm_hip.h)
    AeNetDesc desc;           // the blocks and heads (s3d_aenet.h); real widths, the padding below is this handle's business
    std::vector<ParamSpec> specs;
    std::map<std::string, std::vector<float>> host;
    bool packed = false;
    int up_p = 0, hid_p = 0;
    DevBuf wbuf;
    // packed offsets of desc.blocks[i] and desc.heads[i]
    struct Net { ConvW cin, cout_, sc; size_t gamma[3], beta[3]; } net[3];
    struct Head { size_t mw[6], mb[6]; };
    std::vector<Head> heads;
    // prepared features
    DevBuf feat;
    float* featp[2][3] = {{nullptr, nullptr, nullptr}, {nullptr, nullptr, nullptr}};
    float* feat0p[3] = {nullptr, nullptr, nullptr};      // PBR: the texture planes after block 0 (kept for plane_features)
    int ph[3] = {0, 0, 0}, pw[3] = {0, 0, 0};
    bool prepared = false;
    Arena arena;
    // transposed packs of the geometry head (s3d_decoder_sdf_grad), built on a handle's first gradient call
    DevBuf gbuf;
    bool gpacked = false;
    size_t gwt[6] = {0, 0, 0, 0, 0, 0};                  // wt4, wt3x, wt3h, wt2, wt1, wt0
    const float* dev(size_t off) const { return static_cast<const float*>(wbuf.p) + off; }
};

namespace s3d {

// dense [out][in] -> zero-padded [outp][inp] with column segments (in = seg0 | seg1 -> seg0p | seg1p)
static size_t pack_linear(std::vector<float>& st, const std::vector<float>& W, int out, int seg0, int seg1, int outp,
                          int seg0p, int seg1p) {
    const int in = seg0 + seg1, inp = seg0p + seg1p;
    size_t off = push(st, nullptr, size_t(outp) * inp);
    float* d = st.data() + off;
    std::fill(d, d + size_t(outp) * inp, 0.f);
    for (int o = 0; o < out; ++o) {
        for (int i = 0; i < seg0; ++i) d[size_t(o) * inp + i] = W[size_t(o) * in + i];
        for (int i = 0; i < seg1; ++i) d[size_t(o) * inp + seg0p + i] = W[size_t(o) * in + seg0 + i];
    }
    return off;
}
static size_t pack_vec(std::vector<float>& st, const float* v, int n, int np) {
    size_t off = push(st, nullptr, np);
    std::fill(st.begin() + off, st.begin() + off + np, 0.f);
    std::copy(v, v + n, st.begin() + off);
    return off;
}

static int dec_pack(s3d_decoder* d) {
    for (const auto& sp : d->specs)
        S3D_CHECK(d->host.count(sp.name), S3D_ERR_MISSING, "decoder parameter '%s' was never set", sp.name.c_str());
    const int up = d->desc.up, hid = d->desc.hid, upp = d->up_p, hidp = d->hid_p;
    std::vector<float> st;
    // pad every conv to (cin cip, cout upp): [tap][coutp][cinp]
    auto pack_conv = [&](const std::string& cv, int ci, int cip, int kk, ConvW& cw) {
        const std::vector<float>&W = d->host.at(cv + ".weight"), &b = d->host.at(cv + ".bias");
        cw.cin = cip; cw.cout = upp; cw.k = kk; cw.rollout = false;
        const int taps = kk * kk;
        for (int p = 0; p < 3; ++p) {
            cw.bias[p] = pack_vec(st, b.data() + size_t(p) * up, up, upp);
            cw.dense[p] = push(st, nullptr, size_t(taps) * upp * cip);
            float* dd = st.data() + cw.dense[p];
            std::fill(dd, dd + size_t(taps) * upp * cip, 0.f);
            for (int t = 0; t < taps; ++t)
                for (int co = 0; co < up; ++co)
                    for (int ch = 0; ch < ci; ++ch)
                        dd[(size_t(t) * upp + co) * cip + ch] = W[((size_t(p) * up + co) * ci + ch) * taps + t];
        }
    };
    for (size_t i = 0; i < d->desc.blocks.size(); ++i) {
        const AeBlock& B = d->desc.blocks[i];
        s3d_decoder::Net& N = d->net[i];
        const int cip = rup32(B.cin);
        pack_conv(B.in_conv(), B.cin, cip, B.ks, N.cin);
        pack_conv(B.prefix + ".out_layers.1", up, upp, B.ks, N.cout_);
        if (B.shortcut) pack_conv(B.prefix + ".shortcut", B.cin, cip, 1, N.sc);
        for (int p = 0; p < 3; ++p) {
            N.gamma[p] = pack_vec(st, d->host.at(B.prefix + ".norm_" + kPlane[p] + ".weight").data(), up, upp);
            N.beta[p] = pack_vec(st, d->host.at(B.prefix + ".norm_" + kPlane[p] + ".bias").data(), up, upp);
        }
    }
    d->heads.resize(d->desc.heads.size());
    for (size_t i = 0; i < d->heads.size(); ++i) {
        const std::string ml = d->desc.heads[i].name;
        int I[6], O[6];
        mlp_dims(up, hid, d->desc.heads[i].nout, I, O);
        for (int l = 0; l < 6; ++l) {                    // layers 0 and 3 start with the features, layer 3 goes on with the hidden units
            const int s0 = l == 3 ? up : I[l], s0p = l == 0 || l == 3 ? upp : hidp, outp = l == 5 ? 32 : hidp;
            d->heads[i].mw[l] = pack_linear(st, d->host.at(ml + kMlpLayer[l] + ".weight"), O[l], s0, I[l] - s0, outp, s0p, l == 3 ? hidp : 0);
            d->heads[i].mb[l] = pack_vec(st, d->host.at(ml + kMlpLayer[l] + ".bias").data(), O[l], outp);
        }
    }
    S3D_TRY(upload(d->wbuf, st.data(), st.size() * sizeof(float)));
    d->packed = true;
    return 0;
}
// The compiled (UPT, HIDT) = (up_p / 32, hid_p / 32) pairs of k_decode and k_decode_grad: f(Tiles<UPT, HIDT>()) for the handle's pair
template <int U, int H> struct Tiles { static constexpr int upt = U, hidt = H; };
template <class F>
static int with_tiles(const s3d_decoder* d, F&& f) {
    const int upt = d->up_p / 32, hidt = d->hid_p / 32;
    if (upt == 2 && hidt == 8) return f(Tiles<2, 8>());
    if (upt == 1 && hidt == 1) return f(Tiles<1, 1>());
    if (upt == 1 && hidt == 8) return f(Tiles<1, 8>());
    if (upt == 1 && hidt == 2) return f(Tiles<1, 2>());
    if (upt == 3 && hidt == 4) return f(Tiles<3, 4>());
    set_error("decoder: feat_channel_up=%d / mlp_hidden_channels=%d has no compiled kernel (supported after padding to 32: "
              "up<=64 with hidden 256, up<=32 with hidden 32 or 64, up 96 with hidden 128)", d->cfg.feat_channel_up,
              d->cfg.mlp_hidden_channels);
    return S3D_ERR_UNSUPPORTED;
}
template <int UPT, int HIDT>
static int launch_decode(const DecodeArgs& a, hipStream_t st) {
    const long long blocks = (a.N + 127) / 128;
    if (!blocks) return 0;
    hipLaunchKernelGGL((k_decode<UPT, HIDT>), dim3((unsigned)blocks), dim3(256), 0, st, a);
    S3D_HIP(hipGetLastError());
    return 0;
}

static int run_decode(s3d_decoder* d, const float* pts, long long N, const float aabb[6], const int* gdim, int clamp,
                      float* out, hipStream_t st) {
    S3D_CHECK(d->prepared, S3D_ERR_INVALID, "decoder: call s3d_decoder_prepare_triplane first");
    DecodeArgs a; memset(&a, 0, sizeof a);
    a.pts = pts; a.N = N; a.clamp_color = clamp; a.out = out; a.out_stride = d->desc.out_channels();
    for (int k = 0; k < 3; ++k) {
        a.amin[k] = aabb[k]; a.gsize[k] = aabb[3 + k] - aabb[k];
        a.gdim[k] = gdim ? gdim[k] : 1; a.ph[k] = d->ph[k]; a.pw[k] = d->pw[k];
    }
    a.ngroups = d->desc.nsides;
    for (int g = 0; g < a.ngroups; ++g)
        for (int p = 0; p < 3; ++p) a.feat[g][p] = d->featp[g][p];
    S3D_CHECK(int(d->heads.size()) <= kMaxHeads, S3D_ERR_INVALID, "decoder: %d heads", int(d->heads.size()));
    int h = 0;
    for (int g = 0; g < 2; ++g) {                        // heads are stored group by group
        a.hbeg[g] = h;
        for (; h < int(d->heads.size()) && d->desc.heads[h].side == g; ++h) {
            const AeHead& H = d->desc.heads[h];
            for (int l = 0; l < 6; ++l) { a.mlp[h].w[l] = d->dev(d->heads[h].mw[l]); a.mlp[h].b[l] = d->dev(d->heads[h].mb[l]); }
            a.col0[h] = H.col0; a.ncol[h] = H.nout; a.sigm[h] = H.sigmoid;
        }
    }
    a.hbeg[2] = h;
    return with_tiles(d, [&](auto t) { return launch_decode<decltype(t)::upt, decltype(t)::hidt>(a, st); });
}

// columns [c0, c0+n) of dense W [out][in], transposed and zero-padded: [np][outp]
static size_t pack_transposed(std::vector<float>& st, const std::vector<float>& W, int out, int in, int c0, int n, int np, int outp) {
    std::vector<float> t(size_t(n) * out);
    for (int o = 0; o < out; ++o)
        for (int i = 0; i < n; ++i) t[size_t(i) * out + o] = W[size_t(o) * in + c0 + i];
    return pack_linear(st, t, n, out, 0, np, outp, 0);
}
static int dec_pack_grad(s3d_decoder* d) {
    const int up = d->desc.up, hid = d->desc.hid, upp = d->up_p, hidp = d->hid_p;
    const std::string ml = d->desc.heads[0].name;        // geo_decoder
    auto W = [&](const char* layer) -> const std::vector<float>& { return d->host.at(ml + layer + ".weight"); };
    std::vector<float> st;
    d->gwt[0] = pack_transposed(st, W(".second_layers.2"), hid, hid, 0, hid, hidp, hidp);
    d->gwt[1] = pack_transposed(st, W(".second_layers.0"), hid, up + hid, 0, up, upp, hidp);
    d->gwt[2] = pack_transposed(st, W(".second_layers.0"), hid, up + hid, up, hid, hidp, hidp);
    d->gwt[3] = pack_transposed(st, W(".first_layers.4"), hid, hid, 0, hid, hidp, hidp);
    d->gwt[4] = pack_transposed(st, W(".first_layers.2"), hid, hid, 0, hid, hidp, hidp);
    d->gwt[5] = pack_transposed(st, W(".first_layers.0"), hid, up, 0, up, upp, hidp);
    S3D_TRY(upload(d->gbuf, st.data(), st.size() * sizeof(float)));
    d->gpacked = true;
    return 0;
}
template <int UPT, int HIDT>
static int launch_decode_grad(const GradArgs& a, hipStream_t st) {
    hipLaunchKernelGGL((k_decode_grad<UPT, HIDT>), dim3((unsigned)((a.N + 127) / 128)), dim3(256), 0, st, a);
    S3D_HIP(hipGetLastError());
    return 0;
}

}  // namespace s3d

extern "C" {

int s3d_decoder_create_variant(const s3d_decoder_cfg* cfg, int32_t variant, s3d_decoder** out) {
    S3D_CHECK(cfg && out, S3D_ERR_INVALID, "decoder_create: null argument");
    S3D_CHECK(variant >= 0 && variant <= 2, S3D_ERR_INVALID, "decoder: variant %d (0 skip net with texture, 1 geometry only, 2 PBR)", int(variant));
    S3D_CHECK(cfg->mlp_hidden_layers == 4, S3D_ERR_UNSUPPORTED, "decoder: mlp_hidden_layers=%d (only the default 4 is built)", cfg->mlp_hidden_layers);
    S3D_CHECK(cfg->geo_feat_channels >= 1 && cfg->geo_feat_channels <= 32 && (variant == 1 || (cfg->tex_feat_channels >= 1 && cfg->tex_feat_channels <= 32)),
              S3D_ERR_UNSUPPORTED, "decoder: feature groups must have 1..32 channels");
    S3D_CHECK(variant != 0 || (cfg->tex_channels >= 1 && cfg->tex_channels <= 8), S3D_ERR_UNSUPPORTED, "decoder: tex_channels must be 1..8");
    S3D_CHECK(cfg->feat_channel_up >= 1 && cfg->mlp_hidden_channels >= 1, S3D_ERR_INVALID, "decoder: bad widths");
    std::unique_ptr<s3d_decoder> d(new s3d_decoder());
    d->cfg = *cfg;
    d->variant = variant;
    d->up_p = rup32(cfg->feat_channel_up);
    d->hid_p = rup32(cfg->mlp_hidden_channels);
    d->desc = aenet_describe(*cfg, variant);
    S3D_CHECK(d->desc.runnable(), S3D_ERR_UNSUPPORTED, "decoder: prepare_triplane is not written for this description of the net (s3d_aenet.h)");
    d->specs = aenet_params(d->desc, /*with_encoders=*/false);
    *out = d.release();
    return 0;
}
int s3d_decoder_create(const s3d_decoder_cfg* cfg, s3d_decoder** out) {
    S3D_CHECK(cfg && out, S3D_ERR_INVALID, "decoder_create: null argument");
    S3D_CHECK(cfg->tex_channels >= 1 && cfg->tex_channels <= 3, S3D_ERR_UNSUPPORTED, "decoder: tex_channels must be 1..3");
    return s3d_decoder_create_variant(cfg, 0, out);
}
int s3d_decoder_out_channels(const s3d_decoder* d) { return d ? d->desc.out_channels() : S3D_ERR_INVALID; }
void s3d_decoder_destroy(s3d_decoder* d) { delete d; }
int s3d_decoder_num_params(const s3d_decoder* d) { return d ? int(d->specs.size()) : S3D_ERR_INVALID; }
int s3d_decoder_param_info(const s3d_decoder* d, int i, const char** name, int64_t shape[4], int* ndim) {
    return registry_param_info(d ? &d->specs : nullptr, "decoder ", i, name, shape, ndim);
}
int s3d_decoder_set_param(s3d_decoder* d, const char* name, const float* data, const int64_t* shape, int ndim) {
    S3D_TRY(registry_set_param(d ? &d->specs : nullptr, d ? &d->host : nullptr, "decoder ", name, data, shape, ndim));
    d->packed = false;
    d->gpacked = false;
    return 0;
}

int s3d_decoder_prepare_triplane(s3d_decoder* d, const float* xy, const float* xz, const float* yz, int H, int W, int D,
                                 void* stream) {
    S3D_CHECK(d && xy && xz && yz && H >= 1 && W >= 1 && D >= 1, S3D_ERR_INVALID, "decoder prepare: bad argument");
    if (!d->packed) S3D_TRY(dec_pack(d));
    hipStream_t st = static_cast<hipStream_t>(stream);
    const Geo g = Geo::from_hwd(H, W, D);
    const float* in[3] = {xy, xz, yz};
    const int upp = d->up_p;
    const bool pbr = d->variant == 2;
    const int ngroups = d->desc.nsides;
    // persistent outputs: groups x 3 planes x [h][w][upp]  (+ the PBR texture planes after block 0)
    size_t tot = 0;
    for (int p = 0; p < 3; ++p) tot += size_t(g.h[p]) * g.w[p] * upp;
    S3D_HIP(hipStreamSynchronize(st));               // the feature buffer may still be read by an earlier decode
    S3D_TRY(d->feat.reserve((ngroups + (pbr ? 1 : 0)) * tot * sizeof(float)));
    {
        float* base = static_cast<float*>(d->feat.p);
        for (int n = 0; n < ngroups; ++n)
            for (int p = 0; p < 3; ++p) { d->featp[n][p] = base; base += size_t(g.h[p]) * g.w[p] * upp; }
        for (int p = 0; p < 3; ++p) { d->feat0p[p] = pbr ? base : nullptr; if (pbr) base += size_t(g.h[p]) * g.w[p] * upp; }
    }
    for (int p = 0; p < 3; ++p) { d->ph[p] = g.h[p]; d->pw[p] = g.w[p]; }
    // temporaries (two passes: measure, then run)
    for (int pass = 0; pass < 2; ++pass) {
        Arena& ar = d->arena;
        ar.measuring = pass == 0;
        if (pass == 0) ar.high = 0;
        else if (ar.high > ar.buf.cap) S3D_TRY(ar.buf.reserve(ar.high));
        ar.reset();
        for (int n = 0; n < ngroups; ++n) {
            auto& N = d->net[n];
            const int c0 = n == 0 ? 0 : d->cfg.geo_feat_channels;
            const bool two = pbr && n == 1;              // the PBR texture branch: two 3x3 blocks
            const ConvKind kind = two ? CONV_3x3 : CONV_5x5;
            Tri x, a, y, s; x.C = 32; a.C = y.C = s.C = upp; x.g = a.g = y.g = s.g = g;
            double* part[3];
            for (int p = 0; p < 3; ++p) {
                const size_t hw = size_t(g.h[p]) * g.w[p];
                x.p[p] = ar.alloc<float>(hw * 32); a.p[p] = ar.alloc<float>(hw * upp);
                y.p[p] = ar.alloc<float>(hw * upp); s.p[p] = ar.alloc<float>(hw * upp);
                part[p] = ar.alloc<double>(size_t(kInNormChunks) * upp * 2);
            }
            if (pass == 0) continue;
            for (int p = 0; p < 3; ++p) {
                const int hw = g.h[p] * g.w[p];
                hipLaunchKernelGGL(k_slice_pad, dim3((unsigned)((size_t(hw) * 32 + 255) / 256)), dim3(256), 0, st, in[p], x.p[p], hw, c0, d->desc.blocks[n].cin);
            }
            S3D_HIP(hipGetLastError());
            auto conv = [&](ConvKind kd, const ConvW& cw, const Tri& src, const Tri* res, float* const dst[3]) {
                ConvArgs ca; memset(&ca, 0, sizeof ca);
                ca.B = 1; ca.cin = cw.cin; ca.cout = cw.cout; ca.njobs = 3;
                for (int p = 0; p < 3; ++p) {
                    ConvJob& J = ca.job[p];
                    J.in = src.p[p]; J.wgt = d->dev(cw.dense[p]); J.bias = d->dev(cw.bias[p]);
                    J.res = res ? res->p[p] : nullptr; J.out = dst[p]; J.h = g.h[p]; J.w = g.w[p];
                }
                return launch_conv(kd, ca, st);
            };
            // norm_{p} (+ SiLU) of src with the block's per-plane gamma / beta; keep != null also stores the normalised maps
            auto inorm = [&](const s3d_decoder::Net& B, float* const src[3], float* const keep[3], float* const dst[3]) -> int {
                for (int p = 0; p < 3; ++p) {
                    const int hw = g.h[p] * g.w[p], cq = upp / 4, pl = std::max(1, 256 / cq);
                    hipLaunchKernelGGL(k_chan_partials, dim3(kInNormChunks), dim3(cq * pl), size_t(pl) * upp * 2 * sizeof(double), st, src[p], part[p], hw, upp);
                    const dim3 grid(std::min(1024, (hw * cq + 255) / 256));
                    if (keep)
                        hipLaunchKernelGGL(k_inorm_keep, grid, dim3(256), size_t(2) * upp * sizeof(float), st, src[p], part[p],
                                           d->dev(B.gamma[p]), d->dev(B.beta[p]), keep[p], dst[p], hw, upp, 1e-6f);
                    else
                        hipLaunchKernelGGL(k_inorm_silu, grid, dim3(256), size_t(2) * upp * sizeof(float), st, src[p], part[p],
                                           d->dev(B.gamma[p]), d->dev(B.beta[p]), dst[p], hw, upp, 1e-6f);
                }
                S3D_HIP(hipGetLastError());
                return 0;
            };
            S3D_TRY(conv(kind, N.cin, x, nullptr, a.p));                             // in_layers: conv (no norm/act on the input)
            S3D_TRY(inorm(N, a.p, nullptr, y.p));                                    // norm_{p} -> SiLU
            S3D_TRY(conv(CONV_1x1, N.sc, x, nullptr, s.p));                          // shortcut(x)
            S3D_TRY(conv(kind, N.cout_, y, &s, two ? d->feat0p : d->featp[n]));      // out_layers conv + shortcut
            if (two) {
                // tex_convs.1 (input_norm, input_act): xn = IN(f0); a = conv(SiLU(xn)); y = SiLU(IN(a)) with the SAME norm_p;
                // f1 = conv(y) + xn — the Identity shortcut acts on the block's `x`, which forward() rebuilt from the normalised maps
                auto& N1 = d->net[2];
                Tri f0; f0.C = upp; f0.g = g;
                for (int p = 0; p < 3; ++p) f0.p[p] = d->feat0p[p];
                S3D_TRY(inorm(N1, f0.p, s.p, y.p));                                  // s <- xn, y <- SiLU(xn)   (s is free again)
                S3D_TRY(conv(CONV_3x3, N1.cin, y, nullptr, a.p));
                S3D_TRY(inorm(N1, a.p, nullptr, y.p));
                S3D_TRY(conv(CONV_3x3, N1.cout_, y, &s, d->featp[1]));
            }
        }
    }
    d->prepared = true;
    return 0;
}

int s3d_decoder_plane_features(s3d_decoder* d, int group, int plane, float* out, void* stream) {
    S3D_CHECK(d && out && plane >= 0 && plane < 3, S3D_ERR_INVALID, "plane_features: bad argument");
    S3D_CHECK(d->prepared, S3D_ERR_INVALID, "decoder: call s3d_decoder_prepare_triplane first");
    const float* src = nullptr;
    if (group >= 0 && group < d->desc.nsides) src = d->featp[group][plane];
    else if (group == 2 && d->variant == 2) src = d->feat0p[plane];
    S3D_CHECK(src, S3D_ERR_INVALID, "plane_features: this decoder has no feature group %d", group);
    const long long hw = (long long)d->ph[plane] * d->pw[plane];
    const int up = d->cfg.feat_channel_up;
    hipLaunchKernelGGL(k_plane_to_nchw, dim3((unsigned)((hw * up + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), src, out, hw,
                       d->up_p, up);
    S3D_HIP(hipGetLastError());
    return 0;
}

int s3d_decoder_decode_points(s3d_decoder* d, const float* pts, int64_t N, const float aabb[6], int clamp_color, float* out,
                              void* stream) {
    S3D_CHECK(d && aabb && N >= 0 && (N == 0 || (pts && out)), S3D_ERR_INVALID, "decode_points: bad argument");
    if (N == 0) return 0;                                   // decoding no points is a no-op (empty tensors have null pointers)
    return run_decode(d, pts, N, aabb, nullptr, clamp_color, out, static_cast<hipStream_t>(stream));
}

int s3d_decoder_sdf_grad(s3d_decoder* d, const float* pts, int64_t N, const float aabb[6], int iters, float max_step, float max_move,
                         float* pts_out, float* sdf, float* grad, void* stream) {
    S3D_CHECK(d && aabb && N >= 0 && (N == 0 || (pts && sdf && grad)), S3D_ERR_INVALID, "sdf_grad: bad argument");
    S3D_CHECK(iters >= 0, S3D_ERR_INVALID, "sdf_grad: iters=%d", iters);
    S3D_CHECK(iters == 0 || N == 0 || pts_out, S3D_ERR_INVALID, "sdf_grad: iters=%d needs pts_out", iters);
    S3D_CHECK(iters == 0 || (max_step > 0.f && max_move > 0.f), S3D_ERR_INVALID, "sdf_grad: max_step=%g, max_move=%g must be positive", double(max_step), double(max_move));
    S3D_TRY(with_tiles(d, [](auto) { return 0; }));        // an uncompiled pair is refused whatever N is
    if (N == 0) return 0;
    S3D_CHECK(d->prepared, S3D_ERR_INVALID, "decoder: call s3d_decoder_prepare_triplane first");
    S3D_CHECK(d->packed, S3D_ERR_INVALID, "decoder: parameters changed since s3d_decoder_prepare_triplane; prepare again");
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (!d->gpacked) {
        S3D_HIP(hipStreamSynchronize(st));               // an earlier gradient call may still read the packs
        S3D_TRY(dec_pack_grad(d));
    }
    // the geometry head alone through k_decode: sdf[N] with the bits of decode_points' column 0
    DecodeArgs da; memset(&da, 0, sizeof da);
    da.N = N; da.out = sdf; da.out_stride = 1; da.ngroups = 1;
    GradArgs a; memset(&a, 0, sizeof a);
    a.pts0 = pts; a.N = N; a.max_step = max_step; a.max_move = max_move; a.sdf = sdf; a.grad = grad;
    for (int k = 0; k < 3; ++k) {
        da.amin[k] = a.amin[k] = aabb[k]; da.gsize[k] = a.gsize[k] = aabb[3 + k] - aabb[k];
        da.feat[0][k] = a.feat[k] = d->featp[0][k]; da.ph[k] = a.ph[k] = d->ph[k]; da.pw[k] = a.pw[k] = d->pw[k];
        da.gdim[k] = 1;
    }
    const auto& H = d->heads[0];
    for (int l = 0; l < 6; ++l) { da.mlp[0].w[l] = a.w[l] = d->dev(H.mw[l]); da.mlp[0].b[l] = a.b[l] = d->dev(H.mb[l]); }
    da.hbeg[0] = 0; da.hbeg[1] = da.hbeg[2] = 1; da.col0[0] = 0; da.ncol[0] = 1;
    const float* g = static_cast<const float*>(d->gbuf.p);
    a.wt4 = g + d->gwt[0]; a.wt3x = g + d->gwt[1]; a.wt3h = g + d->gwt[2]; a.wt2 = g + d->gwt[3]; a.wt1 = g + d->gwt[4]; a.wt0 = g + d->gwt[5];
    for (int it = 0; it <= iters; ++it) {                // iters + 1 evaluations: sdf and grad belong to the returned point
        da.pts = a.pts = it == 0 ? pts : pts_out;
        a.step = it < iters;
        a.pts_out = (a.step || iters == 0) ? pts_out : nullptr;
        S3D_TRY(with_tiles(d, [&](auto t) {
            S3D_TRY((launch_decode<decltype(t)::upt, decltype(t)::hidt>(da, st)));
            return launch_decode_grad<decltype(t)::upt, decltype(t)::hidt>(a, st);
        }));
    }
    return 0;
}

int s3d_decoder_grid_dims(const float aabb[6], int reso, int dims[3]) {
    S3D_CHECK(aabb && dims && reso >= 1, S3D_ERR_INVALID, "grid_dims: bad argument");
    // resolutions = (resolution * aabb_size / aabb_size.max()).long()  in fp32 (src/encoding/utils3d.py:17-19)
    float size[3], mx = 0.f;
    for (int k = 0; k < 3; ++k) { size[k] = aabb[3 + k] - aabb[k]; mx = std::max(mx, size[k]); }
    S3D_CHECK(mx > 0.f, S3D_ERR_INVALID, "grid_dims: empty aabb");
    for (int k = 0; k < 3; ++k) dims[k] = int(float(reso) * size[k] / mx);
    return 0;
}

int s3d_decoder_decode_grid(s3d_decoder* d, int reso, const float aabb[6], float* out, void* stream) {
    S3D_CHECK(d && aabb && out, S3D_ERR_INVALID, "decode_grid: bad argument");
    int dims[3];
    S3D_TRY(s3d_decoder_grid_dims(aabb, reso, dims));
    const long long N = (long long)dims[0] * dims[1] * dims[2];
    return run_decode(d, nullptr, N, aabb, dims, /*clamp=*/1, out, static_cast<hipStream_t>(stream));
}

}  // extern "C"
