// s3d_decoder_mlp.h — what the decoder's fused gather + MLP kernels share: the operand types, one MLP layer on the matrix cores
// and the bilinear plane gather (k_decode in s3d_decoder.hip, k_decode_heads in s3d_decoder_heads.hip).
#pragma once
#include "s3d_common.h"

namespace s3d {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef const f32x4 __attribute__((address_space(1)))* gf4p;
__device__ __forceinline__ gf4p g4(const float* p) { return (gf4p)(uintptr_t)p; }

// ------------------------------------------------------------------ fused gather + MLP
struct MlpW {                 // device pointers of one DecoderMLPSkipConcat, padded to multiples of 32
    const float* w[6]; const float* b[6];
};

constexpr int kSlabLd = 36;   // padded slab row (floats)

// One layer on the matrix cores: hout[m] (MT tiles of 32 rows) = W[MT*32][K] x [in0 | in1] + bias, optional ReLU.
// in0 has KT0 tiles of 32 rows, in1 KT1.  All four waves run it in lockstep (they share the LDS weight slabs).
template <int KT0, int KT1, int MT>
__device__ __forceinline__ void mlp_layer(const float* __restrict__ Wg, const float* __restrict__ bias,
                                          const f32x16* in0, const f32x16* in1, f32x16* hout, float* lds, bool relu) {
    constexpr int KT = KT0 + KT1, K = KT * 32, M = MT * 32;
    constexpr int ITEMS = M * 8, NI = (ITEMS + 255) / 256;
    const int tid = threadIdx.x, lane = tid & 63, j = lane & 31, half = lane >> 5;
    // accumulators start at the bias of their rows
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int r = 0; r < 16; ++r) hout[m][r] = bias[m * 32 + (r & 3) + 8 * (r >> 2) + 4 * half];
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

// ------------------------------------------------------------------ feature groups with lists of heads (decoder variants 1 and 2)
// The same machinery as k_decode, organised as feature groups that each carry a list of heads: a group's three planes are
// gathered ONCE into operand registers and every head of the group (its own DecoderMLPSkipConcat) runs on them, one after the
// other, so three heads' hidden tiles are never live together and nothing goes to memory between layers or heads.
//   geometry only          {geo: [sdf]}
//   AutoEncoderGroupPBR    {geo: [sdf]}, {tex: [rgb 3, mr 2, normal 3]}      (no sigmoid, networks.py:311-315)
//   skip net, 8 channels   {geo: [sdf]}, {tex: [8, sigmoid]}
constexpr int kMaxHeads = 4;
struct HeadsArgs {
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

// s3d_decoder_heads.hip.  launch_decode_heads returns S3D_ERR_UNSUPPORTED (no message) for a (up, hidden) tile pair without a kernel.
int launch_decode_heads(const HeadsArgs& a, int upt, int hidt, hipStream_t st);
// InstanceNorm2d of one NHWC plane [hw][C] from the chunk partials of k_chan_partials, both results kept: xn = IN(x), y = SiLU(xn)
int launch_inorm_keep(const float* x, const double* part, const float* gamma, const float* beta, float* xn, float* y, int hw, int C,
                      float eps, hipStream_t st);
// channels [0, up) of an NHWC [hw][C] plane -> NCHW [up][hw]
int launch_plane_to_nchw(const float* in, float* out, long long hw, int C, int up, hipStream_t st);

}  // namespace s3d
