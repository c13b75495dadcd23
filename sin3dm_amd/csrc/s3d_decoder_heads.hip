// s3d_decoder_heads.hip — the decoder's other networks (s3d_decoder_create_variant): geometry only, AutoEncoderGroupPBR
// (src/encoding/networks.py:227-316) and the skip net with up to 8 texture channels.  The point stage is one fused launch per
// decode call, k_decode's scheme with the chains organised as feature groups; the plane stage's two extra small kernels.
#include <algorithm>

#include "s3d_ae.h"
#include "s3d_decoder_mlp.h"

namespace s3d {

// The PBR texture branch's second block normalises its INPUT (blocks.py:238-239) and adds that normalised input back as the
// residual: InstanceNorm2d of one NHWC plane with both results kept, xn = IN(x) and y = SiLU(xn).
__global__ void k_inorm_keep(const float* __restrict__ x, const double* __restrict__ part, const float* __restrict__ gamma,
                             const float* __restrict__ beta, float* __restrict__ xn, float* __restrict__ y, int hw, int C, float eps) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    float* A = reinterpret_cast<float*>(smem_raw); float* Bc = A + C;
    for (int c = threadIdx.x; c < C; c += blockDim.x) {
        double S = 0, SS = 0;
        for (int k = 0; k < kInNormChunks; ++k) { S += part[(size_t(k) * C + c) * 2]; SS += part[(size_t(k) * C + c) * 2 + 1]; }
        const double m = S / hw;
        double var = SS / hw - m * m; if (var < 0) var = 0;
        const float scale = float(1.0 / sqrt(var + double(eps))) * gamma[c];
        A[c] = scale; Bc[c] = beta[c] - scale * float(m);
    }
    __syncthreads();
    const int cq = C / 4;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < (long long)hw * cq; i += (long long)gridDim.x * blockDim.x) {
        const int q = int(i % cq);
        const float4 v = reinterpret_cast<const float4*>(x)[i];
        const float4 a = reinterpret_cast<const float4*>(A)[q], b = reinterpret_cast<const float4*>(Bc)[q];
        float4 n, o;
        n.x = fmaf(v.x, a.x, b.x); n.y = fmaf(v.y, a.y, b.y); n.z = fmaf(v.z, a.z, b.z); n.w = fmaf(v.w, a.w, b.w);
        o.x = n.x / (1.f + expf(-n.x)); o.y = n.y / (1.f + expf(-n.y)); o.z = n.z / (1.f + expf(-n.z)); o.w = n.w / (1.f + expf(-n.w));
        reinterpret_cast<float4*>(xn)[i] = n;
        reinterpret_cast<float4*>(y)[i] = o;
    }
}
// channels [0, up) of an NHWC [h][w][C] plane -> NCHW [up][h][w]  (s3d_decoder_plane_features)
__global__ void k_plane_to_nchw(const float* __restrict__ in, float* __restrict__ out, long long hw, int C, int up) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= hw * up) return;
    const long long pix = i % hw;
    const int c = int(i / hw);
    out[i] = in[pix * C + c];
}

template <int UPT, int HIDT>
__global__ __launch_bounds__(256, 1) void k_decode_heads(HeadsArgs a) {
    __shared__ __attribute__((aligned(16))) float lds[2 * HIDT * 32 * kSlabLd];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, j = lane & 31, half = lane >> 5;
    const long long pt = (long long)blockIdx.x * 128 + wave * 32 + j;
    const bool live = pt < a.N;
    float p[3] = {0.f, 0.f, 0.f};
    if (live) {
        if (a.pts) { p[0] = a.pts[pt * 3]; p[1] = a.pts[pt * 3 + 1]; p[2] = a.pts[pt * 3 + 2]; }
        else {        // the grid of k_decode: cell centres, 'ij' order, one rounding per torch op
            const long long iz = pt % a.gdim[2], iy = (pt / a.gdim[2]) % a.gdim[1], ix = pt / ((long long)a.gdim[2] * a.gdim[1]);
            p[0] = __fadd_rn(__fmul_rn(__fdiv_rn(0.5f + float(ix), float(a.gdim[0])), a.gsize[0]), a.amin[0]);
            p[1] = __fadd_rn(__fmul_rn(__fdiv_rn(0.5f + float(iy), float(a.gdim[1])), a.gsize[1]), a.amin[1]);
            p[2] = __fadd_rn(__fmul_rn(__fdiv_rn(0.5f + float(iz), float(a.gdim[2])), a.gsize[2]), a.amin[2]);
        }
    }
    float qn[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) qn[k] = __fsub_rn(__fdiv_rn(2.f * __fsub_rn(p[k], a.amin[k]), a.gsize[k]), 1.f);
    const float uu[3] = {qn[0], qn[0], qn[1]}, vv[3] = {qn[1], qn[2], qn[2]};
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

template <int UPT, int HIDT>
static int launch_heads(const HeadsArgs& a, hipStream_t st) {
    const long long blocks = (a.N + 127) / 128;
    if (!blocks) return 0;
    hipLaunchKernelGGL((k_decode_heads<UPT, HIDT>), dim3((unsigned)blocks), dim3(256), 0, st, a);
    S3D_HIP(hipGetLastError());
    return 0;
}
int launch_decode_heads(const HeadsArgs& a, int upt, int hidt, hipStream_t st) {      // the tile pairs k_decode is built for
    if (upt == 2 && hidt == 8) return launch_heads<2, 8>(a, st);
    if (upt == 1 && hidt == 1) return launch_heads<1, 1>(a, st);
    if (upt == 1 && hidt == 8) return launch_heads<1, 8>(a, st);
    if (upt == 1 && hidt == 2) return launch_heads<1, 2>(a, st);
    if (upt == 3 && hidt == 4) return launch_heads<3, 4>(a, st);
    return S3D_ERR_UNSUPPORTED;
}

int launch_inorm_keep(const float* x, const double* part, const float* gamma, const float* beta, float* xn, float* y, int hw, int C,
                      float eps, hipStream_t st) {
    const int cq = C / 4;
    hipLaunchKernelGGL(k_inorm_keep, dim3(std::min(1024, (hw * cq + 255) / 256)), dim3(256), size_t(2) * C * sizeof(float), st, x, part,
                       gamma, beta, xn, y, hw, C, eps);
    S3D_HIP(hipGetLastError());
    return 0;
}

int launch_plane_to_nchw(const float* in, float* out, long long hw, int C, int up, hipStream_t st) {
    hipLaunchKernelGGL(k_plane_to_nchw, dim3((unsigned)((hw * up + 255) / 256)), dim3(256), 0, st, in, out, hw, C, up);
    S3D_HIP(hipGetLastError());
    return 0;
}

}  // namespace s3d
