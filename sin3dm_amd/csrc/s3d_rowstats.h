// s3d_rowstats.h — what the two evaluation feature handles (s3d_ssfid.hip, s3d_imgfeat.hip) share: the mean and ddof = 1
// covariance of rows of float32 activations in float64, the stage timing of a handle and the shape check of a
// parameter.
//
//   k_rows_gram<C, Load>  column sums and C x C Gram of the rows in float64 on v_mfma_f64_16x16x4_f64, `span` rows per block
//   k_rows_cov            block partials -> mu, sigma, parts added in index order
//
// No float atomics; every sum has a fixed order that depends on the row count and the span alone.
#pragma once
#include "s3d_common.h"

namespace s3d {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int kRsThreads = 256;
constexpr int kRsStage = 64;                          // rows per LDS stage of k_rows_gram
constexpr int kRsPad = 16;                            // floats between staged rows: the four rows of an MFMA step hit distinct banks

// ------------------------------------------------------------------ rows -> column sums, Gram
// Block (bx, by, img) takes rows [span bx, span bx + span) of image img in stages of 64 and the Gram columns [64 by, 64 by + 64):
// wave w owns the 16 columns jb = 4 by + w and all C / 16 row blocks, one v_mfma_f64_16x16x4_f64 accumulator each.  An MFMA step
// contracts four consecutive rows (lane l supplies row 4 s + l / 16, column l % 16 of its block); steps and stages run in row
// order.  Result register r of lane l is G[16 ib + l / 16 + 4 r][16 jb + l % 16].  Rows past the end are staged as zeros.
// C = 32 has two column blocks: waves 2 and 3 stage and wait at the barriers, and issue no MFMA and no store.
// Load: load.bind(t % (C / 4)) once per thread, then load(img, row, cq) gives the four activations of channel quad cq of a row.
// Where kRsThreads is a multiple of C / 4 (C = 32, 64) cq is the bound quad in every call: a Load may keep that quad's constants.
template <int C, class Load>
__global__ void __launch_bounds__(kRsThreads) k_rows_gram(Load load, long long R, int span, int nparts, double* __restrict__ gpart,
                                                          double* __restrict__ mpart) {
    constexpr int LD = C + kRsPad, NI = C / 16, Q = C / 4;
    __shared__ float a[kRsStage * LD];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const long long img = blockIdx.z;
    const long long r_begin = (long long)blockIdx.x * span;
    const long long r_end = min(R, r_begin + span);
    const int jb = blockIdx.y * 4 + wave;
    const bool own = C % 64 == 0 || jb < NI;
    load.bind(t % Q);
    f64x4 g[NI];
#pragma unroll
    for (int i = 0; i < NI; ++i) g[i] = f64x4{0.0, 0.0, 0.0, 0.0};
    double colsum = 0.0;
    for (long long r0 = r_begin; r0 < r_end; r0 += kRsStage) {
        for (int i = t; i < kRsStage * Q; i += kRsThreads) {
            const int row = i / Q, cq = i - row * Q;
            f32x4 x = {0.f, 0.f, 0.f, 0.f};
            if (r0 + row < r_end) x = load(img, r0 + row, cq);
            *reinterpret_cast<f32x4*>(a + row * LD + cq * 4) = x;
        }
        __syncthreads();
        if (own) {
#pragma unroll 2
            for (int s = 0; s < kRsStage / 4; ++s) {
                const float* ar = a + (s * 4 + (lane >> 4)) * LD + (lane & 15);
                const double bv = double(ar[jb * 16]);
#pragma unroll
                for (int ib = 0; ib < NI; ++ib) g[ib] = __builtin_amdgcn_mfma_f64_16x16x4f64(double(ar[ib * 16]), bv, g[ib], 0, 0, 0);
            }
        }
        if (blockIdx.y == 0 && t < C)
            for (int row = 0; row < kRsStage; ++row) colsum += double(a[row * LD + t]);
        __syncthreads();
    }
    double* gp = gpart + (img * nparts + blockIdx.x) * C * C;
    if (own) {
#pragma unroll
        for (int ib = 0; ib < NI; ++ib)
#pragma unroll
            for (int r = 0; r < 4; ++r) gp[(ib * 16 + (lane >> 4) + 4 * r) * C + jb * 16 + (lane & 15)] = g[ib][r];
    }
    if (blockIdx.y == 0 && t < C) mpart[(img * nparts + blockIdx.x) * C + t] = colsum;
}

// mu[i] = S_i / R; sigma[i][j] = (G_ij - S_i S_j / R) / (R - 1): np.cov(rowvar=False), ddof = 1.  Block (x, img) owns 16 entries;
// lane pl = t % 16 of an entry adds parts pl, pl + 16, ... in order, then a fixed xor tree over the 16 lanes.  (static: no
// template, and each translation unit that includes this header carries its own copy.)
static __global__ void __launch_bounds__(kRsThreads) k_rows_cov(const double* __restrict__ gpart, const double* __restrict__ mpart, int nparts,
                                                                int C, double R, double* __restrict__ mu, double* __restrict__ sigma) {
    const int e = blockIdx.x * 16 + (threadIdx.x >> 4), pl = threadIdx.x & 15;       // C * C is a multiple of 16
    const long long img = blockIdx.y;
    const int i = e / C, j = e % C;
    const double* gp = gpart + img * nparts * C * C;
    const double* mp = mpart + img * nparts * C;
    double g = 0.0, si = 0.0, sj = 0.0;
    for (int p = pl; p < nparts; p += 16) {
        g += gp[(long long)p * C * C + e];
        si += mp[(long long)p * C + i];
        sj += mp[(long long)p * C + j];
    }
#pragma unroll
    for (int off = 8; off >= 1; off >>= 1) {
        g += __shfl_xor(g, off);
        si += __shfl_xor(si, off);
        sj += __shfl_xor(sj, off);
    }
    if (pl == 0) {
        sigma[img * C * C + e] = (g - si * sj / R) / (R - 1.0);
        if (j == 0) mu[img * C + i] = si / R;
    }
}

// The block partials of n images of R rows: grow-only, so a caller that allocates before its first launch reserves them there
// and launch_rows_stats finds them large enough.
inline int reserve_rows_stats(int C, long long R, int n, int span, DevBuf& gpart, DevBuf& mpart) {
    const size_t nparts = size_t((R + span - 1) / span);
    S3D_TRY(gpart.reserve(size_t(n) * nparts * C * C * sizeof(double)));
    return mpart.reserve(size_t(n) * nparts * C * sizeof(double));
}

// mu [n][C] and sigma [n][C][C] of n images of R rows each.  span: rows per Gram block, a multiple of kRsStage.
template <int C, class Load>
int launch_rows_stats(Load load, long long R, int n, int span, DevBuf& gpart, DevBuf& mpart, double* mu, double* sigma, hipStream_t st) {
    static_assert(C == 32 || C == 64 || C == 192, "k_rows_gram: 16-column blocks in groups of four, or two of them");
    S3D_CHECK(span > 0 && span % kRsStage == 0, S3D_ERR_INVALID, "rows statistics: a span of %d rows is no multiple of %d", span, kRsStage);
    S3D_TRY(reserve_rows_stats(C, R, n, span, gpart, mpart));
    const int nparts = int((R + span - 1) / span);
    double* gp = static_cast<double*>(gpart.p);
    double* mp = static_cast<double*>(mpart.p);
    hipLaunchKernelGGL((k_rows_gram<C, Load>), dim3((unsigned)nparts, C / 64 > 0 ? C / 64 : 1, (unsigned)n), dim3(kRsThreads), 0, st, load, R, span,
                       nparts, gp, mp);
    S3D_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_rows_cov, dim3((unsigned)(C * C / 16), (unsigned)n), dim3(kRsThreads), 0, st, gp, mp, nparts, C, double(R), mu, sigma);
    S3D_HIP(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------ stage timing of a handle
// N stages between N + 1 device events.  The events are created when timing is first switched on; a call marks them as it goes
// and sets `timed` at its end; read gives the milliseconds of the last timed call.
template <int N>
struct StageTimer {
    bool on = false, timed = false;
    hipEvent_t ev[N + 1] = {};
    ~StageTimer() {
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
    int enable(bool want) {
        if (want)
            for (hipEvent_t& e : ev)
                if (!e) S3D_HIP(hipEventCreate(&e));
        on = want;
        timed = false;
        return 0;
    }
    int mark(int i, hipStream_t st) {
        if (on) S3D_HIP(hipEventRecord(ev[i], st));
        return 0;
    }
    int read(const char* what, double* ms) {             // what: "ssfid" / "imgfeat", as in the entry points' names
        S3D_CHECK(timed, S3D_ERR_INVALID, "%s_profile_read: no call has been timed (s3d_%s_profile(h, 1), then s3d_%s_features)", what, what, what);
        S3D_HIP(hipEventSynchronize(ev[N]));
        for (int i = 0; i < N; ++i) {
            float t = 0.f;
            S3D_HIP(hipEventElapsedTime(&t, ev[i], ev[i + 1]));
            ms[i] = double(t);
        }
        return 0;
    }
};

// ------------------------------------------------------------------ the shape of a parameter
// shape [ndim] against want [wdim]: 0 and the element count in n, or "<what> set_param: <name> has shape [a, b, c]; <hint>".
inline int check_param_shape(const char* what, const char* name, const int64_t* shape, int ndim, const int64_t* want, int wdim, const char* hint,
                             size_t& n) {
    bool ok = ndim == wdim;
    n = 1;
    for (int k = 0; ok && k < ndim; ++k) { ok = shape[k] == want[k]; n *= size_t(shape[k]); }
    if (ok) return 0;
    std::string got;
    for (int k = 0; k < ndim && k < 8; ++k) got += (k ? ", " : "") + std::to_string((long long)shape[k]);
    set_error("%s set_param: %s has shape [%s]; %s", what, name, got.c_str(), hint);
    return S3D_ERR_UNSUPPORTED;
}

}  // namespace s3d
