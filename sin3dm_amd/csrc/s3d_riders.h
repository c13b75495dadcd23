// s3d_riders.h — device bodies of the three small GroupNorm launches that a 1x1 convolution can carry (ConvRider, s3d_common.h).
// Each body is one block of its kernel: s3d_kernels.hip wraps it in the __global__ kernel every other caller launches, and
// k_conv_mfma_rider (s3d_conv.hip) runs it in the blocks ahead of the convolution's own.  One source, the same sums either way.
#pragma once
#include "s3d_common.h"

namespace s3d {

__device__ __forceinline__ void gn_acc(double s[4], double ss[4], const float4& v) {
    s[0] += v.x; ss[0] += double(v.x) * v.x;
    s[1] += v.y; ss[1] += double(v.y) * v.y;
    s[2] += v.z; ss[2] += double(v.z) * v.z;
    s[3] += v.w; ss[3] += double(v.w) * v.w;
}

// fixed-order reduction of one double per thread over a 256-thread block: butterfly inside each wave (the same pairing for
// every launch), then the four wave sums in wave order: bit-repeatable
__device__ __forceinline__ double block_sum256(double v, double* sm4) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    if ((threadIdx.x & 63) == 0) sm4[threadIdx.x >> 6] = v;
    __syncthreads();
    const double r = (sm4[0] + sm4[1]) + (sm4[2] + sm4[3]);
    __syncthreads();
    return r;
}

// Eight consecutive output rows i0..i0+7 (i0 a multiple of 8) of output column j: the six low-resolution rows they touch
// are interpolated horizontally once (12 loads instead of 32) and combined with the per-row weights of the exact formula;
// the values equal up2x_sample's bit for bit (same products, same order).
struct Up8Rows { int rk[6]; float ly0[8], ly1[8]; };
__device__ __forceinline__ Up8Rows up8_rows(int i0, int hi) {
    Up8Rows R;
    const int base = (i0 >> 1) - 1;
#pragma unroll
    for (int k = 0; k < 6; ++k) { const int r = base + k; R.rk[k] = r < 0 ? 0 : (r > hi - 1 ? hi - 1 : r); }
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        float fy = 0.5f * (float(i0 + r) + 0.5f) - 0.5f; fy = fy < 0.f ? 0.f : fy;
        int y0 = int(fy); y0 = y0 > hi - 1 ? hi - 1 : y0;
        R.ly1[r] = fy - float(y0); R.ly0[r] = 1.f - R.ly1[r];
    }
    return R;
}
__device__ __forceinline__ void up8_column(const float4* __restrict__ src, int wi, int cuq, const Up8Rows& R, int j, float4 out[8]) {
    float fx = 0.5f * (float(j) + 0.5f) - 0.5f; fx = fx < 0.f ? 0.f : fx;
    int x0 = int(fx); x0 = x0 > wi - 1 ? wi - 1 : x0;
    const int x1 = x0 + (x0 < wi - 1 ? 1 : 0);
    const float lx1 = fx - float(x0), lx0 = 1.f - lx1;
    float4 hl[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const float4 a = src[(size_t(R.rk[k]) * wi + x0) * cuq], b = src[(size_t(R.rk[k]) * wi + x1) * cuq];
        hl[k].x = lx0 * a.x + lx1 * b.x; hl[k].y = lx0 * a.y + lx1 * b.y; hl[k].z = lx0 * a.z + lx1 * b.z; hl[k].w = lx0 * a.w + lx1 * b.w;
    }
    // output row r uses low-resolution rows (base + ka, base + ka + 1): ka = (r + 1) >> 1
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const float4 p = hl[(r + 1) >> 1], q = hl[((r + 1) >> 1) + 1];
        out[r].x = R.ly0[r] * p.x + R.ly1[r] * q.x; out[r].y = R.ly0[r] * p.y + R.ly1[r] * q.y;
        out[r].z = R.ly0[r] * p.z + R.ly1[r] * q.z; out[r].w = R.ly0[r] * p.w + R.ly1[r] * q.w;
    }
}

// k_gn_finalize: block (g, p, b) of grid (32, 3, B), 256 threads; sm4: four doubles of LDS
__device__ __forceinline__ void gn_finalize_block(const GnFinArgs& a, int g, int p, int b, double* sm4) {
    const int tid = threadIdx.x;
    const double* base = a.part + (size_t(b) * 3 + p) * a.maxparts * a.nsub * 2;
    double S = 0, SS = 0;
    for (int k = 0; k < a.subs_per_group; ++k) {               // [sub][part]: a group's parts are contiguous
        const double2* row = reinterpret_cast<const double2*>(base + (size_t(g) * a.subs_per_group + k) * a.maxparts * 2);
        for (int part = tid; part < a.nparts[p]; part += 256) { const double2 v = row[part]; S += v.x; SS += v.y; }
    }
    S = block_sum256(S, sm4);
    SS = block_sum256(SS, sm4);
    if (tid == 0) {
        const double m = S / a.count[p];
        double var = SS / a.count[p] - m * m;
        if (var < 0) var = 0;
        float* o = a.mr + ((size_t(b) * 3 + p) * 32 + g) * 2;
        o[0] = float(m);
        o[1] = float(1.0 / sqrt(var + 1e-5));
    }
}

// k_gn_partials_up: block (tile, p, b) of grid (maxtiles, 3, B), cq * pl threads; sm: [pl][C][2] doubles of LDS
__device__ __forceinline__ void gn_partials_up_block(const GnPartUpArgs& a, int tile, int p, int b, double* sm) {
    const int hi = a.hi[p], wi = a.wi[p], h = 2 * hi, w = 2 * wi;
    const int ntc = (w + kActCols - 1) / kActCols, ntr = (h + kActRows - 1) / kActRows;
    if (tile >= ntc * ntr) return;
    const int tr = tile / ntc, tc = tile % ntc;
    const int i0 = tr * kActRows, j0 = tc * kActCols, i1 = min(h, i0 + kActRows), j1 = min(w, j0 + kActCols);
    const int q = threadIdx.x % a.cq, l = threadIdx.x / a.cq;
    double s[4] = {0, 0, 0, 0}, ss[4] = {0, 0, 0, 0};
    const float4* src = reinterpret_cast<const float4*>(a.u[p] + size_t(b) * hi * wi * a.C) + q;
    const Up8Rows R = up8_rows(i0, hi);
    for (int j = j0 + l; j < j1; j += a.pl) {
        float4 v[8];
        up8_column(src, wi, a.cq, R, j, v);
#pragma unroll
        for (int r = 0; r < 8; ++r) if (i0 + r < i1) gn_acc(s, ss, v[r]);
    }
    for (int k = 0; k < 4; ++k) {
        sm[(size_t(l) * a.C + 4 * q + k) * 2 + 0] = s[k];
        sm[(size_t(l) * a.C + 4 * q + k) * 2 + 1] = ss[k];
    }
    __syncthreads();
    for (int sub = threadIdx.x; sub < a.nsub; sub += blockDim.x) {
        double S = 0, SS = 0;
        for (int ll = 0; ll < a.pl; ++ll)
            for (int c = sub * a.sg; c < (sub + 1) * a.sg; ++c) { S += sm[(size_t(ll) * a.C + c) * 2]; SS += sm[(size_t(ll) * a.C + c) * 2 + 1]; }
        double* o = a.part + (((size_t(b) * 3 + p) * a.nsub + sub) * a.maxparts + tile) * 2;
        o[0] = S; o[1] = SS;
    }
}

// k_gn_finalize_cat: block (g, p, b) of grid (32, 3, B), 256 threads; sm4: four doubles of LDS
__device__ __forceinline__ void gn_finalize_cat_block(const GnFinCatArgs& a, int g, int p, int b, double* sm4) {
    const int tid = threadIdx.x;
    double S = 0, SS = 0;
    for (int k = 0; k < a.subs_per_group; ++k) {
        const int sub = g * a.subs_per_group + k;
        const bool up = sub < a.nsub_u;
        const double2* row = reinterpret_cast<const double2*>(
            up ? a.pu + (((size_t(b) * 3 + p) * a.nsub_u + sub) * a.maxparts_u) * 2
               : a.ps + (((size_t(b) * 3 + p) * a.nsub_s + (sub - a.nsub_u)) * a.maxparts_s) * 2);
        const int n = up ? a.nparts_u[p] : a.nparts_s[p];
        for (int part = tid; part < n; part += 256) { const double2 v = row[part]; S += v.x; SS += v.y; }
    }
    S = block_sum256(S, sm4);
    SS = block_sum256(SS, sm4);
    if (tid == 0) {
        const double m = S / a.count[p];
        double var = SS / a.count[p] - m * m;
        if (var < 0) var = 0;
        float* o = a.mr + ((size_t(b) * 3 + p) * 32 + g) * 2;
        o[0] = float(m);
        o[1] = float(1.0 / sqrt(var + 1e-5));
    }
}

// logical block `idx` of a rider, as the block of its own kernel's grid (gx, 3, B) with that linear index; lds: kRiderLdsBytes
__device__ __forceinline__ void run_rider(const ConvRider& r, int idx, void* lds) {
    const int x = idx % r.gx, p = (idx / r.gx) % 3, b = idx / (3 * r.gx);
    double* sm = static_cast<double*>(lds);
    if (r.kind == RIDER_GN_PARTIALS_UP) gn_partials_up_block(r.up, x, p, b, sm);
    else if (r.kind == RIDER_GN_FINALIZE) gn_finalize_block(r.fin, x, p, b, sm);
    else if (r.kind == RIDER_GN_FINALIZE_CAT) gn_finalize_cat_block(r.cat, x, p, b, sm);
}

}  // namespace s3d
