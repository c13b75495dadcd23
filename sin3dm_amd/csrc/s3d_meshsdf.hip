// s3d_meshsdf.hip — a triangle mesh to training data on the device (the reference's data/mesh_sampler.py, by an own design;
// DESIGN.md §16): exact closest point inside a band through a uniform cell grid, the generalized winding number for the sign,
// area-weighted surface samples and nearest-texel colours.  Triangles come as their nine corner floats [F][9] (the caller gathers
// verts[tris] once), so no kernel follows a vertex index.  Sort, scan and compaction stay with the caller (torch), as for
// s3d_tex.hip.  No float atomics; every output element is written by one thread that adds in a fixed order, so the results do not
// depend on the launch geometry.
#include "s3d_cellgrid.h"

namespace s3d {

constexpr int kMeshThreads = 256;
constexpr int kWindTile = 256;                 // triangles staged in LDS per round of k_mesh_winding: 256 * 9 floats = 9216 bytes
constexpr int kWindPts = 2;                    // points per lane of k_mesh_winding
static inline unsigned mesh_blocks(long long n) { return (unsigned)((n + kMeshThreads - 1) / kMeshThreads); }

// what a triangle's box is dilated by: a little more than the band, so that rounding in lo - band never excludes a cell that
// holds a point nearer than the band
__device__ __forceinline__ float dilation(float band) { return band * 1.001f + 1e-6f; }

__device__ __forceinline__ void tri_cell_range(const float* __restrict__ t, float band, const CellGrid& g, int lo[3], int hi[3]) {
    const float d = dilation(band);
    const float o[3] = {g.ox, g.oy, g.oz};
    const int n[3] = {g.nx, g.ny, g.nz};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float mn = fminf(t[k], fminf(t[3 + k], t[6 + k])), mx = fmaxf(t[k], fmaxf(t[3 + k], t[6 + k]));
        lo[k] = cell_of(mn - d, o[k], g.cell, n[k]);
        hi[k] = cell_of(mx + d, o[k], g.cell, n[k]);
    }
}

// ------------------------------------------------------------------ binning: (cell, triangle) pairs of the band-dilated boxes
__global__ void __launch_bounds__(kMeshThreads) k_mesh_bin_count(const float* __restrict__ tri9, long long F, float band, CellGrid g,
                                                                 long long* __restrict__ counts) {
    const long long f = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= F) return;
    float t[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) t[k] = tri9[f * 9 + k];
    int lo[3], hi[3];
    tri_cell_range(t, band, g, lo, hi);
    counts[f] = (long long)(hi[0] - lo[0] + 1) * (hi[1] - lo[1] + 1) * (hi[2] - lo[2] + 1);
}

// offsets = exclusive scan of counts; a triangle writes its pairs at [offsets[f], offsets[f] + count) in ascending cell order and
// never past n_pairs
__global__ void __launch_bounds__(kMeshThreads) k_mesh_bin_fill(const float* __restrict__ tri9, long long F, float band, CellGrid g,
                                                                const long long* __restrict__ offsets, long long n_pairs,
                                                                long long* __restrict__ pair_cell, int* __restrict__ pair_tri) {
    const long long f = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= F) return;
    float t[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) t[k] = tri9[f * 9 + k];
    int lo[3], hi[3];
    tri_cell_range(t, band, g, lo, hi);
    long long o = offsets[f];
    if (o < 0) return;
    for (int ix = lo[0]; ix <= hi[0]; ++ix)
        for (int iy = lo[1]; iy <= hi[1]; ++iy)
            for (int iz = lo[2]; iz <= hi[2]; ++iz) {
                if (o >= n_pairs) return;
                pair_cell[o] = ((long long)ix * g.ny + iy) * g.nz + iz;
                pair_tri[o] = int(f);
                ++o;
            }
}

// ------------------------------------------------------------------ closest point on a triangle: barycentrics of a, b, c and the
// squared distance.  Ericson's region test (Real-Time Collision Detection 5.1.5: the Voronoi region of the point decides between a
// vertex, an edge and the face) is exact in exact arithmetic, but va, vb and vc are differences of products: on a needle or cap
// sliver, or a face without area, their true value lies below their rounding in fp32, the wrong region is chosen and the answer is
// a point of the triangle far from the nearest one (or 0 / 0).  So its answer is one candidate of four: the other three are the
// projections onto the edges ab, ac and bc, clamped to the segment.  Every candidate is a point of the triangle (barycentrics
// clamped to >= 0 with sum 1), so none lies nearer than the truth; the edges bound the result by the distance to the boundary,
// which is the distance itself where the face has no area and at most a sliver's height above it otherwise.  The nearest
// candidate by the squared distance reconstructed from its own barycentrics wins, the earlier one on a tie, a NaN never.
__device__ __forceinline__ float bary_dist2(const float p[3], const float* __restrict__ t, float b0, float b1, float b2) {
    float d2 = 0.0f;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float q = b0 * t[k] + b1 * t[3 + k] + b2 * t[6 + k] - p[k];
        d2 += q * q;
    }
    return d2;
}
__device__ __forceinline__ float clamp01(float x) { return fminf(fmaxf(x, 0.0f), 1.0f); }      // (fmaxf drops a NaN: 0)

__device__ __forceinline__ float closest_on_triangle(const float p[3], const float* __restrict__ t, float bc[3]) {
    float ab[3], ac[3], cb[3], ap[3], bp[3], cp[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        ab[k] = t[3 + k] - t[k]; ac[k] = t[6 + k] - t[k]; cb[k] = t[6 + k] - t[3 + k];
        ap[k] = p[k] - t[k]; bp[k] = p[k] - t[3 + k]; cp[k] = p[k] - t[6 + k];
    }
    const float d1 = ab[0] * ap[0] + ab[1] * ap[1] + ab[2] * ap[2], d2 = ac[0] * ap[0] + ac[1] * ap[1] + ac[2] * ap[2];
    const float d3 = ab[0] * bp[0] + ab[1] * bp[1] + ab[2] * bp[2], d4 = ac[0] * bp[0] + ac[1] * bp[1] + ac[2] * bp[2];
    const float d5 = ab[0] * cp[0] + ab[1] * cp[1] + ab[2] * cp[2], d6 = ac[0] * cp[0] + ac[1] * cp[1] + ac[2] * cp[2];
    const float vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
    // candidate 0: the region test
    float e0, e1, e2;
    if (d1 <= 0.0f && d2 <= 0.0f) { e0 = 1.0f; e1 = 0.0f; e2 = 0.0f; }
    else if (d3 >= 0.0f && d4 <= d3) { e0 = 0.0f; e1 = 1.0f; e2 = 0.0f; }
    else if (vc <= 0.0f && d1 >= 0.0f && d3 <= 0.0f) {
        const float v = __fdiv_rn(d1, d1 - d3);                   // in [0, 1], or NaN where a == b
        e0 = 1.0f - v; e1 = v; e2 = 0.0f;
    } else if (d6 >= 0.0f && d5 <= d6) { e0 = 0.0f; e1 = 0.0f; e2 = 1.0f; }
    else if (vb <= 0.0f && d2 >= 0.0f && d6 <= 0.0f) {
        const float w = __fdiv_rn(d2, d2 - d6);
        e0 = 1.0f - w; e1 = 0.0f; e2 = w;
    } else if (va <= 0.0f && (d4 - d3) >= 0.0f && (d5 - d6) >= 0.0f) {
        const float w = __fdiv_rn(d4 - d3, (d4 - d3) + (d5 - d6));
        e0 = 0.0f; e1 = 1.0f - w; e2 = w;
    } else {
        const float den = va + vb + vc;
        const float v = clamp01(__fdiv_rn(vb, den)), u = 1.0f - v;
        const float w = fminf(fmaxf(__fdiv_rn(vc, den), 0.0f), u);     // (v + w may round past 1 on an edge; past anything on a sliver)
        e0 = u - w; e1 = v; e2 = w;
    }
    float best = INFINITY;
    bc[0] = 1.0f; bc[1] = 0.0f; bc[2] = 0.0f;
    {
        const float d = bary_dist2(p, t, e0, e1, e2);
        if (d < best) { best = d; bc[0] = e0; bc[1] = e1; bc[2] = e2; }
    }
    // candidates 1 to 3: the edges ab, ac, bc
    {
        const float l2 = ab[0] * ab[0] + ab[1] * ab[1] + ab[2] * ab[2];
        const float s = l2 > 0.0f ? clamp01(__fdiv_rn(d1, l2)) : 0.0f;
        const float d = bary_dist2(p, t, 1.0f - s, s, 0.0f);
        if (d < best) { best = d; bc[0] = 1.0f - s; bc[1] = s; bc[2] = 0.0f; }
    }
    {
        const float l2 = ac[0] * ac[0] + ac[1] * ac[1] + ac[2] * ac[2];
        const float s = l2 > 0.0f ? clamp01(__fdiv_rn(d2, l2)) : 0.0f;
        const float d = bary_dist2(p, t, 1.0f - s, 0.0f, s);
        if (d < best) { best = d; bc[0] = 1.0f - s; bc[1] = 0.0f; bc[2] = s; }
    }
    {
        const float l2 = cb[0] * cb[0] + cb[1] * cb[1] + cb[2] * cb[2];
        const float s = l2 > 0.0f ? clamp01(__fdiv_rn(cb[0] * bp[0] + cb[1] * bp[1] + cb[2] * bp[2], l2)) : 0.0f;
        const float d = bary_dist2(p, t, 0.0f, 1.0f - s, s);
        if (d < best) { best = d; bc[0] = 0.0f; bc[1] = 1.0f - s; bc[2] = s; }
    }
    return best;
}

// One thread per query point: the triangles of its cell's segment, the minimum squared distance kept (finite for every face: an
// edge candidate always is), a tie to the lower face index (so the order inside the segment does not matter).  dist = the
// distance, or `band` with face -1 and zero barycentrics when nothing lies nearer than the band.  A point outside the grid looks
// its border cell up: the grid covers the mesh dilated by the band, so such a point has nothing within the band and the walk finds
// nothing either.
__global__ void __launch_bounds__(kMeshThreads) k_mesh_closest(const float* __restrict__ pts, long long N, const float* __restrict__ tri9,
                                                               long long F, float band, CellGrid g, const long long* __restrict__ seg,
                                                               const int* __restrict__ seg_tri, long long n_pairs,
                                                               float* __restrict__ dist, int* __restrict__ face, float* __restrict__ bary) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const float p[3] = {pts[i * 3], pts[i * 3 + 1], pts[i * 3 + 2]};
    const long long c = ((long long)cell_of(p[0], g.ox, g.cell, g.nx) * g.ny + cell_of(p[1], g.oy, g.cell, g.ny)) * g.nz +
                        cell_of(p[2], g.oz, g.cell, g.nz);
    const long long b = max(0LL, seg[c]), e = min(n_pairs, seg[c + 1]);
    float best = INFINITY, bb[3] = {0.0f, 0.0f, 0.0f};
    int bf = -1;
    for (long long j = b; j < e; ++j) {
        const int f = seg_tri[j];
        if (f < 0 || f >= F) continue;
        const float* t = tri9 + (long long)f * 9;
        float bc[3];
        const float d2 = closest_on_triangle(p, t, bc);
        if (d2 < best || (d2 == best && f < bf)) { best = d2; bf = f; bb[0] = bc[0]; bb[1] = bc[1]; bb[2] = bc[2]; }
    }
    float d = bf >= 0 ? sqrtf(best) : band;
    if (!(d < band)) { d = band; bf = -1; bb[0] = bb[1] = bb[2] = 0.0f; }
    dist[i] = d;
    face[i] = bf;
    bary[i * 3] = bb[0]; bary[i * 3 + 1] = bb[1]; bary[i * 3 + 2] = bb[2];
}

// ------------------------------------------------------------------ generalized winding number (Jacobson et al. 2013) from the solid
// angle of every triangle (Van Oosterom & Strackee 1983): tan(omega / 2) = a.(b x c) / (|a||b||c| + a.b |c| + b.c |a| + c.a |b|)
// with a, b, c the corners seen from the point.  wn = sum omega / (4 pi).  All points x all faces: a block stages kWindTile
// triangles in LDS, every lane reads the same triangle (a broadcast, no bank conflict) and adds it to its kWindPts points, so each
// point adds the faces in index order (in double: one add per solid angle, beside ~100 fp32 operations).
__device__ __forceinline__ float solid_angle_half(const float p[3], const float* t) {
    const float a[3] = {t[0] - p[0], t[1] - p[1], t[2] - p[2]}, b[3] = {t[3] - p[0], t[4] - p[1], t[5] - p[2]},
                c[3] = {t[6] - p[0], t[7] - p[1], t[8] - p[2]};
    // the hardware square root (1 ulp, no denormal rescue: a squared length is 0 or far above the denormals), a third of the
    // correctly rounded sequence's instructions
    const float la = __builtin_amdgcn_sqrtf(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]), lb = __builtin_amdgcn_sqrtf(b[0] * b[0] + b[1] * b[1] + b[2] * b[2]),
                lc = __builtin_amdgcn_sqrtf(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]);
    const float num = a[0] * (b[1] * c[2] - b[2] * c[1]) + a[1] * (b[2] * c[0] - b[0] * c[2]) + a[2] * (b[0] * c[1] - b[1] * c[0]);
    const float ab = a[0] * b[0] + a[1] * b[1] + a[2] * b[2], bc = b[0] * c[0] + b[1] * c[1] + b[2] * c[2],
                ca = c[0] * a[0] + c[1] * a[1] + c[2] * a[2];
    return atan2f(num, la * lb * lc + ab * lc + bc * la + ca * lb);
}

__global__ void __launch_bounds__(kMeshThreads) k_mesh_winding(const float* __restrict__ pts, long long N, const float* __restrict__ tri9,
                                                               long long F, float* __restrict__ wn) {
    __shared__ float tile[kWindTile * 9];
    const long long base = (long long)blockIdx.x * (kMeshThreads * kWindPts) + threadIdx.x;
    float p[kWindPts][3];
    double acc[kWindPts];
#pragma unroll
    for (int j = 0; j < kWindPts; ++j) {
        const long long i = base + (long long)j * kMeshThreads;
        const bool ok = i < N;
#pragma unroll
        for (int k = 0; k < 3; ++k) p[j][k] = ok ? pts[i * 3 + k] : 0.0f;
        acc[j] = 0.0;
    }
    for (long long f0 = 0; f0 < F; f0 += kWindTile) {
        const int cnt = int(min((long long)kWindTile, F - f0));
        __syncthreads();                                       // the previous tile has been read by every lane
        for (int k = threadIdx.x; k < cnt * 9; k += kMeshThreads) tile[k] = tri9[f0 * 9 + k];
        __syncthreads();
        for (int f = 0; f < cnt; ++f) {
#pragma unroll
            for (int j = 0; j < kWindPts; ++j) acc[j] += double(solid_angle_half(p[j], tile + f * 9));
        }
    }
#pragma unroll
    for (int j = 0; j < kWindPts; ++j) {
        const long long i = base + (long long)j * kMeshThreads;
        if (i < N) wn[i] = float(acc[j] * (1.0 / (2.0 * 3.14159265358979323846)));      // 2 * sum(omega / 2) / (4 pi)
    }
}

// ------------------------------------------------------------------ surface samples
__global__ void __launch_bounds__(kMeshThreads) k_mesh_face_areas(const float* __restrict__ tri9, long long F, float* __restrict__ area) {
    const long long f = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= F) return;
    const float* t = tri9 + f * 9;
    const float u[3] = {t[3] - t[0], t[4] - t[1], t[5] - t[2]}, v[3] = {t[6] - t[0], t[7] - t[1], t[8] - t[2]};
    const float nx = u[1] * v[2] - u[2] * v[1], ny = u[2] * v[0] - u[0] * v[2], nz = u[0] * v[1] - u[1] * v[0];
    area[f] = 0.5f * sqrtf(nx * nx + ny * ny + nz * nz);
}

// One thread per sample from three uniforms in [0, 1): the face is the first one whose inclusive area sum exceeds u0 * total
// (binary search), the barycentrics follow the square-root rule b = (1 - sqrt(u1), sqrt(u1) (1 - u2), sqrt(u1) u2)
__global__ void __launch_bounds__(kMeshThreads) k_mesh_sample_surface(const float* __restrict__ tri9, long long F, const double* __restrict__ cdf,
                                                                      const float* __restrict__ u, long long N, float* __restrict__ pts,
                                                                      int* __restrict__ face, float* __restrict__ bary) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const double target = double(u[i * 3]) * cdf[F - 1];
    long long lo = 0, hi = F - 1;                               // the answer lies in [lo, hi]
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (cdf[mid] > target) hi = mid; else lo = mid + 1;
    }
    const float* t = tri9 + lo * 9;
    const float r = sqrtf(u[i * 3 + 1]), u2 = u[i * 3 + 2];
    const float b0 = 1.0f - r, b1 = r * (1.0f - u2), b2 = r * u2;
    face[i] = int(lo);
    bary[i * 3] = b0; bary[i * 3 + 1] = b1; bary[i * 3 + 2] = b2;
#pragma unroll
    for (int k = 0; k < 3; ++k) pts[i * 3 + k] = b0 * t[k] + b1 * t[3 + k] + b2 * t[6 + k];
}

// ------------------------------------------------------------------ colour of (face, barycentrics): the nearest texel of the face's
// material image at the interpolated uv — x = round(u (W - 1)) mod W, y = round((1 - v) (H - 1)) mod H, rounding half to even —
// or the material's Kd when it has no image (W == 0) or the texel would lie outside the packed buffer.  mat [M][3] = {byte offset, W,
// H} of tightly packed RGB rows; face -1 gives 0.
__global__ void __launch_bounds__(kMeshThreads) k_mesh_texture(const int* __restrict__ face, const float* __restrict__ bary, long long N,
                                                               const float* __restrict__ uv, const int* __restrict__ face_mat, long long F,
                                                               const long long* __restrict__ mat, const float* __restrict__ kd, int M,
                                                               const unsigned char* __restrict__ img, long long img_bytes,
                                                               float* __restrict__ out) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const int f = face[i];
    float c[3] = {0.0f, 0.0f, 0.0f};
    if (f >= 0 && f < F) {
        const int m = face_mat[f];
        if (m >= 0 && m < M) {
            const long long off = mat[m * 3], W = mat[m * 3 + 1], H = mat[m * 3 + 2];
            c[0] = kd[m * 3]; c[1] = kd[m * 3 + 1]; c[2] = kd[m * 3 + 2];
            if (W > 0 && H > 0 && off >= 0 && W <= 65536 && H <= 65536 && off + W * H * 3 <= img_bytes) {
                const float b0 = bary[i * 3], b1 = bary[i * 3 + 1], b2 = bary[i * 3 + 2];
                const float* q = uv + (long long)f * 6;
                const float tu = b0 * q[0] + b1 * q[2] + b2 * q[4], tv = b0 * q[1] + b1 * q[3] + b2 * q[5];
                const float fx = rintf(tu * float(W - 1)), fy = rintf((1.0f - tv) * float(H - 1));
                if (fabsf(fx) < 1e9f && fabsf(fy) < 1e9f) {                    // (a NaN or runaway uv keeps Kd)
                    const long long x = (((long long)fx % W) + W) % W, y = (((long long)fy % H) + H) % H;
                    const unsigned char* px = img + off + (y * W + x) * 3;
#pragma unroll
                    for (int k = 0; k < 3; ++k) c[k] = __fdiv_rn(float(px[k]), 255.0f);
                }
            }
        }
    }
    out[i * 3] = c[0]; out[i * 3 + 1] = c[1]; out[i * 3 + 2] = c[2];
}

static int check_grid(const char* who, const float origin[3], float cell, const int dims[3], float band, CellGrid& g) {
    S3D_CHECK(origin && dims, S3D_ERR_INVALID, "%s: null grid argument", who);
    S3D_CHECK(band > 0.0f && cell > 0.0f && std::isfinite(band) && std::isfinite(cell) && std::isfinite(origin[0]) && std::isfinite(origin[1]) &&
                  std::isfinite(origin[2]),
              S3D_ERR_INVALID, "%s: band %g, cell edge %g", who, double(band), double(cell));
    S3D_CHECK(dims[0] >= 1 && dims[1] >= 1 && dims[2] >= 1 && (long long)dims[0] * dims[1] * (long long)dims[2] <= S3D_MESHSDF_MAX_CELLS,
              S3D_ERR_INVALID, "%s: cell grid %d x %d x %d (at most %lld cells)", who, dims[0], dims[1], dims[2], (long long)S3D_MESHSDF_MAX_CELLS);
    g = CellGrid{origin[0], origin[1], origin[2], cell, dims[0], dims[1], dims[2]};
    return 0;
}

}  // namespace s3d

using namespace s3d;

extern "C" {

int s3d_meshsdf_bin_count(const float* tri9, int64_t n_faces, float band, const float origin[3], float cell, const int dims[3],
                          int64_t* counts, void* stream) {
    CellGrid g;
    S3D_TRY(check_grid("meshsdf_bin_count", origin, cell, dims, band, g));
    S3D_CHECK(n_faces >= 0 && n_faces <= INT32_MAX && (n_faces == 0 || (tri9 && counts)), S3D_ERR_INVALID, "meshsdf_bin_count: %lld faces or a null argument",
              (long long)n_faces);
    if (!n_faces) return 0;
    hipLaunchKernelGGL(k_mesh_bin_count, dim3(mesh_blocks(n_faces)), dim3(kMeshThreads), 0, static_cast<hipStream_t>(stream), tri9,
                       (long long)n_faces, band, g, reinterpret_cast<long long*>(counts));
    S3D_HIP(hipGetLastError());
    return 0;
}

int s3d_meshsdf_bin_fill(const float* tri9, int64_t n_faces, float band, const float origin[3], float cell, const int dims[3],
                         const int64_t* offsets, int64_t n_pairs, int64_t* pair_cell, int32_t* pair_tri, void* stream) {
    CellGrid g;
    S3D_TRY(check_grid("meshsdf_bin_fill", origin, cell, dims, band, g));
    S3D_CHECK(n_faces >= 0 && n_faces <= INT32_MAX && n_pairs >= 0, S3D_ERR_INVALID, "meshsdf_bin_fill: bad sizes");
    S3D_CHECK(n_pairs <= S3D_MESHSDF_MAX_PAIRS, S3D_ERR_UNSUPPORTED,
              "meshsdf_bin_fill: %lld (cell, triangle) pairs need %.2f GiB of workspace (12 bytes a pair), more than the cap of %lld pairs = 1.5 GiB: "
              "the band is too wide for this mesh",
              (long long)n_pairs, double(n_pairs) * 12.0 / double(1 << 30), (long long)S3D_MESHSDF_MAX_PAIRS);
    S3D_CHECK(n_faces == 0 || n_pairs == 0 || (tri9 && offsets && pair_cell && pair_tri), S3D_ERR_INVALID, "meshsdf_bin_fill: null argument");
    if (!n_faces || !n_pairs) return 0;
    hipLaunchKernelGGL(k_mesh_bin_fill, dim3(mesh_blocks(n_faces)), dim3(kMeshThreads), 0, static_cast<hipStream_t>(stream), tri9,
                       (long long)n_faces, band, g, reinterpret_cast<const long long*>(offsets), (long long)n_pairs,
                       reinterpret_cast<long long*>(pair_cell), pair_tri);
    S3D_HIP(hipGetLastError());
    return 0;
}

int s3d_meshsdf_closest(const float* points, int64_t n_points, const float* tri9, int64_t n_faces, float band, const float origin[3],
                        float cell, const int dims[3], const int64_t* seg, const int32_t* seg_tri, int64_t n_pairs, float* dist,
                        int32_t* face, float* bary, void* stream) {
    CellGrid g;
    S3D_TRY(check_grid("meshsdf_closest", origin, cell, dims, band, g));
    S3D_CHECK(n_points >= 0 && n_faces >= 0 && n_faces <= INT32_MAX && n_pairs >= 0 && n_pairs <= S3D_MESHSDF_MAX_PAIRS, S3D_ERR_INVALID,
              "meshsdf_closest: bad sizes");
    S3D_CHECK(n_points == 0 || (points && seg && dist && face && bary && (n_pairs == 0 || (seg_tri && tri9))), S3D_ERR_INVALID,
              "meshsdf_closest: null argument");
    if (!n_points) return 0;
    hipLaunchKernelGGL(k_mesh_closest, dim3(mesh_blocks(n_points)), dim3(kMeshThreads), 0, static_cast<hipStream_t>(stream), points,
                       (long long)n_points, tri9, (long long)n_faces, band, g, reinterpret_cast<const long long*>(seg), seg_tri,
                       (long long)n_pairs, dist, face, bary);
    S3D_HIP(hipGetLastError());
    return 0;
}

int s3d_meshsdf_winding(const float* points, int64_t n_points, const float* tri9, int64_t n_faces, float* wn, void* stream) {
    S3D_CHECK(n_points >= 0 && n_faces >= 0 && n_faces <= INT32_MAX, S3D_ERR_INVALID, "meshsdf_winding: bad sizes");
    S3D_CHECK(n_points == 0 || (points && wn && (n_faces == 0 || tri9)), S3D_ERR_INVALID, "meshsdf_winding: null argument");
    if (!n_points) return 0;
    const long long per_block = (long long)kMeshThreads * kWindPts, blocks = (n_points + per_block - 1) / per_block;
    S3D_CHECK(blocks <= INT32_MAX, S3D_ERR_UNSUPPORTED, "meshsdf_winding: %lld points in one call", (long long)n_points);
    hipLaunchKernelGGL(k_mesh_winding, dim3((unsigned)blocks), dim3(kMeshThreads), 0, static_cast<hipStream_t>(stream), points,
                       (long long)n_points, tri9, (long long)n_faces, wn);
    S3D_HIP(hipGetLastError());
    return 0;
}

int s3d_meshsdf_face_areas(const float* tri9, int64_t n_faces, float* areas, void* stream) {
    S3D_CHECK(n_faces >= 0 && n_faces <= INT32_MAX && (n_faces == 0 || (tri9 && areas)), S3D_ERR_INVALID, "meshsdf_face_areas: %lld faces or a null argument",
              (long long)n_faces);
    if (!n_faces) return 0;
    hipLaunchKernelGGL(k_mesh_face_areas, dim3(mesh_blocks(n_faces)), dim3(kMeshThreads), 0, static_cast<hipStream_t>(stream), tri9,
                       (long long)n_faces, areas);
    S3D_HIP(hipGetLastError());
    return 0;
}

int s3d_meshsdf_sample_surface(const float* tri9, int64_t n_faces, const double* cdf, const float* uniforms, int64_t n, float* points,
                               int32_t* face, float* bary, void* stream) {
    S3D_CHECK(n >= 0 && n_faces >= 0 && n_faces <= INT32_MAX, S3D_ERR_INVALID, "meshsdf_sample_surface: bad sizes");
    S3D_CHECK(n == 0 || n_faces >= 1, S3D_ERR_INVALID, "meshsdf_sample_surface: no faces to sample");
    S3D_CHECK(n == 0 || (tri9 && cdf && uniforms && points && face && bary), S3D_ERR_INVALID, "meshsdf_sample_surface: null argument");
    if (!n) return 0;
    hipLaunchKernelGGL(k_mesh_sample_surface, dim3(mesh_blocks(n)), dim3(kMeshThreads), 0, static_cast<hipStream_t>(stream), tri9,
                       (long long)n_faces, cdf, uniforms, (long long)n, points, face, bary);
    S3D_HIP(hipGetLastError());
    return 0;
}

int s3d_meshsdf_texture(const int32_t* face, const float* bary, int64_t n, const float* uv, const int32_t* face_mat, int64_t n_faces,
                        const int64_t* mat_table, const float* mat_kd, int n_mats, const uint8_t* images, int64_t image_bytes, float* colors,
                        void* stream) {
    S3D_CHECK(n >= 0 && n_faces >= 0 && n_faces <= INT32_MAX && n_mats >= 0 && n_mats <= (1 << 20) && image_bytes >= 0, S3D_ERR_INVALID,
              "meshsdf_texture: bad sizes");
    S3D_CHECK(n == 0 || (face && bary && colors), S3D_ERR_INVALID, "meshsdf_texture: null argument");
    S3D_CHECK(n_faces == 0 || (uv && face_mat), S3D_ERR_INVALID, "meshsdf_texture: null face table");
    S3D_CHECK(n_mats == 0 || (mat_table && mat_kd), S3D_ERR_INVALID, "meshsdf_texture: null material table");
    S3D_CHECK(image_bytes == 0 || images, S3D_ERR_INVALID, "meshsdf_texture: null image buffer");
    if (!n) return 0;
    hipLaunchKernelGGL(k_mesh_texture, dim3(mesh_blocks(n)), dim3(kMeshThreads), 0, static_cast<hipStream_t>(stream), face, bary,
                       (long long)n, uv, face_mat, (long long)n_faces, reinterpret_cast<const long long*>(mat_table), mat_kd, n_mats, images,
                       (long long)image_bytes, colors);
    S3D_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
