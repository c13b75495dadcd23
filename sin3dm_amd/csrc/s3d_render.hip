// s3d_render.hip — multi-view renders of triangle meshes: a tiled rasteriser.  Project (vertices to snapped sample
// coordinates and 1/w), set up and bin ((tile, triangle) pairs of the clamped screen boxes), raster (one workgroup per 16 x 16 tile,
// exact int64 edge functions, nearest 1/w, the lower face on a tie), shade and resolve (perspective-correct attributes, one overhead
// light, the supersamples of a pixel averaged in a fixed order).  Scan and sort between the calls stay with the caller (torch), as
// for s3d_meshsdf.hip.  Every loop bound is known at launch; no float atomics, no communication between workgroups; every output
// element is written by one thread, so the same input gives the same bits.
#include "s3d_render_dev.h"

namespace s3d {

constexpr int kRenderThreads = 256;
constexpr int kRasterTile = S3D_RENDER_TILE;           // samples per tile edge: 16 * 16 = one sample per thread
constexpr int kRasterChunk = 128;                      // triangles staged in LDS per round of k_render_raster: 72 bytes each
static_assert(kRasterTile * kRasterTile == kRenderThreads, "one sample per thread");
static inline unsigned render_blocks(long long n) { return (unsigned)((n + kRenderThreads - 1) / kRenderThreads); }

struct ViewProj { float m[16]; };

// ------------------------------------------------------------------ project: clip = M (x, y, z, 1); sample coordinates with row 0 on
// top, sample (i, j) centred at (i + 0.5, j + 0.5); snapped to 1 / 256.  w <= near (or not a number): inv_w = 0, the flag.
__global__ void __launch_bounds__(kRenderThreads) k_render_project(const float* __restrict__ verts, long long V, ViewProj vp, float ws, float hs,
                                                                   float near, int* __restrict__ xy, float* __restrict__ inv_w) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= V) return;
    const float x = verts[i * 3], y = verts[i * 3 + 1], z = verts[i * 3 + 2];
    const float cx = vp.m[0] * x + vp.m[1] * y + vp.m[2] * z + vp.m[3];
    const float cy = vp.m[4] * x + vp.m[5] * y + vp.m[6] * z + vp.m[7];
    const float cw = vp.m[12] * x + vp.m[13] * y + vp.m[14] * z + vp.m[15];
    int fx = 0, fy = 0;
    float iw = 0.0f;
    if (cw > near && cw < INFINITY) {                                             // (a NaN compares false)
        const float sx = (__fdiv_rn(cx, cw) * 0.5f + 0.5f) * ws, sy = (0.5f - __fdiv_rn(cy, cw) * 0.5f) * hs;
        const float lim = 1073741824.0f;                                          // 2^30: far past kMaxCoord, inside int32
        const float qx = rintf(sx * float(kSub)), qy = rintf(sy * float(kSub));
        fx = int(fminf(fmaxf(qx, -lim), lim));                                    // (fmaxf drops a NaN: -2^30, out of range)
        fy = int(fminf(fmaxf(qy, -lim), lim));
        iw = __fdiv_rn(1.0f, cw);
    }
    xy[i * 2] = fx; xy[i * 2 + 1] = fy;
    inv_w[i] = iw;
}

// (a face on the screen, its edges and the fill rule: s3d_render_dev.h)
// 1 / w at a sample: the edge values are the (unnormalised) screen-space barycentric weights of the opposite corners
__device__ __forceinline__ float depth_at(long long e12, long long e20, long long e01, float iw0, float iw1, float iw2, float area2) {
    return __fdiv_rn(float(e12) * iw0 + float(e20) * iw1 + float(e01) * iw2, area2);
}

// the samples whose centre lies inside the box of the snapped corners, clamped to the grid, as a range of tiles; false: none
__device__ __forceinline__ bool tri_tile_range(const ScreenTri& t, int ws, int hs, int& tx0, int& tx1, int& ty0, int& ty1) {
    const int xmin = min(t.x0, min(t.x1, t.x2)), xmax = max(t.x0, max(t.x1, t.x2));
    const int ymin = min(t.y0, min(t.y1, t.y2)), ymax = max(t.y0, max(t.y1, t.y2));
    // centre of sample i: i * 256 + 128.  first i with centre >= xmin, last with centre <= xmax (>> floors, also below zero)
    const int i0 = max(0, (xmin - kSub / 2 + kSub - 1) >> 8), i1 = min(ws - 1, (xmax - kSub / 2) >> 8);
    const int j0 = max(0, (ymin - kSub / 2 + kSub - 1) >> 8), j1 = min(hs - 1, (ymax - kSub / 2) >> 8);
    if (i0 > i1 || j0 > j1) return false;
    tx0 = i0 / kRasterTile; tx1 = i1 / kRasterTile; ty0 = j0 / kRasterTile; ty1 = j1 / kRasterTile;
    return true;
}
static_assert(kSub == 256, "the shifts above divide by 256");

// ------------------------------------------------------------------ set up and bin
__global__ void __launch_bounds__(kRenderThreads) k_render_bin_count(const int* __restrict__ xy, const float* __restrict__ inv_w, long long V,
                                                                     const int* __restrict__ faces, long long F, int ws, int hs,
                                                                     long long* __restrict__ counts, unsigned char* __restrict__ status) {
    const long long f = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= F) return;
    ScreenTri t;
    const int st = load_screen_tri(xy, inv_w, V, faces, f, t);
    long long n = 0;
    int tx0, tx1, ty0, ty1;
    if (st == TRI_OK && tri_tile_range(t, ws, hs, tx0, tx1, ty0, ty1)) n = (long long)(tx1 - tx0 + 1) * (ty1 - ty0 + 1);
    counts[f] = n;
    status[f] = (unsigned char)st;
}

// offsets = exclusive scan of counts; a triangle writes its pairs at [offsets[f], offsets[f] + count) in ascending tile order and
// never past n_pairs
__global__ void __launch_bounds__(kRenderThreads) k_render_bin_fill(const int* __restrict__ xy, const float* __restrict__ inv_w, long long V,
                                                                    const int* __restrict__ faces, long long F, int ws, int hs, int tiles_x,
                                                                    const long long* __restrict__ offsets, long long n_pairs,
                                                                    int* __restrict__ pair_tile, int* __restrict__ pair_tri) {
    const long long f = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= F) return;
    ScreenTri t;
    int tx0, tx1, ty0, ty1;
    if (load_screen_tri(xy, inv_w, V, faces, f, t) != TRI_OK || !tri_tile_range(t, ws, hs, tx0, tx1, ty0, ty1)) return;
    long long o = offsets[f];
    if (o < 0) return;
    for (int ty = ty0; ty <= ty1; ++ty)
        for (int tx = tx0; tx <= tx1; ++tx) {
            if (o >= n_pairs) return;
            pair_tile[o] = ty * tiles_x + tx;
            pair_tri[o] = int(f);
            ++o;
        }
}

// ------------------------------------------------------------------ raster: block = tile, thread = sample.  The tile's list
// seg_tri[seg[tile] .. seg[tile + 1]) goes through LDS kRasterChunk triangles at a time (thread k sets triangle k up once for all
// 256 samples; every lane then reads the same address, a broadcast).  A triangle covers a sample when all three edge values say
// inside; the largest 1 / w wins, the lower face index on equal 1 / w.
__global__ void __launch_bounds__(kRenderThreads) k_render_raster(const int* __restrict__ xy, const float* __restrict__ inv_w, long long V,
                                                                  const int* __restrict__ faces, long long F, int ws, int hs, int tiles_x,
                                                                  const long long* __restrict__ seg, const int* __restrict__ seg_tri,
                                                                  long long n_pairs, int* __restrict__ face_id, float* __restrict__ depth,
                                                                  unsigned char* __restrict__ count) {
    __shared__ long long sC[kRasterChunk][3];
    __shared__ int sAB[kRasterChunk][6];
    __shared__ float sW[kRasterChunk][4];
    __shared__ int sMeta[kRasterChunk][2];
    const int tile = blockIdx.x, tx = tile % tiles_x, ty = tile / tiles_x;
    const int sx = tx * kRasterTile + (threadIdx.x & (kRasterTile - 1)), sy = ty * kRasterTile + (threadIdx.x / kRasterTile);
    const int px = sx * kSub + kSub / 2, py = sy * kSub + kSub / 2;
    const long long b = max(0LL, seg[tile]), e = min(n_pairs, seg[tile + 1]);
    float best = -INFINITY;
    int bf = -1;
    unsigned cnt = 0;
    for (long long c0 = b; c0 < e; c0 += kRasterChunk) {
        const int n = int(min((long long)kRasterChunk, e - c0));
        __syncthreads();                                       // the previous chunk has been read by every lane
        if (int(threadIdx.x) < n) {
            const int k = threadIdx.x, f = seg_tri[c0 + k];
            ScreenTri t;
            int face = -1;
            if (f >= 0 && f < F && load_screen_tri(xy, inv_w, V, faces, f, t) == TRI_OK) {
                const Edge e01 = make_edge(t.x0, t.y0, t.x1, t.y1), e12 = make_edge(t.x1, t.y1, t.x2, t.y2),
                           e20 = make_edge(t.x2, t.y2, t.x0, t.y0);
                sAB[k][0] = e12.A; sAB[k][1] = e12.B; sAB[k][2] = e20.A; sAB[k][3] = e20.B; sAB[k][4] = e01.A; sAB[k][5] = e01.B;
                sC[k][0] = e12.C; sC[k][1] = e20.C; sC[k][2] = e01.C;
                sW[k][0] = t.iw0; sW[k][1] = t.iw1; sW[k][2] = t.iw2; sW[k][3] = float(t.area2);
                sMeta[k][1] = e12.tl | (e20.tl << 1) | (e01.tl << 2);
                face = f;
            }
            sMeta[k][0] = face;
        }
        __syncthreads();
        for (int k = 0; k < n; ++k) {
            const int f = sMeta[k][0];
            if (f < 0) continue;
            const int tl = sMeta[k][1];
            const long long E12 = edge_at(sAB[k][0], sAB[k][1], sC[k][0], px, py);
            const long long E20 = edge_at(sAB[k][2], sAB[k][3], sC[k][1], px, py);
            const long long E01 = edge_at(sAB[k][4], sAB[k][5], sC[k][2], px, py);
            if (edge_inside(E12, tl & 1) && edge_inside(E20, (tl >> 1) & 1) && edge_inside(E01, (tl >> 2) & 1)) {
                ++cnt;
                const float z = depth_at(E12, E20, E01, sW[k][0], sW[k][1], sW[k][2], sW[k][3]);
                if (z > best || (z == best && f < bf)) { best = z; bf = f; }
            }
        }
    }
    if (sx < ws && sy < hs) {
        const long long o = (long long)sy * ws + sx;
        face_id[o] = bf;
        depth[o] = bf >= 0 ? best : 0.0f;
        count[o] = (unsigned char)min(cnt, 255u);
    }
}

// ------------------------------------------------------------------ shade and resolve: thread = pixel, its ss x ss samples in row
// order.  Per covered sample: the edge values again (exact), b_k = E_k iw_k / sum — the perspective-correct barycentrics —, the
// base colour (vertex colours, or the material's image at the interpolated uv, or its Kd, or white), times ambient + diffuse *
// max(0, n . light) with n the flat normal turned towards the camera.  Which side faces the camera is the sign of the integer
// screen area (times the handedness of the matrix, front_sign), so it is decided exactly.
// The shared pieces (barycentrics, bilinear lookup, base colour, face normal) are in s3d_render_dev.h.
__global__ void __launch_bounds__(kRenderThreads) k_render_shade(ShadeArgs a) {
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= (long long)a.W * a.H) return;
    const int ix = int(p % a.W), iy = int(p / a.W);
    float acc[3] = {0.0f, 0.0f, 0.0f};
    int covered = 0;
    for (int j = 0; j < a.ss; ++j)
        for (int i = 0; i < a.ss; ++i) {
            const int sx = ix * a.ss + i, sy = iy * a.ss + j;
            const int f = a.face_id[(long long)sy * a.ws + sx];
            ScreenTri t;
            if (f < 0 || f >= a.F || load_screen_tri(a.xy, a.inv_w, a.V, a.faces, f, t) != TRI_OK) continue;
            float b0, b1, b2, c[3] = {1.0f, 1.0f, 1.0f}, n[3];
            sample_barycentrics(t, sx, sy, b0, b1, b2);
            base_colour(a, t, f, b0, b1, b2, c);
            // the flat normal of the face in its own vertex order, towards the camera
            bool front;
            face_normal(a.verts, t, a.front_sign, n, front);
            const float nx = n[0], ny = n[1], nz = n[2];
            const float len = sqrtf(nx * nx + ny * ny + nz * nz);
            float lambert = 0.0f;
            if (len > 0.0f) {
                const float d = __fdiv_rn(nx * a.light[0] + ny * a.light[1] + nz * a.light[2], len);
                lambert = fmaxf(front ? d : -d, 0.0f);
            }
            const float shade = S3D_RENDER_AMBIENT + S3D_RENDER_DIFFUSE * lambert;
#pragma unroll
            for (int k = 0; k < 3; ++k) acc[k] += fminf(fmaxf(c[k] * shade, 0.0f), 1.0f);
            ++covered;
        }
    unsigned char out[4] = {0, 0, 0, 0};
    if (covered) {
#pragma unroll
        for (int k = 0; k < 3; ++k) out[k] = (unsigned char)int(__fdiv_rn(acc[k], float(covered)) * 255.0f + 0.5f);
        out[3] = (unsigned char)int(__fdiv_rn(float(covered), float(a.ss * a.ss)) * 255.0f + 0.5f);
    }
    a.rgba[p * 4] = out[0]; a.rgba[p * 4 + 1] = out[1]; a.rgba[p * 4 + 2] = out[2]; a.rgba[p * 4 + 3] = out[3];
}

static inline int tiles_of(int n) { return (n + kRasterTile - 1) / kRasterTile; }

}  // namespace s3d

using namespace s3d;

extern "C" {

int s3d_render_project(const float* verts, int64_t n_verts, const float view_proj[16], int ws, int hs, float near, int32_t* xy_fixed,
                       float* inv_w, void* stream) {
    S3D_TRY(check_grid_size("render_project", ws, hs));
    S3D_CHECK(view_proj, S3D_ERR_INVALID, "render_project: null matrix");
    for (int k = 0; k < 16; ++k) S3D_CHECK(std::isfinite(view_proj[k]), S3D_ERR_INVALID, "render_project: matrix entry %d is not finite", k);
    S3D_CHECK(near > 0.0f && std::isfinite(near), S3D_ERR_INVALID, "render_project: near %g (must be positive)", double(near));
    S3D_CHECK(n_verts >= 0 && n_verts <= INT32_MAX && (n_verts == 0 || (verts && xy_fixed && inv_w)), S3D_ERR_INVALID,
              "render_project: %lld vertices or a null argument", (long long)n_verts);
    if (!n_verts) return 0;
    ViewProj vp;
    for (int k = 0; k < 16; ++k) vp.m[k] = view_proj[k];
    hipLaunchKernelGGL(k_render_project, dim3(render_blocks(n_verts)), dim3(kRenderThreads), 0, static_cast<hipStream_t>(stream), verts,
                       (long long)n_verts, vp, float(ws), float(hs), near, xy_fixed, inv_w);
    S3D_HIP(hipGetLastError());
    return 0;
}

int s3d_render_bin_count(const int32_t* xy_fixed, const float* inv_w, int64_t n_verts, const int32_t* faces, int64_t n_faces, int ws, int hs,
                         int64_t* counts, uint8_t* status, void* stream) {
    S3D_TRY(check_grid_size("render_bin_count", ws, hs));
    S3D_TRY(check_mesh("render_bin_count", xy_fixed, inv_w, n_verts, faces, n_faces));
    S3D_CHECK(n_faces == 0 || (counts && status), S3D_ERR_INVALID, "render_bin_count: null output");
    if (!n_faces) return 0;
    hipLaunchKernelGGL(k_render_bin_count, dim3(render_blocks(n_faces)), dim3(kRenderThreads), 0, static_cast<hipStream_t>(stream), xy_fixed, inv_w,
                       (long long)n_verts, faces, (long long)n_faces, ws, hs, reinterpret_cast<long long*>(counts), status);
    S3D_HIP(hipGetLastError());
    return 0;
}

int s3d_render_bin_fill(const int32_t* xy_fixed, const float* inv_w, int64_t n_verts, const int32_t* faces, int64_t n_faces, int ws, int hs,
                        const int64_t* offsets, int64_t n_pairs, int32_t* pair_tile, int32_t* pair_tri, void* stream) {
    S3D_TRY(check_grid_size("render_bin_fill", ws, hs));
    S3D_TRY(check_mesh("render_bin_fill", xy_fixed, inv_w, n_verts, faces, n_faces));
    S3D_CHECK(n_pairs >= 0, S3D_ERR_INVALID, "render_bin_fill: %lld pairs", (long long)n_pairs);
    S3D_CHECK(n_pairs <= S3D_RENDER_MAX_PAIRS, S3D_ERR_UNSUPPORTED,
              "render_bin_fill: %lld (tile, triangle) pairs need %.2f GiB of workspace (8 bytes a pair), more than the cap of %lld pairs = 1 GiB: "
              "the mesh has too many large triangles for this sample grid",
              (long long)n_pairs, double(n_pairs) * 8.0 / double(1 << 30), (long long)S3D_RENDER_MAX_PAIRS);
    S3D_CHECK(n_faces == 0 || n_pairs == 0 || (offsets && pair_tile && pair_tri), S3D_ERR_INVALID, "render_bin_fill: null argument");
    if (!n_faces || !n_pairs) return 0;
    hipLaunchKernelGGL(k_render_bin_fill, dim3(render_blocks(n_faces)), dim3(kRenderThreads), 0, static_cast<hipStream_t>(stream), xy_fixed, inv_w,
                       (long long)n_verts, faces, (long long)n_faces, ws, hs, tiles_of(ws), reinterpret_cast<const long long*>(offsets),
                       (long long)n_pairs, pair_tile, pair_tri);
    S3D_HIP(hipGetLastError());
    return 0;
}

int s3d_render_raster(const int32_t* xy_fixed, const float* inv_w, int64_t n_verts, const int32_t* faces, int64_t n_faces, int ws, int hs,
                      const int64_t* seg, const int32_t* seg_tri, int64_t n_pairs, int32_t* face_id, float* depth, uint8_t* count, void* stream) {
    S3D_TRY(check_grid_size("render_raster", ws, hs));
    S3D_TRY(check_mesh("render_raster", xy_fixed, inv_w, n_verts, faces, n_faces));
    S3D_CHECK(n_pairs >= 0 && n_pairs <= S3D_RENDER_MAX_PAIRS, S3D_ERR_INVALID, "render_raster: %lld pairs", (long long)n_pairs);
    S3D_CHECK(seg && face_id && depth && count && (n_pairs == 0 || seg_tri), S3D_ERR_INVALID, "render_raster: null argument");
    hipLaunchKernelGGL(k_render_raster, dim3(unsigned(tiles_of(ws) * tiles_of(hs))), dim3(kRenderThreads), 0, static_cast<hipStream_t>(stream), xy_fixed,
                       inv_w, (long long)n_verts, faces, (long long)n_faces, ws, hs, tiles_of(ws), reinterpret_cast<const long long*>(seg), seg_tri,
                       (long long)n_pairs, face_id, depth, count);
    S3D_HIP(hipGetLastError());
    return 0;
}

int s3d_render_shade(const float* verts, const int32_t* xy_fixed, const float* inv_w, int64_t n_verts, const int32_t* faces, int64_t n_faces,
                     const int32_t* face_id, int ws, int hs, int supersample, const float view_proj[16], const float light[3],
                     const float* vertex_colors, const float* uv, const int32_t* face_mat, const int64_t* mat_table, const float* mat_kd,
                     int n_mats, const uint8_t* images, int64_t image_bytes, uint8_t* rgba, void* stream) {
    ShadeArgs a;
    S3D_TRY(pack_shade_args("render_shade", verts, xy_fixed, inv_w, n_verts, faces, n_faces, face_id, ws, hs, supersample, view_proj, light,
                            vertex_colors, uv, face_mat, mat_table, mat_kd, n_mats, images, image_bytes, rgba, a));
    hipLaunchKernelGGL(k_render_shade, dim3(render_blocks((long long)a.W * a.H)), dim3(kRenderThreads), 0, static_cast<hipStream_t>(stream), a);
    S3D_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
