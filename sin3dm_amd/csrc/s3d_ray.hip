// s3d_ray.hip — any-hit ray queries against a triangle mesh through the uniform cell grid of s3d_meshsdf.hip, and the shadows of
// the PBR renders built on them: s3d_mesh_ray_occluded (one thread per ray), s3d_pbr_shadow_mask (one thread
// per sample of a view: one shadow ray per light that the sample's face is turned to) and s3d_pbr_shade_lit (the shade kernel of
// s3d_render_pbr.hip, skipping the lights the mask switches off).
//
// The ray-triangle test (Moeller-Trumbore) is a pure function of the ray, the triangle's nine floats a, b, c and [t_min, t_max],
// in fp32 WITHOUT contraction (no product is fused into a sum), in this order:
//     e1 = b - a,  e2 = c - a,  p = d x e2,  s = o - a,  q = s x e1        (x x y = (x1 y2 - x2 y1, x2 y0 - x0 y2, x0 y1 - x1 y0))
//     det = (e1.p),  u = (s.p),  v = (d.q),  w = (e2.q)                    (x . y = (x0 y0 + x1 y1) + x2 y2)
//     det < 0: det, u, v, w change sign
//     hit = det > 0 and u >= 0 and v >= 0 and u + v <= det and t_min <= w / det <= t_max
// Edges are inclusive, det == 0 (a zero-area triangle, a ray in the triangle's plane) is a miss, a value that is not finite is a
// miss.  The test is never clipped to the cell being visited, and the query returns at the first hit: so `hit` does not depend on
// the grid, on the order of a cell's list or on a triangle standing in several cells — as long as the walk visits a cell that
// lists the triangle, which the slack of the binning guarantees.  Not watertight: a ray through a shared edge may
// miss both neighbours (u, v and det of the two triangles are rounded separately).
//
// The walk is a 3-D DDA from the ray's entry into the grid box (or t_min) to its exit (or t_max).  Every border crossing is
// computed from the border's index, (origin + i * cell - o) / d, never accumulated; an axis with d == 0 has its crossing at
// +infinity and is never stepped.  The loop runs on an integer counter bounded by nx + ny + nz + 1 cells whatever the floats say,
// every cell index is clamped into the grid, every list bound into [0, n_pairs] and every triangle index is checked against
// n_faces: no input makes the kernels spin or read out of bounds.
#include "s3d_cellgrid.h"
#include "s3d_pbr_shade.h"

namespace s3d {

constexpr int kRayThreads = 256;
static inline unsigned ray_blocks(long long n) { return (unsigned)((n + kRayThreads - 1) / kRayThreads); }

struct RayMesh { const float* tri9; long long F; CellGrid g; const long long* seg; const int* seg_tri; long long n_pairs; };

__device__ __forceinline__ bool ray_hits_triangle(float ox, float oy, float oz, float dx, float dy, float dz, const float* __restrict__ t,
                                                  float t_min, float t_max) {
#pragma clang fp contract(off)
    const float e1x = t[3] - t[0], e1y = t[4] - t[1], e1z = t[5] - t[2];
    const float e2x = t[6] - t[0], e2y = t[7] - t[1], e2z = t[8] - t[2];
    const float px = dy * e2z - dz * e2y, py = dz * e2x - dx * e2z, pz = dx * e2y - dy * e2x;
    const float sx = ox - t[0], sy = oy - t[1], sz = oz - t[2];
    const float qx = sy * e1z - sz * e1y, qy = sz * e1x - sx * e1z, qz = sx * e1y - sy * e1x;
    float det = (e1x * px + e1y * py) + e1z * pz;
    float u = (sx * px + sy * py) + sz * pz;
    float v = (dx * qx + dy * qy) + dz * qz;
    float w = (e2x * qx + e2y * qy) + e2z * qz;
    if (det < 0.0f) { det = -det; u = -u; v = -v; w = -w; }
    if (!(det > 0.0f && u >= 0.0f && v >= 0.0f && u + v <= det)) return false;      // (a NaN compares false)
    const float tt = __fdiv_rn(w, det);
    return tt >= t_min && tt <= t_max;
}

// the parameter at which the ray crosses the border of index i along one axis
__device__ __forceinline__ float border_t(int i, float go, float cell, float o, float d) {
#pragma clang fp contract(off)
    return __fdiv_rn((go + float(i) * cell) - o, d);
}

// 1 when some triangle other than `skip` is crossed at a parameter in [t_min, t_max].  status: 0 walked, 1 the ray never enters the
// grid box within [t_min, t_max], 2 an origin or direction that is not finite or a zero direction.
__device__ __forceinline__ int mesh_ray_occluded(const RayMesh& m, float ox, float oy, float oz, float dx, float dy, float dz, int skip,
                                                 float t_min, float t_max, int& status) {
#pragma clang fp contract(off)
    const CellGrid& g = m.g;
    const bool finite = fabsf(ox) < INFINITY && fabsf(oy) < INFINITY && fabsf(oz) < INFINITY && fabsf(dx) < INFINITY && fabsf(dy) < INFINITY &&
                        fabsf(dz) < INFINITY;                                         // (a NaN compares false)
    if (!finite || (dx == 0.0f && dy == 0.0f && dz == 0.0f)) { status = 2; return 0; }
    // ---- the ray against the grid box, slab by slab; an axis the ray does not move along only decides inside / outside
    float t0 = t_min, t1 = t_max;
    bool outside = false;
    {
        const float hx = g.ox + float(g.nx) * g.cell, hy = g.oy + float(g.ny) * g.cell, hz = g.oz + float(g.nz) * g.cell;
        if (dx == 0.0f) outside = outside || !(ox >= g.ox && ox <= hx);
        else { const float a = __fdiv_rn(g.ox - ox, dx), b = __fdiv_rn(hx - ox, dx); t0 = fmaxf(t0, fminf(a, b)); t1 = fminf(t1, fmaxf(a, b)); }
        if (dy == 0.0f) outside = outside || !(oy >= g.oy && oy <= hy);
        else { const float a = __fdiv_rn(g.oy - oy, dy), b = __fdiv_rn(hy - oy, dy); t0 = fmaxf(t0, fminf(a, b)); t1 = fminf(t1, fmaxf(a, b)); }
        if (dz == 0.0f) outside = outside || !(oz >= g.oz && oz <= hz);
        else { const float a = __fdiv_rn(g.oz - oz, dz), b = __fdiv_rn(hz - oz, dz); t0 = fmaxf(t0, fminf(a, b)); t1 = fminf(t1, fmaxf(a, b)); }
    }
    if (outside || !(t0 <= t1)) { status = 1; return 0; }
    status = 0;
    // ---- the cell of the entry point (clamped), the direction of the steps and the next crossing per axis
    int ix = cell_of(ox + t0 * dx, g.ox, g.cell, g.nx), iy = cell_of(oy + t0 * dy, g.oy, g.cell, g.ny), iz = cell_of(oz + t0 * dz, g.oz, g.cell, g.nz);
    const int stx = dx > 0.0f ? 1 : (dx < 0.0f ? -1 : 0), sty = dy > 0.0f ? 1 : (dy < 0.0f ? -1 : 0), stz = dz > 0.0f ? 1 : (dz < 0.0f ? -1 : 0);
    float tx = stx ? border_t(ix + (stx > 0 ? 1 : 0), g.ox, g.cell, ox, dx) : INFINITY;
    float ty = sty ? border_t(iy + (sty > 0 ? 1 : 0), g.oy, g.cell, oy, dy) : INFINITY;
    float tz = stz ? border_t(iz + (stz > 0 ? 1 : 0), g.oz, g.cell, oz, dz) : INFINITY;
    const int max_cells = g.nx + g.ny + g.nz + 1;
    for (int n = 0; n < max_cells; ++n) {
        const long long c = ((long long)ix * g.ny + iy) * g.nz + iz;
        const long long b = max(0LL, m.seg[c]), e = min(m.n_pairs, m.seg[c + 1]);
        for (long long j = b; j < e; ++j) {
            const int f = m.seg_tri[j];
            if (f < 0 || f >= m.F || f == skip) continue;
            if (ray_hits_triangle(ox, oy, oz, dx, dy, dz, m.tri9 + (long long)f * 9, t_min, t_max)) return 1;
        }
        // the nearest crossing (equal: x before y before z); past the end of the ray, or out of the grid: done
        if (tx <= ty && tx <= tz) {
            if (!(tx <= t1)) break;
            ix += stx;
            if (ix < 0 || ix >= g.nx) break;
            tx = border_t(ix + (stx > 0 ? 1 : 0), g.ox, g.cell, ox, dx);
        } else if (ty <= tz) {
            if (!(ty <= t1)) break;
            iy += sty;
            if (iy < 0 || iy >= g.ny) break;
            ty = border_t(iy + (sty > 0 ? 1 : 0), g.oy, g.cell, oy, dy);
        } else {
            if (!(tz <= t1) || stz == 0) break;                                       // (stz == 0 here: tz = +inf, and so are the others)
            iz += stz;
            if (iz < 0 || iz >= g.nz) break;
            tz = border_t(iz + (stz > 0 ? 1 : 0), g.oz, g.cell, oz, dz);
        }
    }
    return 0;
}

// ------------------------------------------------------------------ rays given as arrays: thread = ray
__global__ void __launch_bounds__(kRayThreads) k_mesh_ray_occluded(const float* __restrict__ origins, const float* __restrict__ dirs,
                                                                   const int* __restrict__ skip_face, long long N, float t_min, float t_max,
                                                                   RayMesh m, unsigned char* __restrict__ hit, unsigned char* __restrict__ status) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    int st;
    const int h = mesh_ray_occluded(m, origins[i * 3], origins[i * 3 + 1], origins[i * 3 + 2], dirs[i * 3], dirs[i * 3 + 1], dirs[i * 3 + 2],
                                    skip_face ? skip_face[i] : -1, t_min, t_max, st);
    hit[i] = (unsigned char)h;
    status[i] = (unsigned char)st;
}

// ------------------------------------------------------------------ the shadow mask of a view: thread = sample.  The point is the one
// k_render_shade_pbr takes its view vector from, b0 P0 + b1 P1 + b2 P2 with the sample's perspective-correct barycentrics; the
// normal is the face's own (not normalised: only its sign against the light is used), turned to the camera by face_normal's
// integer rule.  A light the face is turned away from gets bit 0 without a ray; the others send one ray from the point towards the
// light that skips the sample's own face and starts at t_min.
struct ShadowArgs {
    const float* verts; const int* xy; const float* inv_w; long long V;
    const int* faces; long long F;
    const int* face_id; int ws, hs;
    int front_sign, n_lights;
    float t_min;
    float lights[kMaxLights][4];
    RayMesh m;
    unsigned char* lit;
};

__global__ void __launch_bounds__(kRayThreads) k_render_shadow_mask(ShadowArgs a) {
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= (long long)a.ws * a.hs) return;
    const int sx = int(p % a.ws), sy = int(p / a.ws);
    const int f = a.face_id[p];
    ScreenTri t;
    unsigned out = 0;
    if (f >= 0 && f < a.F && load_screen_tri(a.xy, a.inv_w, a.V, a.faces, f, t) == TRI_OK) {
        float b0, b1, b2;
        sample_barycentrics(t, sx, sy, b0, b1, b2);
        float N[3];
        bool front;
        face_normal(a.verts, t, a.front_sign, N, front);
        if (!front) { N[0] = -N[0]; N[1] = -N[1]; N[2] = -N[2]; }
        const float* P0 = a.verts + t.v0 * 3LL;
        const float* P1 = a.verts + t.v1 * 3LL;
        const float* P2 = a.verts + t.v2 * 3LL;
        float P[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) P[k] = b0 * P0[k] + b1 * P1[k] + b2 * P2[k];
#pragma unroll 1
        for (int li = 0; li < a.n_lights; ++li) {               // (rolled: the lights stay in the argument block, not in registers)
            if (li < kMaxLights) {
                const float L[3] = {a.lights[li][0], a.lights[li][1], a.lights[li][2]};
                if (!(dot3(N, L) > 0.0f)) continue;
                int st;
                if (!mesh_ray_occluded(a.m, P[0], P[1], P[2], L[0], L[1], L[2], f, a.t_min, INFINITY, st)) out |= 1u << li;
            }
        }
    }
    a.lit[p] = (unsigned char)out;
}

// ------------------------------------------------------------------ shade and resolve with the mask: s3d_pbr_shade_body.h with LIT
__global__ void __launch_bounds__(kPbrThreads) k_render_shade_pbr_lit(PbrArgs a, const unsigned char* __restrict__ lit) {
    constexpr bool LIT = true;
#include "s3d_pbr_shade_body.h"
}

// the grid and the segment lists of an entry point
static int pack_ray_mesh(const char* who, const float* tri9, int64_t n_faces, const float origin[3], float cell, const int dims[3],
                         const int64_t* seg, const int32_t* seg_tri, int64_t n_pairs, RayMesh& m) {
    S3D_CHECK(origin && dims, S3D_ERR_INVALID, "%s: null grid argument", who);
    S3D_CHECK(cell > 0.0f && std::isfinite(cell) && std::isfinite(origin[0]) && std::isfinite(origin[1]) && std::isfinite(origin[2]), S3D_ERR_INVALID,
              "%s: cell edge %g or an origin that is not finite", who, double(cell));
    S3D_CHECK(dims[0] >= 1 && dims[1] >= 1 && dims[2] >= 1 && (long long)dims[0] * dims[1] * (long long)dims[2] <= S3D_MESHSDF_MAX_CELLS,
              S3D_ERR_INVALID, "%s: cell grid %d x %d x %d (1 a side at least, at most %lld cells)", who, dims[0], dims[1], dims[2],
              (long long)S3D_MESHSDF_MAX_CELLS);
    S3D_CHECK(n_faces >= 0 && n_faces <= INT32_MAX && n_pairs >= 0 && n_pairs <= S3D_MESHSDF_MAX_PAIRS, S3D_ERR_INVALID, "%s: %lld faces, %lld pairs", who,
              (long long)n_faces, (long long)n_pairs);
    S3D_CHECK(seg && (n_pairs == 0 || (seg_tri && tri9)), S3D_ERR_INVALID, "%s: null segment list or triangles", who);
    m.tri9 = tri9; m.F = n_faces; m.g = CellGrid{origin[0], origin[1], origin[2], cell, dims[0], dims[1], dims[2]};
    m.seg = reinterpret_cast<const long long*>(seg); m.seg_tri = seg_tri; m.n_pairs = n_pairs;
    return 0;
}

}  // namespace s3d

using namespace s3d;

extern "C" {

int s3d_mesh_ray_occluded(const float* origins, const float* dirs, const int32_t* skip_face, int64_t n_rays, float t_min, float t_max,
                          const float* tri9, int64_t n_faces, const float origin[3], float cell, const int dims[3], const int64_t* seg,
                          const int32_t* seg_tri, int64_t n_pairs, uint8_t* hit, uint8_t* status, void* stream) {
    RayMesh m;
    S3D_TRY(pack_ray_mesh("mesh_ray_occluded", tri9, n_faces, origin, cell, dims, seg, seg_tri, n_pairs, m));
    S3D_CHECK(n_rays >= 0, S3D_ERR_INVALID, "mesh_ray_occluded: %lld rays", (long long)n_rays);
    S3D_CHECK(t_min >= 0.0f && std::isfinite(t_min) && t_max >= t_min, S3D_ERR_INVALID,
              "mesh_ray_occluded: t_min %g (finite, not negative), t_max %g (not below t_min; +inf allowed)", double(t_min), double(t_max));
    S3D_CHECK(hit && status, S3D_ERR_INVALID, "mesh_ray_occluded: null output");
    S3D_CHECK(n_rays == 0 || (origins && dirs), S3D_ERR_INVALID, "mesh_ray_occluded: null rays");
    if (!n_rays) return 0;
    hipLaunchKernelGGL(k_mesh_ray_occluded, dim3(ray_blocks(n_rays)), dim3(kRayThreads), 0, static_cast<hipStream_t>(stream), origins, dirs, skip_face,
                       (long long)n_rays, t_min, t_max, m, hit, status);
    S3D_HIP(hipGetLastError());
    return 0;
}

int s3d_pbr_shadow_mask(const float* verts, const int32_t* xy_fixed, const float* inv_w, int64_t n_verts, const int32_t* faces, int64_t n_faces,
                           const int32_t* face_id, int ws, int hs, const float view_proj[16], const float* lights, int n_lights, float t_min,
                           const float* tri9, const float origin[3], float cell, const int dims[3], const int64_t* seg, const int32_t* seg_tri,
                           int64_t n_pairs, uint8_t* lit, void* stream) {
    ShadowArgs a;
    S3D_TRY(check_grid_size("pbr_shadow_mask", ws, hs));
    S3D_TRY(check_mesh("pbr_shadow_mask", xy_fixed, inv_w, n_verts, faces, n_faces));
    S3D_TRY(check_lights("pbr_shadow_mask", lights, n_lights));
    S3D_TRY(pack_ray_mesh("pbr_shadow_mask", tri9, n_faces, origin, cell, dims, seg, seg_tri, n_pairs, a.m));
    S3D_CHECK(t_min >= 0.0f && std::isfinite(t_min), S3D_ERR_INVALID, "pbr_shadow_mask: t_min %g (finite, not negative)", double(t_min));
    S3D_CHECK(lit && face_id && view_proj && (n_verts == 0 || verts) && (n_faces == 0 || tri9), S3D_ERR_INVALID, "pbr_shadow_mask: null argument");
    for (int k = 0; k < 16; ++k) S3D_CHECK(std::isfinite(view_proj[k]), S3D_ERR_INVALID, "pbr_shadow_mask: matrix entry %d is not finite", k);
    a.verts = verts; a.xy = xy_fixed; a.inv_w = inv_w; a.V = n_verts; a.faces = faces; a.F = n_faces; a.face_id = face_id; a.ws = ws; a.hs = hs;
    a.front_sign = matrix_front_sign(view_proj); a.n_lights = n_lights; a.t_min = t_min; a.lit = lit;
    memset(a.lights, 0, sizeof(a.lights));
    for (int k = 0; k < n_lights * 4; ++k) a.lights[k / 4][k % 4] = lights[k];
    hipLaunchKernelGGL(k_render_shadow_mask, dim3(ray_blocks((long long)ws * hs)), dim3(kRayThreads), 0, static_cast<hipStream_t>(stream), a);
    S3D_HIP(hipGetLastError());
    return 0;
}

int s3d_pbr_shade_lit(const float* verts, const int32_t* xy_fixed, const float* inv_w, int64_t n_verts, const int32_t* faces, int64_t n_faces,
                      const int32_t* face_id, int ws, int hs, int supersample, const float view_proj[16], const float* vertex_colors,
                      const float* uv, const int32_t* face_mat, const int64_t* mat_table, const float* mat_kd, int n_mats, const uint8_t* images,
                      int64_t image_bytes, const float* normals, const float* tangents, const int64_t* pbr_table, const float* pbr_factors,
                      const float eye[3], const float* lights, int n_lights, float ambient, int pass, const uint8_t* lit, uint8_t* rgba,
                      void* stream) {
    if (!lit)                                                     // no mask: s3d_pbr_shade itself, its kernel and its bits
        return s3d_pbr_shade(verts, xy_fixed, inv_w, n_verts, faces, n_faces, face_id, ws, hs, supersample, view_proj, vertex_colors, uv, face_mat,
                             mat_table, mat_kd, n_mats, images, image_bytes, normals, tangents, pbr_table, pbr_factors, eye, lights, n_lights, ambient,
                             pass, rgba, stream);
    PbrArgs a;
    S3D_TRY(pack_pbr_args("pbr_shade_lit", verts, xy_fixed, inv_w, n_verts, faces, n_faces, face_id, ws, hs, supersample, view_proj, vertex_colors, uv,
                          face_mat, mat_table, mat_kd, n_mats, images, image_bytes, normals, tangents, pbr_table, pbr_factors, eye, lights, n_lights,
                          ambient, pass, rgba, a));
    hipLaunchKernelGGL(k_render_shade_pbr_lit, dim3(pbr_blocks((long long)a.s.W * a.s.H)), dim3(kPbrThreads), 0, static_cast<hipStream_t>(stream), a,
                       lit);
    S3D_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
