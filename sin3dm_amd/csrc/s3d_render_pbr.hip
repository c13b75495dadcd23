// s3d_render_pbr.hip — PBR renders of triangle meshes: area-weighted vertex normals, per-face tangents of the uv
// map, and a shade-and-resolve kernel with smooth normals, normal maps, a GGX / Schlick / Smith-Schlick light model under up to
// four directional lights, and the material passes of the reference's rendering/blender_render_pbr.py.  The raster stage is
// s3d_render.hip's; the face on the screen, the barycentrics, the bilinear lookup and the base colour are the shared definitions of
// s3d_render_dev.h.  Every loop bound is known at launch; no atomics; every output element is written by one thread, in one fixed
// order of operations, so the same input gives the same bits.
#include "s3d_render_dev.h"
#include "s3d_pbr_shade.h"

namespace s3d {

// ------------------------------------------------------------------ vertex normals: thread = vertex.  corner_order lists the 3 F
// corners (corner k = vertex k % 3 of face k / 3) sorted by vertex, stably, so ascending; vertex v owns [start[v], start[v + 1]).
// The sum of the unnormalised face normals (area weights) is taken in float64: the kernel waits on its gathers, the few float64
// operations per corner are free, and the sum then carries no rounding of its own — the result is the float32 rounding of the
// exact normalised sum to a few float64 units, whatever the valence.
__global__ void __launch_bounds__(kPbrThreads) k_render_vertex_normals(const float* __restrict__ verts, long long V, const int* __restrict__ faces,
                                                                      long long F, const long long* __restrict__ order,
                                                                      const long long* __restrict__ start, float* __restrict__ normals) {
    const long long v = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= V) return;
    const long long b = max(0LL, start[v]), e = min(3 * F, start[v + 1]);
    double sx = 0.0, sy = 0.0, sz = 0.0;
    for (long long c = b; c < e; ++c) {
        const long long k = order[c];
        if (k < 0 || k >= 3 * F) continue;
        const long long f = k / 3;
        const int ia = faces[f * 3], ib = faces[f * 3 + 1], ic = faces[f * 3 + 2];
        if (ia < 0 || ib < 0 || ic < 0 || ia >= V || ib >= V || ic >= V) continue;
        const float* A = verts + ia * 3LL;
        const float* B = verts + ib * 3LL;
        const float* Cc = verts + ic * 3LL;
        const double ux = double(B[0]) - A[0], uy = double(B[1]) - A[1], uz = double(B[2]) - A[2];
        const double vx = double(Cc[0]) - A[0], vy = double(Cc[1]) - A[1], vz = double(Cc[2]) - A[2];
        sx += uy * vz - uz * vy; sy += uz * vx - ux * vz; sz += ux * vy - uy * vx;
    }
    const double l2 = sx * sx + sy * sy + sz * sz;
    float nx = 0.0f, ny = 0.0f, nz = 0.0f;
    if (l2 > 0.0 && l2 < INFINITY) {                                             // (a NaN compares false)
        const double l = sqrt(l2);
        nx = float(sx / l); ny = float(sy / l); nz = float(sz / l);
    }
    normals[v * 3] = nx; normals[v * 3 + 1] = ny; normals[v * 3 + 2] = nz;
}

// ------------------------------------------------------------------ face tangents: thread = face.  T = d position / d u and
// B = d position / d v of the face's uv map (v as in the lookups: the GL convention), in float64 for the same reason as above:
// det = du1 dv2 - du2 dv1 cancels, and the float64 form costs nothing here.  det == 0, a bad index or a result that is not finite:
// T = B = 0, "no tangent".
__global__ void __launch_bounds__(kPbrThreads) k_render_face_tangents(const float* __restrict__ verts, long long V, const int* __restrict__ faces,
                                                                     long long F, const float* __restrict__ uv, float* __restrict__ tangents) {
    const long long f = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= F) return;
    float out[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    const int ia = faces[f * 3], ib = faces[f * 3 + 1], ic = faces[f * 3 + 2];
    if (ia >= 0 && ib >= 0 && ic >= 0 && ia < V && ib < V && ic < V) {
        const float* A = verts + ia * 3LL;
        const float* B = verts + ib * 3LL;
        const float* Cc = verts + ic * 3LL;
        const float* q = uv + f * 6;
        const double du1 = double(q[2]) - q[0], dv1 = double(q[3]) - q[1], du2 = double(q[4]) - q[0], dv2 = double(q[5]) - q[1];
        const double det = du1 * dv2 - du2 * dv1;
        if (det != 0.0) {
            bool ok = true;
            float r[6];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const double e1 = double(B[k]) - A[k], e2 = double(Cc[k]) - A[k];
                r[k] = float((e1 * dv2 - e2 * dv1) / det);
                r[3 + k] = float((e2 * du1 - e1 * du2) / det);
                ok = ok && fabsf(r[k]) < INFINITY && fabsf(r[3 + k]) < INFINITY;   // (a NaN compares false)
            }
            if (ok) {
#pragma unroll
                for (int k = 0; k < 6; ++k) out[k] = r[k];
            }
        }
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) tangents[f * 6 + k] = out[k];
}

// ------------------------------------------------------------------ shade and resolve with the PBR light model: the argument block and
// the helpers are s3d_pbr_shade.h's, the body is s3d_pbr_shade_body.h (shared with k_render_shade_pbr_lit of s3d_ray.hip)
__global__ void __launch_bounds__(kPbrThreads) k_render_shade_pbr(PbrArgs a) {
    constexpr bool LIT = false;
    const unsigned char* const lit = nullptr;
#include "s3d_pbr_shade_body.h"
}

}  // namespace s3d

using namespace s3d;

extern "C" {

int s3d_pbr_vertex_normals(const float* verts, int64_t n_verts, const int32_t* faces, int64_t n_faces, const int64_t* corner_order,
                              const int64_t* vertex_start, float* normals, void* stream) {
    S3D_CHECK(n_verts >= 0 && n_verts <= INT32_MAX && n_faces >= 0 && n_faces <= INT32_MAX, S3D_ERR_INVALID,
              "pbr_vertex_normals: %lld vertices, %lld faces", (long long)n_verts, (long long)n_faces);
    S3D_CHECK(n_verts == 0 || (verts && vertex_start && normals), S3D_ERR_INVALID, "pbr_vertex_normals: null vertex argument");
    S3D_CHECK(n_faces == 0 || (faces && corner_order), S3D_ERR_INVALID, "pbr_vertex_normals: null face table or corner order");
    if (!n_verts) return 0;
    hipLaunchKernelGGL(k_render_vertex_normals, dim3(pbr_blocks(n_verts)), dim3(kPbrThreads), 0, static_cast<hipStream_t>(stream), verts,
                       (long long)n_verts, faces, (long long)n_faces, reinterpret_cast<const long long*>(corner_order),
                       reinterpret_cast<const long long*>(vertex_start), normals);
    S3D_HIP(hipGetLastError());
    return 0;
}

int s3d_pbr_face_tangents(const float* verts, int64_t n_verts, const int32_t* faces, int64_t n_faces, const float* uv, float* tangents,
                             void* stream) {
    S3D_CHECK(n_verts >= 0 && n_verts <= INT32_MAX && n_faces >= 0 && n_faces <= INT32_MAX, S3D_ERR_INVALID,
              "pbr_face_tangents: %lld vertices, %lld faces", (long long)n_verts, (long long)n_faces);
    S3D_CHECK(n_faces == 0 || (faces && uv && tangents && (n_verts == 0 || verts)), S3D_ERR_INVALID, "pbr_face_tangents: null argument");
    if (!n_faces) return 0;
    hipLaunchKernelGGL(k_render_face_tangents, dim3(pbr_blocks(n_faces)), dim3(kPbrThreads), 0, static_cast<hipStream_t>(stream), verts,
                       (long long)n_verts, faces, (long long)n_faces, uv, tangents);
    S3D_HIP(hipGetLastError());
    return 0;
}

int s3d_pbr_shade(const float* verts, const int32_t* xy_fixed, const float* inv_w, int64_t n_verts, const int32_t* faces,
                         int64_t n_faces, const int32_t* face_id, int ws, int hs, int supersample, const float view_proj[16],
                         const float* vertex_colors, const float* uv, const int32_t* face_mat, const int64_t* mat_table, const float* mat_kd,
                         int n_mats, const uint8_t* images, int64_t image_bytes, const float* normals, const float* tangents,
                         const int64_t* pbr_table, const float* pbr_factors, const float eye[3], const float* lights, int n_lights,
                         float ambient, int pass, uint8_t* rgba, void* stream) {
    PbrArgs a;
    S3D_TRY(pack_pbr_args("pbr_shade", verts, xy_fixed, inv_w, n_verts, faces, n_faces, face_id, ws, hs, supersample, view_proj, vertex_colors, uv,
                          face_mat, mat_table, mat_kd, n_mats, images, image_bytes, normals, tangents, pbr_table, pbr_factors, eye, lights, n_lights,
                          ambient, pass, rgba, a));
    hipLaunchKernelGGL(k_render_shade_pbr, dim3(pbr_blocks((long long)a.s.W * a.s.H)), dim3(kPbrThreads), 0, static_cast<hipStream_t>(stream), a);
    S3D_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
