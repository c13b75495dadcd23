// s3d_render_pbr.hip — PBR renders of triangle meshes: area-weighted vertex normals, per-face tangents of the uv
// map, and a shade-and-resolve kernel with smooth normals, normal maps, a GGX / Schlick / Smith-Schlick light model under up to
// four directional lights, and the material passes of the reference's rendering/blender_render_pbr.py.  The raster stage is
// s3d_render.hip's; the face on the screen, the barycentrics, the bilinear lookup and the base colour are the shared definitions of
// s3d_render_dev.h.  Every loop bound is known at launch; no atomics; every output element is written by one thread, in one fixed
// order of operations, so the same input gives the same bits.
#include "s3d_render_dev.h"

namespace s3d {

constexpr int kPbrThreads = 256;
constexpr int kMaxLights = S3D_RENDER_MAX_LIGHTS;
constexpr int kMaxPbrMats = S3D_RENDER_PBR_MAX_MATERIALS;
static inline unsigned pbr_blocks(long long n) { return (unsigned)((n + kPbrThreads - 1) / kPbrThreads); }

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

// ------------------------------------------------------------------ shade and resolve with the PBR light model: thread = pixel, its
// ss x ss samples in row order, as k_render_shade.
struct PbrArgs {
    ShadeArgs s;
    const float* normals;                  // [V][3] or null: flat
    const float* tangents;                 // [F][2][3] or null: no normal maps
    int pbr;                               // 1: tab / fac describe the materials; 0: the base colour of k_render_shade, metallic 0, roughness 0.5
    int n_lights, pass;
    float ambient;
    float eye[3];
    float lights[kMaxLights][4];           // unit direction towards the light, intensity
    long long tab[kMaxPbrMats][4][3];      // {byte offset, W, H} of albedo, metallic, roughness, normal; W = 0: absent.  Checked on the host
    float fac[kMaxPbrMats][5];             // Kd r g b, metallic, roughness
};

__device__ __forceinline__ float dot3(const float a[3], const float b[3]) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
// v / |v|; false (v untouched) when the squared length is 0 or not finite
__device__ __forceinline__ bool normalize3(float v[3]) {
    const float l2 = dot3(v, v);
    if (!(l2 > 0.0f && l2 < INFINITY)) return false;
    const float l = sqrtf(l2);
    v[0] = __fdiv_rn(v[0], l); v[1] = __fdiv_rn(v[1], l); v[2] = __fdiv_rn(v[2], l);
    return true;
}
__device__ __forceinline__ void cross3(const float a[3], const float b[3], float c[3]) {
    c[0] = a[1] * b[2] - a[2] * b[1]; c[1] = a[2] * b[0] - a[0] * b[2]; c[2] = a[0] * b[1] - a[1] * b[0];
}

__global__ void __launch_bounds__(kPbrThreads) k_render_shade_pbr(PbrArgs a) {
    const ShadeArgs& s = a.s;
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= (long long)s.W * s.H) return;
    const int ix = int(p % s.W), iy = int(p / s.W);
    const float kPi = 3.14159265358979323846f;
    float acc[3] = {0.0f, 0.0f, 0.0f};
    int covered = 0;
    for (int j = 0; j < s.ss; ++j)
        for (int i = 0; i < s.ss; ++i) {
            const int sx = ix * s.ss + i, sy = iy * s.ss + j;
            const int f = s.face_id[(long long)sy * s.ws + sx];
            ScreenTri t;
            if (f < 0 || f >= s.F || load_screen_tri(s.xy, s.inv_w, s.V, s.faces, f, t) != TRI_OK) continue;
            float b0, b1, b2;
            sample_barycentrics(t, sx, sy, b0, b1, b2);
            // ---- the shading normal: flat, towards the camera by the integer rule
            float N[3];
            bool front;
            face_normal(s.verts, t, s.front_sign, N, front);
            const bool has_flat = normalize3(N);
            if (!has_flat) { N[0] = 0.0f; N[1] = 0.0f; N[2] = 0.0f; }
            if (!front) { N[0] = -N[0]; N[1] = -N[1]; N[2] = -N[2]; }
            if (a.normals && has_flat) {                       // smooth: the mix of the corners' normals, unless it is unusable
                const float* n0 = a.normals + t.v0 * 3LL;
                const float* n1 = a.normals + t.v1 * 3LL;
                const float* n2 = a.normals + t.v2 * 3LL;
                const bool any_zero = (n0[0] == 0.0f && n0[1] == 0.0f && n0[2] == 0.0f) || (n1[0] == 0.0f && n1[1] == 0.0f && n1[2] == 0.0f) ||
                                      (n2[0] == 0.0f && n2[1] == 0.0f && n2[2] == 0.0f);
                float mix[3];
#pragma unroll
                for (int k = 0; k < 3; ++k) mix[k] = b0 * n0[k] + b1 * n1[k] + b2 * n2[k];
                if (!any_zero && normalize3(mix)) {
                    if (!front) { mix[0] = -mix[0]; mix[1] = -mix[1]; mix[2] = -mix[2]; }
                    if (dot3(mix, N) > 0.0f) { N[0] = mix[0]; N[1] = mix[1]; N[2] = mix[2]; }
                }
            }
            // ---- the material
            float albedo[3] = {1.0f, 1.0f, 1.0f}, metal = 0.0f, rough = 0.5f;
            float tu = 0.0f, tv = 0.0f;
            int m = -1;
            if (a.pbr) {
                m = s.face_mat ? s.face_mat[f] : 0;
                if (m < 0 || m >= s.M) m = -1;
                if (s.uv) sample_uv(s.uv, f, t.swapped, b0, b1, b2, tu, tv);
                if (m >= 0) {
                    albedo[0] = a.fac[m][0]; albedo[1] = a.fac[m][1]; albedo[2] = a.fac[m][2];
                    metal = a.fac[m][3]; rough = a.fac[m][4];
                    if (s.uv) {
                        if (a.tab[m][0][1] > 0) tex_bilinear<3>(s.img, a.tab[m][0][0], int(a.tab[m][0][1]), int(a.tab[m][0][2]), tu, tv, albedo);
                        if (a.tab[m][1][1] > 0) tex_bilinear<1>(s.img, a.tab[m][1][0], int(a.tab[m][1][1]), int(a.tab[m][1][2]), tu, tv, &metal);
                        if (a.tab[m][2][1] > 0) tex_bilinear<1>(s.img, a.tab[m][2][0], int(a.tab[m][2][1]), int(a.tab[m][2][2]), tu, tv, &rough);
                    }
                }
            } else {
                base_colour(s, t, f, b0, b1, b2, albedo);
            }
            // ---- the normal map, in the face's tangent frame made orthonormal around N
            if (a.pbr && m >= 0 && a.pass != S3D_RENDER_PASS_GEO && a.tangents && s.uv && has_flat && a.tab[m][3][1] > 0) {
                const float* tg = a.tangents + (long long)f * 6;
                float T[3] = {tg[0], tg[1], tg[2]};
                const float B[3] = {tg[3], tg[4], tg[5]};
                const float nt = dot3(N, T);
#pragma unroll
                for (int k = 0; k < 3; ++k) T[k] = T[k] - N[k] * nt;
                if (normalize3(T)) {
                    float Bp[3], tx[3];
                    cross3(N, T, Bp);
                    const float sg = dot3(Bp, B) < 0.0f ? -1.0f : 1.0f;
                    tex_bilinear<3>(s.img, a.tab[m][3][0], int(a.tab[m][3][1]), int(a.tab[m][3][2]), tu, tv, tx);
#pragma unroll
                    for (int k = 0; k < 3; ++k) tx[k] = 2.0f * tx[k] - 1.0f;
                    float Nm[3];
#pragma unroll
                    for (int k = 0; k < 3; ++k) Nm[k] = tx[0] * T[k] + tx[1] * (sg * Bp[k]) + tx[2] * N[k];
                    if (normalize3(Nm)) { N[0] = Nm[0]; N[1] = Nm[1]; N[2] = Nm[2]; }
                }
            }
            if (a.pass == S3D_RENDER_PASS_GEO) {
                albedo[0] = albedo[1] = albedo[2] = S3D_RENDER_GEO_GREY;
                metal = 0.0f; rough = 0.5f;
            }
            // ---- the value of the pass
            float out[3];
            if (a.pass == S3D_RENDER_PASS_ALBEDO) {
                out[0] = albedo[0]; out[1] = albedo[1]; out[2] = albedo[2];
            } else if (a.pass == S3D_RENDER_PASS_METALLIC) {
                out[0] = out[1] = out[2] = metal;
            } else if (a.pass == S3D_RENDER_PASS_ROUGHNESS) {
                out[0] = out[1] = out[2] = rough;
            } else if (a.pass == S3D_RENDER_PASS_NORMAL) {
#pragma unroll
                for (int k = 0; k < 3; ++k) out[k] = 0.5f * N[k] + 0.5f;
            } else {
                const float r = fminf(fmaxf(rough, S3D_RENDER_MIN_ROUGHNESS), 1.0f);
                const float alpha = r * r, a2 = alpha * alpha, kk = 0.5f * alpha;
                // the point on the face, and the unit vector from it to the eye
                const float* P0 = s.verts + t.v0 * 3LL;
                const float* P1 = s.verts + t.v1 * 3LL;
                const float* P2 = s.verts + t.v2 * 3LL;
                float Vv[3];
#pragma unroll
                for (int k = 0; k < 3; ++k) Vv[k] = a.eye[k] - (b0 * P0[k] + b1 * P1[k] + b2 * P2[k]);
                if (!normalize3(Vv)) { Vv[0] = N[0]; Vv[1] = N[1]; Vv[2] = N[2]; }
                const float NV = fmaxf(dot3(N, Vv), 1e-4f);
                const float gv = __fdiv_rn(NV, NV * (1.0f - kk) + kk);
                float F0[3];
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    F0[k] = 0.04f * (1.0f - metal) + albedo[k] * metal;
                    out[k] = a.ambient * albedo[k];
                }
#pragma unroll 1
                for (int li = 0; li < a.n_lights; ++li) {       // (rolled: the lights stay in the argument block, not in registers)
                    if (li < kMaxLights) {
                        const float L[3] = {a.lights[li][0], a.lights[li][1], a.lights[li][2]};
                        const float NL = fmaxf(dot3(N, L), 0.0f);
                        float Hh[3] = {L[0] + Vv[0], L[1] + Vv[1], L[2] + Vv[2]};
                        if (!normalize3(Hh)) { Hh[0] = N[0]; Hh[1] = N[1]; Hh[2] = N[2]; }
                        const float NH = dot3(N, Hh), VH = fminf(fmaxf(dot3(Vv, Hh), 0.0f), 1.0f);
                        const float x = 1.0f - VH, x2 = x * x, x5 = x2 * x2 * x;
                        const float dd = NH * NH * (a2 - 1.0f) + 1.0f;
                        const float D = __fdiv_rn(a2, kPi * dd * dd);
                        const float G = __fdiv_rn(NL, NL * (1.0f - kk) + kk) * gv;
                        const float spec = __fdiv_rn(kPi * D * G, 4.0f * NL * NV + 1e-6f);
                        const float w = a.lights[li][3] * NL;
#pragma unroll
                        for (int k = 0; k < 3; ++k) {
                            const float Fk = F0[k] + (1.0f - F0[k]) * x5;
                            out[k] += w * ((1.0f - Fk) * (1.0f - metal) * albedo[k] + spec * Fk);
                        }
                    }
                }
            }
#pragma unroll
            for (int k = 0; k < 3; ++k) acc[k] += fminf(fmaxf(out[k], 0.0f), 1.0f);
            ++covered;
        }
    unsigned char o[4] = {0, 0, 0, 0};
    if (covered) {
#pragma unroll
        for (int k = 0; k < 3; ++k) o[k] = (unsigned char)int(__fdiv_rn(acc[k], float(covered)) * 255.0f + 0.5f);
        o[3] = (unsigned char)int(__fdiv_rn(float(covered), float(s.ss * s.ss)) * 255.0f + 0.5f);
    }
    s.rgba[p * 4] = o[0]; s.rgba[p * 4 + 1] = o[1]; s.rgba[p * 4 + 2] = o[2]; s.rgba[p * 4 + 3] = o[3];
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
    static const float no_light[3] = {0.0f, 0.0f, 0.0f};     // (the one overhead light of s3d_render_shade has no part here)
    PbrArgs a;
    const bool pbr = pbr_table != nullptr;
    // with a PBR table the materials are host arrays: the device table of s3d_render_shade is not read
    S3D_TRY(pack_shade_args("pbr_shade", verts, xy_fixed, inv_w, n_verts, faces, n_faces, face_id, ws, hs, supersample, view_proj, no_light,
                            vertex_colors, uv, face_mat, pbr ? nullptr : mat_table, pbr ? nullptr : mat_kd, pbr ? 0 : n_mats, images, image_bytes,
                            rgba, a.s));
    S3D_CHECK(n_lights >= 0 && n_lights <= S3D_RENDER_MAX_LIGHTS, S3D_ERR_INVALID, "pbr_shade: %d lights (0 to %d)", n_lights,
              S3D_RENDER_MAX_LIGHTS);
    S3D_CHECK(n_lights == 0 || lights, S3D_ERR_INVALID, "pbr_shade: null lights");
    S3D_CHECK(pass >= S3D_RENDER_PASS_SHADED && pass <= S3D_RENDER_PASS_GEO, S3D_ERR_INVALID, "pbr_shade: unknown pass %d", pass);
    S3D_CHECK(eye && std::isfinite(eye[0]) && std::isfinite(eye[1]) && std::isfinite(eye[2]), S3D_ERR_INVALID,
              "pbr_shade: the eye is null or not finite");
    S3D_CHECK(std::isfinite(ambient), S3D_ERR_INVALID, "pbr_shade: ambient is not finite");
    for (int k = 0; k < n_lights * 4; ++k) S3D_CHECK(std::isfinite(lights[k]), S3D_ERR_INVALID, "pbr_shade: light %d is not finite", k / 4);
    S3D_CHECK(!tangents || uv, S3D_ERR_INVALID, "pbr_shade: tangents without uv");
    S3D_CHECK(!pbr || pbr_factors, S3D_ERR_INVALID, "pbr_shade: a PBR table without factors");
    S3D_CHECK(!pbr || (n_mats >= 1 && n_mats <= S3D_RENDER_PBR_MAX_MATERIALS), pbr && n_mats > S3D_RENDER_PBR_MAX_MATERIALS ? S3D_ERR_UNSUPPORTED : S3D_ERR_INVALID,
              "pbr_shade: %d PBR materials (1 to %d: the table travels with the launch)", n_mats, S3D_RENDER_PBR_MAX_MATERIALS);
    memset(a.tab, 0, sizeof(a.tab));
    memset(a.fac, 0, sizeof(a.fac));
    memset(a.lights, 0, sizeof(a.lights));
    if (pbr) {
        static const int channels[4] = {3, 1, 1, 3};
        static const char* const names[4] = {"albedo", "metallic", "roughness", "normal"};
        for (int m = 0; m < n_mats; ++m) {
            for (int j = 0; j < 4; ++j) {
                const int64_t off = pbr_table[(m * 4 + j) * 3], W = pbr_table[(m * 4 + j) * 3 + 1], H = pbr_table[(m * 4 + j) * 3 + 2];
                if (W == 0) continue;                             // absent: the factor
                S3D_CHECK(W >= 1 && H >= 1 && W <= 65536 && H <= 65536 && off >= 0, S3D_ERR_INVALID,
                          "pbr_shade: material %d, %s map: offset %lld, %lld x %lld", m, names[j], (long long)off, (long long)W, (long long)H);
                S3D_CHECK(off + W * H * channels[j] <= image_bytes, S3D_ERR_INVALID,
                          "pbr_shade: material %d, %s map: %lld x %lld x %d bytes at offset %lld run past the %lld image bytes", m, names[j],
                          (long long)W, (long long)H, channels[j], (long long)off, (long long)image_bytes);
                a.tab[m][j][0] = off; a.tab[m][j][1] = W; a.tab[m][j][2] = H;
            }
            for (int k = 0; k < 5; ++k) {
                S3D_CHECK(std::isfinite(pbr_factors[m * 5 + k]), S3D_ERR_INVALID, "pbr_shade: material %d: factor %d is not finite", m, k);
                a.fac[m][k] = pbr_factors[m * 5 + k];
            }
        }
        a.s.M = n_mats;
    }
    a.normals = normals; a.tangents = tangents; a.pbr = pbr ? 1 : 0; a.n_lights = n_lights; a.pass = pass; a.ambient = ambient;
    for (int k = 0; k < 3; ++k) a.eye[k] = eye[k];
    for (int k = 0; k < n_lights * 4; ++k) a.lights[k / 4][k % 4] = lights[k];
    hipLaunchKernelGGL(k_render_shade_pbr, dim3(pbr_blocks((long long)a.s.W * a.s.H)), dim3(kPbrThreads), 0, static_cast<hipStream_t>(stream), a);
    S3D_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
