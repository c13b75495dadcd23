// s3d_pbr_shade.h — what the two kernels around s3d_pbr_shade_body.h share: k_render_shade_pbr of
// s3d_render_pbr.hip and k_render_shade_pbr_lit of s3d_ray.hip, which skips the lights a shadow mask switches off.  The argument
// block, the small vector helpers and the checks and packing of the entry points' arguments: one definition each.
#pragma once
#include "s3d_render_dev.h"

#include <cstring>

namespace s3d {

constexpr int kPbrThreads = 256;
constexpr int kMaxLights = S3D_RENDER_MAX_LIGHTS;
constexpr int kMaxPbrMats = S3D_RENDER_PBR_MAX_MATERIALS;
static inline unsigned pbr_blocks(long long n) { return (unsigned)((n + kPbrThreads - 1) / kPbrThreads); }

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

// the lights of an entry point: at most S3D_RENDER_MAX_LIGHTS rows of four finite floats
static inline int check_lights(const char* who, const float* lights, int n_lights) {
    S3D_CHECK(n_lights >= 0 && n_lights <= S3D_RENDER_MAX_LIGHTS, S3D_ERR_INVALID, "%s: %d lights (0 to %d)", who, n_lights, S3D_RENDER_MAX_LIGHTS);
    S3D_CHECK(n_lights == 0 || lights, S3D_ERR_INVALID, "%s: null lights", who);
    for (int k = 0; k < n_lights * 4; ++k) S3D_CHECK(std::isfinite(lights[k]), S3D_ERR_INVALID, "%s: light %d is not finite", who, k / 4);
    return 0;
}

// the arguments of s3d_pbr_shade and s3d_pbr_shade_lit, checked and packed
static inline int pack_pbr_args(const char* who, const float* verts, const int32_t* xy_fixed, const float* inv_w, int64_t n_verts,
                                const int32_t* faces, int64_t n_faces, const int32_t* face_id, int ws, int hs, int supersample,
                                const float view_proj[16], const float* vertex_colors, const float* uv, const int32_t* face_mat,
                                const int64_t* mat_table, const float* mat_kd, int n_mats, const uint8_t* images, int64_t image_bytes,
                                const float* normals, const float* tangents, const int64_t* pbr_table, const float* pbr_factors, const float eye[3],
                                const float* lights, int n_lights, float ambient, int pass, uint8_t* rgba, PbrArgs& a) {
    static const float no_light[3] = {0.0f, 0.0f, 0.0f};     // (the one overhead light of s3d_render_shade has no part here)
    const bool pbr = pbr_table != nullptr;
    // with a PBR table the materials are host arrays: the device table of s3d_render_shade is not read
    S3D_TRY(pack_shade_args(who, verts, xy_fixed, inv_w, n_verts, faces, n_faces, face_id, ws, hs, supersample, view_proj, no_light,
                            vertex_colors, uv, face_mat, pbr ? nullptr : mat_table, pbr ? nullptr : mat_kd, pbr ? 0 : n_mats, images, image_bytes,
                            rgba, a.s));
    S3D_TRY(check_lights(who, lights, n_lights));
    S3D_CHECK(pass >= S3D_RENDER_PASS_SHADED && pass <= S3D_RENDER_PASS_GEO, S3D_ERR_INVALID, "%s: unknown pass %d", who, pass);
    S3D_CHECK(eye && std::isfinite(eye[0]) && std::isfinite(eye[1]) && std::isfinite(eye[2]), S3D_ERR_INVALID,
              "%s: the eye is null or not finite", who);
    S3D_CHECK(std::isfinite(ambient), S3D_ERR_INVALID, "%s: ambient is not finite", who);
    S3D_CHECK(!tangents || uv, S3D_ERR_INVALID, "%s: tangents without uv", who);
    S3D_CHECK(!pbr || pbr_factors, S3D_ERR_INVALID, "%s: a PBR table without factors", who);
    S3D_CHECK(!pbr || (n_mats >= 1 && n_mats <= S3D_RENDER_PBR_MAX_MATERIALS), pbr && n_mats > S3D_RENDER_PBR_MAX_MATERIALS ? S3D_ERR_UNSUPPORTED : S3D_ERR_INVALID,
              "%s: %d PBR materials (1 to %d: the table travels with the launch)", who, n_mats, S3D_RENDER_PBR_MAX_MATERIALS);
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
                          "%s: material %d, %s map: offset %lld, %lld x %lld", who, m, names[j], (long long)off, (long long)W, (long long)H);
                S3D_CHECK(off + W * H * channels[j] <= image_bytes, S3D_ERR_INVALID,
                          "%s: material %d, %s map: %lld x %lld x %d bytes at offset %lld run past the %lld image bytes", who, m, names[j],
                          (long long)W, (long long)H, channels[j], (long long)off, (long long)image_bytes);
                a.tab[m][j][0] = off; a.tab[m][j][1] = W; a.tab[m][j][2] = H;
            }
            for (int k = 0; k < 5; ++k) {
                S3D_CHECK(std::isfinite(pbr_factors[m * 5 + k]), S3D_ERR_INVALID, "%s: material %d: factor %d is not finite", who, m, k);
                a.fac[m][k] = pbr_factors[m * 5 + k];
            }
        }
        a.s.M = n_mats;
    }
    a.normals = normals; a.tangents = tangents; a.pbr = pbr ? 1 : 0; a.n_lights = n_lights; a.pass = pass; a.ambient = ambient;
    for (int k = 0; k < 3; ++k) a.eye[k] = eye[k];
    for (int k = 0; k < n_lights * 4; ++k) a.lights[k / 4][k % 4] = lights[k];
    return 0;
}

}  // namespace s3d
