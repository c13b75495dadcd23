// s3d_meshpbr.hip — the eight material channels of (face, barycentrics) pairs for the PBR variant of the mesh preprocessing (the
// reference's data/mesh_sampler_pbr.py, by an own design; DESIGN.md §16, "PBR variant"): albedo rgb | metallic | roughness |
// normal xyz, each from the nearest texel of its own map by the rule of k_mesh_texture (s3d_meshsdf.hip), or from the material's
// factor where the map is absent.  One thread per query; every row is written by one thread, so the result does not depend on
// the launch geometry.
#include "s3d_common.h"

namespace s3d {

constexpr int kPbrThreads = 256;
constexpr int kPbrMaps = 4;                    // albedo, metallic, roughness, normal: the rows of a material's table entry
static inline unsigned pbr_blocks(long long n) { return (unsigned)((n + kPbrThreads - 1) / kPbrThreads); }

// k_mesh_texture's texel of a W x H map at (tu, tv): x = rint(tu (W - 1)) mod W, y = rint((1 - tv) (H - 1)) mod H, half to even.
// False (a NaN from inf * 0, or a runaway coordinate): the caller keeps the fallback.
__device__ __forceinline__ bool texel_index(float tu, float tv, long long W, long long H, long long& idx) {
    const float fx = rintf(tu * float(W - 1)), fy = rintf((1.0f - tv) * float(H - 1));
    if (!(fabsf(fx) < 1e9f && fabsf(fy) < 1e9f)) return false;
    const int w = int(W), h = int(H);                                                    // W, H <= 65536 and |fx|, |fy| < 1e9: all of it fits 32 bits
    const int x = ((int(fx) % w) + w) % w, y = ((int(fy) % h) + h) % h;
    idx = (long long)y * W + x;
    return true;
}

// table [M][4][3] = {byte offset, W, H} of the albedo (RGB), metallic (one plane), roughness (one plane) and normal (RGB) map of
// a material, W = 0: absent; factors [M][5] = Kd rgb, metallic, roughness.  A map that would run past img_bytes counts as absent.
__global__ void __launch_bounds__(kPbrThreads) k_mesh_texture_pbr(const int* __restrict__ face, const float* __restrict__ bary, long long N,
                                                                  const float* __restrict__ uv, const int* __restrict__ face_mat, long long F,
                                                                  const long long* __restrict__ table, const float* __restrict__ factors, int M,
                                                                  const unsigned char* __restrict__ img, long long img_bytes,
                                                                  float* __restrict__ out) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const int f = face[i];
    float c[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    if (f >= 0 && f < F) {
        const int m = face_mat[f];
        if (m >= 0 && m < M) {
            const float* fac = factors + (long long)m * 5;
            c[0] = fac[0]; c[1] = fac[1]; c[2] = fac[2]; c[3] = fac[3]; c[4] = fac[4];
            c[5] = __fdiv_rn(128.0f, 255.0f); c[6] = c[5]; c[7] = 1.0f;                  // the flat tangent-space normal (128, 128, 255) / 255
            const float b0 = bary[i * 3], b1 = bary[i * 3 + 1], b2 = bary[i * 3 + 2];
            const float* q = uv + (long long)f * 6;
            float tu = b0 * q[0] + b1 * q[2] + b2 * q[4], tv = b0 * q[1] + b1 * q[3] + b2 * q[5];
            tu = tu != tu ? 0.0f : tu;                                                    // a NaN uv component reads the texel of 0
            tv = tv != tv ? 0.0f : tv;
            const long long* t = table + (long long)m * (kPbrMaps * 3);
            long long off[kPbrMaps], W[kPbrMaps], H[kPbrMaps], idx[kPbrMaps];
            bool ok[kPbrMaps];
#pragma unroll
            for (int j = 0; j < kPbrMaps; ++j) {
                const long long ch = (j == 0 || j == 3) ? 3 : 1;
                off[j] = t[j * 3]; W[j] = t[j * 3 + 1]; H[j] = t[j * 3 + 2];
                const bool present = W[j] > 0 && H[j] > 0 && off[j] >= 0 && W[j] <= 65536 && H[j] <= 65536 && off[j] + W[j] * H[j] * ch <= img_bytes;
                if (!present) W[j] = 0;
                ok[j] = false; idx[j] = 0;
                if (present) {
                    bool found = false;
#pragma unroll
                    for (int k = 0; k < j; ++k)                                         // two maps of one size share the index
                        if (!found && W[k] == W[j] && H[k] == H[j]) { ok[j] = ok[k]; idx[j] = idx[k]; found = true; }
                    if (!found) ok[j] = texel_index(tu, tv, W[j], H[j], idx[j]);
                }
            }
            if (ok[0]) {
                const unsigned char* px = img + off[0] + idx[0] * 3;
#pragma unroll
                for (int k = 0; k < 3; ++k) c[k] = __fdiv_rn(float(px[k]), 255.0f);
            }
            if (ok[1]) c[3] = __fdiv_rn(float(img[off[1] + idx[1]]), 255.0f);
            if (ok[2]) c[4] = __fdiv_rn(float(img[off[2] + idx[2]]), 255.0f);
            if (ok[3]) {
                const unsigned char* px = img + off[3] + idx[3] * 3;
#pragma unroll
                for (int k = 0; k < 3; ++k) c[5 + k] = __fdiv_rn(float(px[k]), 255.0f);
            }
        }
    }
    float4* row = reinterpret_cast<float4*>(out) + i * 2;                                 // 32 bytes a row: the launcher checked the alignment
    row[0] = make_float4(c[0], c[1], c[2], c[3]);
    row[1] = make_float4(c[4], c[5], c[6], c[7]);
}

}  // namespace s3d

using namespace s3d;

extern "C" {

int s3d_meshsdf_texture_pbr(const int32_t* face, const float* bary, int64_t n, const float* uv, const int32_t* face_mat, int64_t n_faces,
                            const int64_t* mat_table, const float* mat_factors, int n_mats, const uint8_t* images, int64_t image_bytes,
                            float* out, void* stream) {
    S3D_CHECK(n >= 0 && n_faces >= 0 && n_faces <= INT32_MAX && n_mats >= 0 && n_mats <= (1 << 20) && image_bytes >= 0, S3D_ERR_INVALID,
              "meshsdf_texture_pbr: bad sizes");
    S3D_CHECK(n == 0 || (face && bary && out), S3D_ERR_INVALID, "meshsdf_texture_pbr: null argument");
    S3D_CHECK(n_faces == 0 || (uv && face_mat), S3D_ERR_INVALID, "meshsdf_texture_pbr: null face table");
    S3D_CHECK(n_mats == 0 || (mat_table && mat_factors), S3D_ERR_INVALID, "meshsdf_texture_pbr: null material table");
    S3D_CHECK(image_bytes == 0 || images, S3D_ERR_INVALID, "meshsdf_texture_pbr: null image buffer");
    S3D_CHECK(n == 0 || reinterpret_cast<uintptr_t>(out) % 16 == 0, S3D_ERR_INVALID,
              "meshsdf_texture_pbr: out %p is not 16-byte aligned (a row is written as two float4)", (void*)out);
    if (!n) return 0;
    S3D_CHECK((n + kPbrThreads - 1) / kPbrThreads <= INT32_MAX, S3D_ERR_UNSUPPORTED, "meshsdf_texture_pbr: %lld queries in one call", (long long)n);
    hipLaunchKernelGGL(k_mesh_texture_pbr, dim3(pbr_blocks(n)), dim3(kPbrThreads), 0, static_cast<hipStream_t>(stream), face, bary,
                       (long long)n, uv, face_mat, (long long)n_faces, reinterpret_cast<const long long*>(mat_table), mat_factors, n_mats,
                       images, (long long)image_bytes, out);
    S3D_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
