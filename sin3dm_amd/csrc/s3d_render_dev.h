// s3d_render_dev.h — what the kernels of s3d_render.hip and s3d_render_pbr.hip share: a face on the screen, its
// exact edge values, the perspective-correct barycentrics of a sample, the bilinear lookup, the base colour of a sample and the
// argument checks of the entry points.  One definition each, so that the flat and the PBR shader cannot drift apart.
#pragma once
#include "s3d_common.h"

#include <cmath>

namespace s3d {

constexpr int kSub = S3D_RENDER_SUBPIXEL;              // fixed-point units per sample
constexpr int kMaxCoord = S3D_RENDER_MAX_COORD;        // |snapped coordinate| of a drawn triangle: products of two differences fit 2^43

enum TriStatus { TRI_OK = 0, TRI_NEAR = 1, TRI_RANGE = 2, TRI_DEGENERATE = 3 };

// ------------------------------------------------------------------ a face on the screen.  The corners are ordered so that the doubled
// area (x1 - x0)(y2 - y0) - (y1 - y0)(x2 - x0) is positive (corners 1 and 2 exchanged when it was negative: `swapped`), so that the
// inside of every edge is the positive side.
struct ScreenTri { int x0, y0, x1, y1, x2, y2; float iw0, iw1, iw2; int v0, v1, v2; long long area2; bool swapped; };

__device__ __forceinline__ int load_screen_tri(const int* __restrict__ xy, const float* __restrict__ inv_w, long long V,
                                               const int* __restrict__ faces, long long f, ScreenTri& t) {
    const int a = faces[f * 3], b = faces[f * 3 + 1], c = faces[f * 3 + 2];
    if (a < 0 || b < 0 || c < 0 || a >= V || b >= V || c >= V) return TRI_RANGE;
    t.iw0 = inv_w[a]; t.iw1 = inv_w[b]; t.iw2 = inv_w[c];
    if (!(t.iw0 > 0.0f) || !(t.iw1 > 0.0f) || !(t.iw2 > 0.0f)) return TRI_NEAR;
    t.x0 = xy[a * 2LL]; t.y0 = xy[a * 2LL + 1];
    t.x1 = xy[b * 2LL]; t.y1 = xy[b * 2LL + 1];
    t.x2 = xy[c * 2LL]; t.y2 = xy[c * 2LL + 1];
    if (max(max(abs(t.x0), abs(t.x1)), max(max(abs(t.x2), abs(t.y0)), max(abs(t.y1), abs(t.y2)))) > kMaxCoord) return TRI_RANGE;
    t.v0 = a; t.v1 = b; t.v2 = c;
    t.area2 = (long long)(t.x1 - t.x0) * (t.y2 - t.y0) - (long long)(t.y1 - t.y0) * (t.x2 - t.x0);
    if (t.area2 == 0) return TRI_DEGENERATE;
    t.swapped = t.area2 < 0;
    if (t.swapped) {
        int s;
        s = t.x1; t.x1 = t.x2; t.x2 = s;
        s = t.y1; t.y1 = t.y2; t.y2 = s;
        s = t.v1; t.v1 = t.v2; t.v2 = s;
        const float w = t.iw1; t.iw1 = t.iw2; t.iw2 = w;
        t.area2 = -t.area2;
    }
    return TRI_OK;
}

// One edge a -> b as E(p) = A px + B py + C with the inside positive, and whether a sample ON the edge belongs to the triangle:
// the sample is tested as if it stood at p + (-eps, -eps^2), which moves E by dy eps - dx eps^2 — positive exactly when
// dy > 0, or dy == 0 and dx < 0 (the top-left rule).  One displaced point lies in exactly one triangle of a tiling.
struct Edge { int A, B; long long C; int tl; };
__device__ __forceinline__ Edge make_edge(int xa, int ya, int xb, int yb) {
    Edge e;
    const int dx = xb - xa, dy = yb - ya;
    e.A = -dy; e.B = dx;
    e.C = -((long long)e.A * xa + (long long)e.B * ya);
    e.tl = (dy > 0 || (dy == 0 && dx < 0)) ? 1 : 0;
    return e;
}
__device__ __forceinline__ long long edge_at(int A, int B, long long C, int px, int py) { return (long long)A * px + (long long)B * py + C; }
__device__ __forceinline__ bool edge_inside(long long E, int tl) { return E + tl > 0; }

// The perspective-correct barycentrics of sample (sx, sy) in the ordered triangle: the edge values again (exact),
// b_k = E_k iw_k / sum.
__device__ __forceinline__ void sample_barycentrics(const ScreenTri& t, int sx, int sy, float& b0, float& b1, float& b2) {
    const int px = sx * kSub + kSub / 2, py = sy * kSub + kSub / 2;
    const Edge e01 = make_edge(t.x0, t.y0, t.x1, t.y1), e12 = make_edge(t.x1, t.y1, t.x2, t.y2), e20 = make_edge(t.x2, t.y2, t.x0, t.y0);
    const float n0 = float(edge_at(e12.A, e12.B, e12.C, px, py)) * t.iw0, n1 = float(edge_at(e20.A, e20.B, e20.C, px, py)) * t.iw1,
                n2 = float(edge_at(e01.A, e01.B, e01.C, px, py)) * t.iw2;
    const float sum = n0 + n1 + n2;
    b0 = __fdiv_rn(n0, sum); b1 = __fdiv_rn(n1, sum); b2 = __fdiv_rn(n2, sum);
}

// Bilinear lookup, the GL / Blender convention: texel (i, j) is centred at u = (i + 0.5) / W, v = 1 - (j + 0.5) / H with row j = 0
// the top row of the image; clamp to edge.  CH interleaved channels per texel; the result is in [0, 1].
template <int CH>
__device__ __forceinline__ void texel(const unsigned char* __restrict__ img, long long off, long long W, int x, int y, float c[CH]) {
    const unsigned char* p = img + off + ((long long)y * W + x) * CH;
#pragma unroll
    for (int k = 0; k < CH; ++k) c[k] = float(p[k]);
}
template <int CH>
__device__ __forceinline__ void tex_bilinear(const unsigned char* __restrict__ img, long long off, int W, int H, float u, float v, float c[CH]) {
    const float x = fminf(fmaxf(u * float(W) - 0.5f, -1.0f), float(W)), y = fminf(fmaxf((1.0f - v) * float(H) - 0.5f, -1.0f), float(H));
    const float xf = floorf(x), yf = floorf(y), fx = x - xf, fy = y - yf;
    const int x0 = min(max(int(xf), 0), W - 1), x1 = min(max(int(xf) + 1, 0), W - 1);
    const int y0 = min(max(int(yf), 0), H - 1), y1 = min(max(int(yf) + 1, 0), H - 1);
    float c00[CH], c10[CH], c01[CH], c11[CH];
    texel<CH>(img, off, W, x0, y0, c00); texel<CH>(img, off, W, x1, y0, c10); texel<CH>(img, off, W, x0, y1, c01); texel<CH>(img, off, W, x1, y1, c11);
#pragma unroll
    for (int k = 0; k < CH; ++k) {
        const float top = c00[k] + fx * (c10[k] - c00[k]), bot = c01[k] + fx * (c11[k] - c01[k]);
        c[k] = __fdiv_rn(top + fy * (bot - top), 255.0f);
    }
}

// the uv of a sample: the corners of uv [F][3][2] are in the face's own order, the barycentrics in the ordered triangle's
__device__ __forceinline__ void sample_uv(const float* __restrict__ uv, long long f, bool swapped, float b0, float b1, float b2, float& tu, float& tv) {
    const float* q = uv + f * 6;
    const int c1 = swapped ? 4 : 2, c2 = swapped ? 2 : 4;
    tu = b0 * q[0] + b1 * q[c1] + b2 * q[c2]; tv = b0 * q[1] + b1 * q[c1 + 1] + b2 * q[c2 + 1];
}

struct ShadeArgs {
    const float* verts; const int* xy; const float* inv_w; long long V;
    const int* faces; long long F;
    const int* face_id; int ws, hs, ss, W, H;
    float light[3]; int front_sign;
    const float* vcol; const float* uv; const int* face_mat;
    const long long* mat; const float* kd; int M;
    const unsigned char* img; long long img_bytes;
    unsigned char* rgba;
};

// base colour of a sample of face f: vertex colours, or the material's image at the interpolated uv, or its Kd; otherwise c is
// left as the caller set it, to white (set there, not here: set here, k_render_shade's uv-to-texel step lost two fused multiply-adds)
__device__ __forceinline__ void base_colour(const ShadeArgs& a, const ScreenTri& t, int f, float b0, float b1, float b2, float c[3]) {
    if (a.vcol) {
#pragma unroll
        for (int k = 0; k < 3; ++k) c[k] = b0 * a.vcol[t.v0 * 3LL + k] + b1 * a.vcol[t.v1 * 3LL + k] + b2 * a.vcol[t.v2 * 3LL + k];
    } else if (a.M > 0) {
        const int m = a.face_mat ? a.face_mat[f] : 0;
        if (m >= 0 && m < a.M) {
            c[0] = a.kd[m * 3]; c[1] = a.kd[m * 3 + 1]; c[2] = a.kd[m * 3 + 2];
            const long long off = a.mat[m * 3], W = a.mat[m * 3 + 1], H = a.mat[m * 3 + 2];
            if (a.uv && W > 0 && H > 0 && off >= 0 && W <= 65536 && H <= 65536 && off + W * H * 3 <= a.img_bytes) {
                float tu, tv;
                sample_uv(a.uv, f, t.swapped, b0, b1, b2, tu, tv);
                tex_bilinear<3>(a.img, off, int(W), int(H), tu, tv, c);
            }
        }
    }
}

// the normal of face f in its own vertex order, not normalised; front: whether that side faces the camera.  Own order: the screen
// area (rows downwards) is negative when `swapped`.  A right-handed camera (front_sign -1) sees a face whose normal points at it
// counter-clockwise, which is a negative area here: front when the product is positive — decided exactly, on integers.
__device__ __forceinline__ void face_normal(const float* __restrict__ verts, const ScreenTri& t, int front_sign, float n[3], bool& front) {
    const int o1 = t.swapped ? t.v2 : t.v1, o2 = t.swapped ? t.v1 : t.v2;
    const float* A = verts + t.v0 * 3LL;
    const float* B = verts + o1 * 3LL;
    const float* Cc = verts + o2 * 3LL;
    const float ux = B[0] - A[0], uy = B[1] - A[1], uz = B[2] - A[2], vx = Cc[0] - A[0], vy = Cc[1] - A[1], vz = Cc[2] - A[2];
    n[0] = uy * vz - uz * vy; n[1] = uz * vx - ux * vz; n[2] = ux * vy - uy * vx;
    front = (t.swapped ? -1 : 1) * front_sign > 0;
}

// ------------------------------------------------------------------ host: the argument checks of the entry points
static inline int check_grid_size(const char* who, int ws, int hs) {
    S3D_CHECK(ws >= 1 && hs >= 1 && ws <= S3D_RENDER_MAX_GRID && hs <= S3D_RENDER_MAX_GRID, S3D_ERR_INVALID,
              "%s: sample grid %d x %d (1 to %d a side)", who, ws, hs, S3D_RENDER_MAX_GRID);
    return 0;
}
static inline int check_mesh(const char* who, const void* xy, const void* inv_w, int64_t n_verts, const void* faces, int64_t n_faces) {
    S3D_CHECK(n_verts >= 0 && n_verts <= INT32_MAX && n_faces >= 0 && n_faces <= INT32_MAX, S3D_ERR_INVALID, "%s: %lld vertices, %lld faces", who,
              (long long)n_verts, (long long)n_faces);
    S3D_CHECK(n_faces == 0 || faces, S3D_ERR_INVALID, "%s: null face table", who);
    S3D_CHECK(n_verts == 0 || (xy && inv_w), S3D_ERR_INVALID, "%s: null vertex table", who);
    return 0;
}
// the handedness of an object-to-clip matrix: the sign of the determinant of the x, y and w rows' linear parts
static inline int matrix_front_sign(const float m[16]) {
    const double det = double(m[0]) * (double(m[5]) * m[14] - double(m[6]) * m[13]) - double(m[1]) * (double(m[4]) * m[14] - double(m[6]) * m[12]) +
                       double(m[2]) * (double(m[4]) * m[13] - double(m[5]) * m[12]);
    return det < 0.0 ? -1 : 1;
}
// the arguments s3d_render_shade and s3d_pbr_shade share, checked and packed (front_sign: matrix_front_sign)
static inline int pack_shade_args(const char* who, const float* verts, const int32_t* xy_fixed, const float* inv_w, int64_t n_verts,
                                  const int32_t* faces, int64_t n_faces, const int32_t* face_id, int ws, int hs, int supersample,
                                  const float view_proj[16], const float light[3], const float* vertex_colors, const float* uv,
                                  const int32_t* face_mat, const int64_t* mat_table, const float* mat_kd, int n_mats, const uint8_t* images,
                                  int64_t image_bytes, uint8_t* rgba, ShadeArgs& a) {
    S3D_TRY(check_grid_size(who, ws, hs));
    S3D_TRY(check_mesh(who, xy_fixed, inv_w, n_verts, faces, n_faces));
    S3D_CHECK(supersample >= 1 && supersample <= 8 && ws % supersample == 0 && hs % supersample == 0, S3D_ERR_INVALID,
              "%s: supersample %d (1 to 8, dividing the %d x %d sample grid)", who, supersample, ws, hs);
    S3D_CHECK(view_proj && light, S3D_ERR_INVALID, "%s: null matrix or light", who);
    for (int k = 0; k < 16; ++k) S3D_CHECK(std::isfinite(view_proj[k]), S3D_ERR_INVALID, "%s: matrix entry %d is not finite", who, k);
    S3D_CHECK(std::isfinite(light[0]) && std::isfinite(light[1]) && std::isfinite(light[2]), S3D_ERR_INVALID, "%s: light is not finite", who);
    S3D_CHECK(n_mats >= 0 && n_mats <= (1 << 20) && image_bytes >= 0, S3D_ERR_INVALID, "%s: bad material sizes", who);
    S3D_CHECK(n_mats == 0 || (mat_table && mat_kd), S3D_ERR_INVALID, "%s: null material table", who);
    S3D_CHECK(image_bytes == 0 || images, S3D_ERR_INVALID, "%s: null image buffer", who);
    S3D_CHECK(face_id && rgba && (n_verts == 0 || verts), S3D_ERR_INVALID, "%s: null argument", who);
    a.verts = verts; a.xy = xy_fixed; a.inv_w = inv_w; a.V = n_verts; a.faces = faces; a.F = n_faces; a.face_id = face_id;
    a.ws = ws; a.hs = hs; a.ss = supersample; a.W = ws / supersample; a.H = hs / supersample;
    a.light[0] = light[0]; a.light[1] = light[1]; a.light[2] = light[2];
    a.front_sign = matrix_front_sign(view_proj);
    a.vcol = vertex_colors; a.uv = uv; a.face_mat = face_mat; a.mat = reinterpret_cast<const long long*>(mat_table); a.kd = mat_kd; a.M = n_mats;
    a.img = images; a.img_bytes = image_bytes; a.rgba = rgba;
    return 0;
}

}  // namespace s3d
