// s3d_tex.hip — what follows the iso-surface in decode_texmesh (src/encoding/model.py:389-430), on the device: vertex-clustering
// decimation (keys, segment means, face remap), the per-face atlas's texel positions, and the texture finishing (quantise,
// 3x3 dilation), and the field's normals as a tangent-space map on that atlas.  Sorting, unique and compaction
// stay with the caller (torch), as for largest_component.  DESIGN.md §15.
// Every kernel is one thread per output element, integer or fixed-order arithmetic only: no float atomics, so the results
// are deterministic.  Divisions are __fdiv_rn (correctly rounded) so that a NumPy float32 restatement gives the same cells.
#include "s3d_common.h"

namespace s3d {

constexpr int kTexThreads = 256;
static inline unsigned tex_blocks(long long n) { return (unsigned)((n + kTexThreads - 1) / kTexThreads); }

// ------------------------------------------------------------------ decimation: vertex clustering on a uniform grid
// key[v] = linear index of v's cell: per axis min(R_axis - 1, floor((v - lo) / s)) in fp32
__global__ void __launch_bounds__(kTexThreads) k_cluster_keys(const float* __restrict__ verts, long long nv, float lx, float ly, float lz,
                                                              float s, int rx, int ry, int rz, long long* __restrict__ keys) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nv) return;
    const int ix = min(rx - 1, max(0, int(floorf(__fdiv_rn(verts[i * 3] - lx, s)))));
    const int iy = min(ry - 1, max(0, int(floorf(__fdiv_rn(verts[i * 3 + 1] - ly, s)))));
    const int iz = min(rz - 1, max(0, int(floorf(__fdiv_rn(verts[i * 3 + 2] - lz, s)))));
    keys[i] = ((long long)ix * ry + iy) * rz + iz;
}

// out[cl][ch] = mean of vals[order[j]][ch] over the segment j in [seg[cl], seg[cl+1]): one thread walks one segment of one channel
// in the sorted order, accumulating in double (the rounding of the mean is then the single conversion to fp32)
__global__ void __launch_bounds__(kTexThreads) k_cluster_means(const float* __restrict__ vals, int C, const long long* __restrict__ order,
                                                               const long long* __restrict__ seg, long long nc, long long nv,
                                                               float* __restrict__ out) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nc * C) return;
    const long long cl = t / C;
    const int ch = int(t - cl * C);
    const long long b = max(0LL, seg[cl]), e = min(nv, seg[cl + 1]);
    double acc = 0.0;
    for (long long j = b; j < e; ++j) {
        const long long v = order[j];
        if (v >= 0 && v < nv) acc += double(vals[v * C + ch]);
    }
    out[t] = e > b ? float(acc / double(e - b)) : 0.0f;
}

// faces through the clusters: out = vmap[tris]; fkey = the face's vertex SET as one integer ((lo * nc + mid) * nc + hi), or -1 for
// a face with two equal indices (or an index outside the vertex array)
__global__ void __launch_bounds__(kTexThreads) k_remap_faces(const int* __restrict__ tris, long long nt, const int* __restrict__ vmap,
                                                             long long nv, long long nc, int* __restrict__ out,
                                                             long long* __restrict__ fkey) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nt) return;
    const int ia = tris[i * 3], ib = tris[i * 3 + 1], ic = tris[i * 3 + 2];
    const bool ok = ia >= 0 && ia < nv && ib >= 0 && ib < nv && ic >= 0 && ic < nv;
    const int a = ok ? vmap[ia] : 0, b = ok ? vmap[ib] : 0, c = ok ? vmap[ic] : 0;
    out[i * 3] = a; out[i * 3 + 1] = b; out[i * 3 + 2] = c;
    if (!ok || a == b || b == c || a == c) { fkey[i] = -1; return; }
    const long long lo = min(a, min(b, c)), hi = max(a, max(b, c)), mid = (long long)a + b + c - lo - hi;
    fkey[i] = (lo * nc + mid) * nc + hi;
}

// ------------------------------------------------------------------ atlas: which vertex sits in the chart's right angle
// corner0[f] = index (0..2) of the vertex opposite the face's longest edge; ties: the first of v0v1, v1v2, v2v0
__global__ void __launch_bounds__(kTexThreads) k_face_corner0(const float* __restrict__ verts, const int* __restrict__ tris, long long F,
                                                              long long nv, int* __restrict__ corner0) {
    const long long f = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= F) return;
    float p[3][3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const int v = tris[f * 3 + j];
        const bool ok = v >= 0 && v < nv;
#pragma unroll
        for (int k = 0; k < 3; ++k) p[j][k] = ok ? verts[(long long)v * 3 + k] : 0.0f;
    }
    float d[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const int n = (j + 1) % 3;
        const float dx = p[n][0] - p[j][0], dy = p[n][1] - p[j][1], dz = p[n][2] - p[j][2];
        d[j] = dx * dx + dy * dy + dz * dz;
    }
    int e = 0;
    float m = d[0];
    if (d[1] > m) { e = 1; m = d[1]; }
    if (d[2] > m) e = 2;
    corner0[f] = (e + 2) % 3;               // edge e joins vertices e and e+1: the third one is opposite
}

// One thread per texel of the T x T atlas (n x n cells of c x c texels, two faces per cell; texel (x, y) at y * T + x):
// face_id = the face whose closed chart triangle holds the texel centre (integer test at 2x scale, reduced) or -1;
// pos = b0 V0 + b1 V1 + b2 V2 with the barycentrics of the centre, V0 the corner0 vertex, V1 / V2 after it in the face's order.
__global__ void __launch_bounds__(kTexThreads) k_texel_positions(const float* __restrict__ verts, const int* __restrict__ tris,
                                                                 const int* __restrict__ corner0, long long F, long long nv, int T, int n, int c,
                                                                 int* __restrict__ face_id, float* __restrict__ pos) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (long long)T * T) return;
    const int x = int(t % T), y = int(t / T);
    const int col = x / c, row = y / c;
    long long k = -1;
    int u = 0, v = 0;
    if (col < n && row < n) {
        const int lx = x - col * c, ly = y - row * c;
        const long long cell = (long long)row * n + col;
        // lower chart (1,1) (c-4,1) (1,c-4): 2x+1 >= 2, 2y+1 >= 2, (2x+1) + (2y+1) <= 2c-6
        if (lx >= 1 && ly >= 1 && lx + ly <= c - 4) { k = 2 * cell; u = lx; v = ly; }
        // upper chart (c-1,c-1) (4,c-1) (c-1,4): the same triangle mirrored through the cell centre
        else if (lx <= c - 2 && ly <= c - 2 && lx + ly >= c + 2) { k = 2 * cell + 1; u = c - 1 - lx; v = c - 1 - ly; }
        if (k >= F) k = -1;
    }
    int vi[3] = {0, 0, 0};
    bool ok = k >= 0;
    if (ok) {
        const int r = min(2, max(0, corner0[k]));
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            vi[j] = tris[k * 3 + (r + j) % 3];
            ok = ok && vi[j] >= 0 && vi[j] < nv;
        }
    }
    if (!ok) {
        face_id[t] = -1;
        pos[t * 3] = 0.0f; pos[t * 3 + 1] = 0.0f; pos[t * 3 + 2] = 0.0f;
        return;
    }
    const float L = float(c - 5);
    const float b1 = __fdiv_rn(float(u) - 0.5f, L), b2 = __fdiv_rn(float(v) - 0.5f, L), b0 = 1.0f - b1 - b2;
    face_id[t] = int(k);
#pragma unroll
    for (int j = 0; j < 3; ++j)
        pos[t * 3 + j] = b0 * verts[(long long)vi[0] * 3 + j] + b1 * verts[(long long)vi[1] * 3 + j] + b2 * verts[(long long)vi[2] * 3 + j];
}

// ------------------------------------------------------------------ texture finishing
// img[idx[i]][ch] = uint8(col[i][ch] * 255), truncating (numpy's astype(np.uint8) on the reference's clamped colours)
__global__ void __launch_bounds__(kTexThreads) k_tex_quantize(const float* __restrict__ col, const long long* __restrict__ idx, long long N, int C,
                                                              long long TT, unsigned char* __restrict__ img) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= N * C) return;
    const long long i = t / C;
    const int ch = int(t - i * C);
    const long long p = idx[i];
    if (p < 0 || p >= TT) return;
    img[p * C + ch] = (unsigned char)int(fminf(fmaxf(col[t] * 255.0f, 0.0f), 255.0f));
}

// cv2.dilate(img, ones(3,3)) where the mask is off, img where it is on (model.py:426-428): an uncovered texel takes the
// per-channel maximum of its 3 x 3 neighbourhood of the quantised image; neighbours outside the image do not take part
__global__ void __launch_bounds__(kTexThreads) k_tex_dilate(const unsigned char* __restrict__ q, const int* __restrict__ face_id, int T, int C,
                                                            unsigned char* __restrict__ out) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (long long)T * T * C) return;
    const long long px = t / C;
    const int ch = int(t - px * C);
    if (face_id[px] >= 0) { out[t] = q[t]; return; }
    const int x = int(px % T), y = int(px / T);
    int m = 0;
    for (int dy = -1; dy <= 1; ++dy) {
        const int yy = y + dy;
        if (yy < 0 || yy >= T) continue;
        for (int dx = -1; dx <= 1; ++dx) {
            const int xx = x + dx;
            if (xx < 0 || xx >= T) continue;
            m = max(m, int(q[((long long)yy * T + xx) * C + ch]));
        }
    }
    out[t] = (unsigned char)m;
}

// ------------------------------------------------------------------ tangent-space normal map of the field
// every texel the flat normal (128, 128, 255), status 0: what k_normal_texels does not reach keeps it
__global__ void __launch_bounds__(kTexThreads) k_normal_fill(long long TT, unsigned char* __restrict__ img, unsigned char* __restrict__ status) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= TT) return;
    img[t * 3] = 128; img[t * 3 + 1] = 128; img[t * 3 + 2] = 255;
    status[t] = 0;
}

// (the pragma is per function body: these are inlined into a kernel that must not contract either)
__device__ __forceinline__ double ddot3(const double a[3], const double b[3]) {
#pragma clang fp contract(off)
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2];
}
// v / |v|; false (v untouched) when the squared length is 0 or not finite: normalize3 of s3d_render_pbr.hip in float64
__device__ __forceinline__ bool dnormalize3(double v[3]) {
#pragma clang fp contract(off)
    const double l2 = ddot3(v, v);
    if (!(l2 > 0.0 && l2 < double(INFINITY))) return false;
    const double l = sqrt(l2);
    v[0] = v[0] / l; v[1] = v[1] / l; v[2] = v[2] / l;
    return true;
}
__device__ __forceinline__ void dcross3(const double a[3], const double b[3], double c[3]) {
#pragma clang fp contract(off)
    c[0] = a[1] * b[2] - a[2] * b[1]; c[1] = a[2] * b[0] - a[0] * b[2]; c[2] = a[0] * b[1] - a[1] * b[0];
}

// One thread per covered texel i (texel idx[i], all different): the unit gradient g^ = grad[i] / |grad[i]| in the tangent frame of
// s3d_pbr_shade on the texel's face, as the bytes that shader decodes.  Face and barycentrics are the float32 expressions of
// k_texel_positions; everything after them is float64 with one rounding per operation (no contraction: a NumPy float64
// restatement takes every branch the same way) — the kernel waits on its gathers, the arithmetic is free.
// status: 0 not written (index outside the atlas, no chart, a bad vertex index), 1 encoded, 2 no gradient direction, 3 no frame
// (a face without area or without tangent), 4 encoded around the face normal because the base normal was unusable.
__global__ void __launch_bounds__(kTexThreads) k_normal_texels(const float* __restrict__ grad, const long long* __restrict__ idx, long long N,
                                                               const float* __restrict__ verts, long long nv, const int* __restrict__ tris,
                                                               const int* __restrict__ corner0, long long F, int T, int n, int c,
                                                               const float* __restrict__ base, const float* __restrict__ tangents,
                                                               unsigned char* __restrict__ img, unsigned char* __restrict__ status) {
#pragma clang fp contract(off)
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const long long p = idx[i];
    if (p < 0 || p >= (long long)T * T) return;
    // ---- 1: the face and the barycentrics of the texel centre, as in k_texel_positions
    const int x = int(p % T), y = int(p / T);
    const int col = x / c, row = y / c;
    if (col >= n || row >= n) return;
    const int lx = x - col * c, ly = y - row * c;
    const long long cell = (long long)row * n + col;
    long long k;
    int u, v;
    if (lx >= 1 && ly >= 1 && lx + ly <= c - 4) { k = 2 * cell; u = lx; v = ly; }
    else if (lx <= c - 2 && ly <= c - 2 && lx + ly >= c + 2) { k = 2 * cell + 1; u = c - 1 - lx; v = c - 1 - ly; }
    else return;
    if (k >= F) return;
    const int r = min(2, max(0, corner0[k]));
    int vi[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        vi[j] = tris[k * 3 + (r + j) % 3];
        if (vi[j] < 0 || vi[j] >= nv) return;
    }
    const float L = float(c - 5);
    const float b1f = __fdiv_rn(float(u) - 0.5f, L), b2f = __fdiv_rn(float(v) - 0.5f, L), b0f = 1.0f - b1f - b2f;
    const double b0 = b0f, b1 = b1f, b2 = b2f;
    unsigned char out[3] = {128, 128, 255};
    unsigned char st = 1;
    do {
        // ---- 2: the unit gradient
        const float gf[3] = {grad[i * 3], grad[i * 3 + 1], grad[i * 3 + 2]};
        double g[3] = {double(gf[0]), double(gf[1]), double(gf[2])};
        const bool g_finite = fabsf(gf[0]) < INFINITY && fabsf(gf[1]) < INFINITY && fabsf(gf[2]) < INFINITY;      // (a NaN compares false)
        if (!g_finite || ddot3(g, g) < 1e-20) { st = 2; break; }
        dnormalize3(g);
        // ---- 3, 4: the face normal, turned to the gradient's side
        double P[3][3];
#pragma unroll
        for (int j = 0; j < 3; ++j)
#pragma unroll
            for (int a = 0; a < 3; ++a) P[j][a] = double(verts[(long long)vi[j] * 3 + a]);
        const double e1[3] = {P[1][0] - P[0][0], P[1][1] - P[0][1], P[1][2] - P[0][2]};
        const double e2[3] = {P[2][0] - P[0][0], P[2][1] - P[0][1], P[2][2] - P[0][2]};
        double Nf[3];
        dcross3(e1, e2, Nf);
        if (!dnormalize3(Nf)) { st = 3; break; }
        const double s = ddot3(Nf, g) >= 0.0 ? 1.0 : -1.0;
        Nf[0] = s * Nf[0]; Nf[1] = s * Nf[1]; Nf[2] = s * Nf[2];
        // ---- 5: the base normal: the mix of the corners' normals, unless it is unusable (the smooth-normal rule of s3d_pbr_shade)
        double Nb[3] = {Nf[0], Nf[1], Nf[2]};
        bool smooth = false;
        if (base) {
            const float* n0 = base + (long long)vi[0] * 3;
            const float* n1 = base + (long long)vi[1] * 3;
            const float* n2 = base + (long long)vi[2] * 3;
            const bool any_zero = (n0[0] == 0.0f && n0[1] == 0.0f && n0[2] == 0.0f) || (n1[0] == 0.0f && n1[1] == 0.0f && n1[2] == 0.0f) ||
                                  (n2[0] == 0.0f && n2[1] == 0.0f && n2[2] == 0.0f);
            double mix[3];
#pragma unroll
            for (int a = 0; a < 3; ++a) mix[a] = b0 * double(n0[a]) + b1 * double(n1[a]) + b2 * double(n2[a]);
            if (!any_zero && dnormalize3(mix)) {
                mix[0] = s * mix[0]; mix[1] = s * mix[1]; mix[2] = s * mix[2];
                if (ddot3(mix, Nf) > 0.0) { Nb[0] = mix[0]; Nb[1] = mix[1]; Nb[2] = mix[2]; smooth = true; }
            }
        }
        // ---- 6: the face's tangent frame made orthonormal around the base normal
        const float* tg = tangents + k * 6;
        double Tp[3] = {double(tg[0]), double(tg[1]), double(tg[2])};
        const double B[3] = {double(tg[3]), double(tg[4]), double(tg[5])};
        if (tg[0] == 0.0f && tg[1] == 0.0f && tg[2] == 0.0f && tg[3] == 0.0f && tg[4] == 0.0f && tg[5] == 0.0f) { st = 3; break; }
        const double nt = ddot3(Nb, Tp);
#pragma unroll
        for (int a = 0; a < 3; ++a) Tp[a] = Tp[a] - Nb[a] * nt;
        if (!dnormalize3(Tp)) { st = 3; break; }
        double Bp[3];
        dcross3(Nb, Tp, Bp);
        const double sg = ddot3(Bp, B) < 0.0 ? -1.0 : 1.0;
        Bp[0] = sg * Bp[0]; Bp[1] = sg * Bp[1]; Bp[2] = sg * Bp[2];
        // ---- 7: the bytes
        const double tc[3] = {ddot3(g, Tp), ddot3(g, Bp), ddot3(g, Nb)};
#pragma unroll
        for (int a = 0; a < 3; ++a) out[a] = (unsigned char)int(floor(fmin(fmax((tc[a] + 1.0) * 127.5, 0.0), 255.0) + 0.5));
        if (!smooth) st = 4;
    } while (false);
    if (st == 2 || st == 3) { out[0] = 128; out[1] = 128; out[2] = 255; }
    img[p * 3] = out[0]; img[p * 3 + 1] = out[1]; img[p * 3 + 2] = out[2];
    status[p] = st;
}

// out = img where the mask is on; an uncovered texel takes the texel of its FIRST covered neighbour inside the atlas, in the order
// below (edge neighbours before corner neighbours), whole — all channels from the same texel, which the per-channel maximum of
// k_tex_dilate does not give —; img itself where no neighbour is covered
__global__ void __launch_bounds__(kTexThreads) k_tex_dilate_nearest(const unsigned char* __restrict__ q, const int* __restrict__ face_id, int T,
                                                                    int C, unsigned char* __restrict__ out) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (long long)T * T * C) return;
    const long long px = t / C;
    const int ch = int(t - px * C);
    long long src = px;
    if (face_id[px] < 0) {
        const int x = int(px % T), y = int(px / T);
        const int dx[8] = {0, -1, 1, 0, -1, 1, -1, 1}, dy[8] = {-1, 0, 0, 1, -1, -1, 1, 1};
        bool found = false;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int xx = x + dx[j], yy = y + dy[j];
            if (found || xx < 0 || xx >= T || yy < 0 || yy >= T) continue;
            const long long q2 = (long long)yy * T + xx;
            if (face_id[q2] >= 0) { src = q2; found = true; }
        }
    }
    out[t] = q[src * C + ch];
}

}  // namespace s3d

using namespace s3d;

extern "C" {

int s3d_mesh_cluster_keys(const float* verts, int64_t n_verts, const float origin[3], float cell, const int dims[3], int64_t* keys,
                          void* stream) {
    S3D_CHECK(origin && dims && (n_verts == 0 || (verts && keys)), S3D_ERR_INVALID, "mesh_cluster_keys: null argument");
    S3D_CHECK(n_verts >= 0 && cell > 0.0f && dims[0] >= 1 && dims[1] >= 1 && dims[2] >= 1, S3D_ERR_INVALID,
              "mesh_cluster_keys: cell side %g, grid %d x %d x %d", double(cell), dims[0], dims[1], dims[2]);
    S3D_CHECK((long long)dims[0] * dims[1] < (1LL << 42) && (long long)dims[0] * dims[1] * (long long)dims[2] < (1LL << 62), S3D_ERR_UNSUPPORTED,
              "mesh_cluster_keys: grid too large for 64-bit cell keys");
    if (!n_verts) return 0;
    hipLaunchKernelGGL(k_cluster_keys, dim3(tex_blocks(n_verts)), dim3(kTexThreads), 0, static_cast<hipStream_t>(stream), verts,
                       (long long)n_verts, origin[0], origin[1], origin[2], cell, dims[0], dims[1], dims[2], reinterpret_cast<long long*>(keys));
    S3D_HIP(hipGetLastError());
    return 0;
}

int s3d_mesh_cluster_means(const float* vals, int channels, const int64_t* order, const int64_t* seg, int64_t n_clusters, int64_t n_verts,
                           float* out, void* stream) {
    S3D_CHECK(n_clusters >= 0 && n_verts >= 0 && channels >= 1, S3D_ERR_INVALID, "mesh_cluster_means: bad sizes");
    S3D_CHECK(n_clusters == 0 || (vals && order && seg && out), S3D_ERR_INVALID, "mesh_cluster_means: null argument");
    if (!n_clusters) return 0;
    hipLaunchKernelGGL(k_cluster_means, dim3(tex_blocks(n_clusters * channels)), dim3(kTexThreads), 0, static_cast<hipStream_t>(stream), vals,
                       channels, reinterpret_cast<const long long*>(order), reinterpret_cast<const long long*>(seg), (long long)n_clusters,
                       (long long)n_verts, out);
    S3D_HIP(hipGetLastError());
    return 0;
}

int s3d_mesh_remap_faces(const int32_t* tris, int64_t n_tris, const int32_t* vmap, int64_t n_verts, int64_t n_clusters, int32_t* out_tris,
                         int64_t* face_keys, void* stream) {
    S3D_CHECK(n_tris >= 0 && n_verts >= 0 && n_clusters >= 0, S3D_ERR_INVALID, "mesh_remap_faces: bad sizes");
    S3D_CHECK(n_tris == 0 || (tris && vmap && out_tris && face_keys), S3D_ERR_INVALID, "mesh_remap_faces: null argument");
    S3D_CHECK(n_clusters <= (1LL << 20), S3D_ERR_UNSUPPORTED, "mesh_remap_faces: %lld clusters do not fit a 64-bit face key (2^20 at most)",
              (long long)n_clusters);
    if (!n_tris) return 0;
    hipLaunchKernelGGL(k_remap_faces, dim3(tex_blocks(n_tris)), dim3(kTexThreads), 0, static_cast<hipStream_t>(stream), tris, (long long)n_tris,
                       vmap, (long long)n_verts, (long long)n_clusters, out_tris, reinterpret_cast<long long*>(face_keys));
    S3D_HIP(hipGetLastError());
    return 0;
}

int s3d_tex_face_corner0(const float* verts, int64_t n_verts, const int32_t* tris, int64_t n_faces, int32_t* corner0, void* stream) {
    S3D_CHECK(n_faces >= 0 && n_verts >= 0, S3D_ERR_INVALID, "tex_face_corner0: bad sizes");
    S3D_CHECK(n_faces == 0 || (verts && tris && corner0), S3D_ERR_INVALID, "tex_face_corner0: null argument");
    if (!n_faces) return 0;
    hipLaunchKernelGGL(k_face_corner0, dim3(tex_blocks(n_faces)), dim3(kTexThreads), 0, static_cast<hipStream_t>(stream), verts, tris,
                       (long long)n_faces, (long long)n_verts, corner0);
    S3D_HIP(hipGetLastError());
    return 0;
}

int s3d_tex_texel_positions(const float* verts, int64_t n_verts, const int32_t* tris, const int32_t* corner0, int64_t n_faces, int texreso,
                            int cells_per_row, int cell, int32_t* face_id, float* pos, void* stream) {
    S3D_CHECK(face_id && pos && (n_faces == 0 || (verts && tris && corner0)), S3D_ERR_INVALID, "tex_texel_positions: null argument");
    S3D_CHECK(n_faces >= 0 && n_verts >= 0 && texreso >= 1 && texreso <= 16384, S3D_ERR_INVALID, "tex_texel_positions: bad sizes");
    S3D_CHECK(cell >= 8 && cells_per_row >= 1 && (long long)cells_per_row * cell <= texreso, S3D_ERR_INVALID,
              "tex_texel_positions: %d cells of %d texels per row in a %d texel atlas", cells_per_row, cell, texreso);
    S3D_CHECK(2LL * cells_per_row * cells_per_row >= n_faces, S3D_ERR_INVALID, "tex_texel_positions: %lld faces, %d x %d cells of two",
              (long long)n_faces, cells_per_row, cells_per_row);
    hipLaunchKernelGGL(k_texel_positions, dim3(tex_blocks((long long)texreso * texreso)), dim3(kTexThreads), 0, static_cast<hipStream_t>(stream),
                       verts, tris, corner0, (long long)n_faces, (long long)n_verts, texreso, cells_per_row, cell, face_id, pos);
    S3D_HIP(hipGetLastError());
    return 0;
}

int s3d_tex_quantize(const float* colors, const int64_t* texel_index, int64_t n, int channels, int texreso, uint8_t* image, void* stream) {
    S3D_CHECK(image && (n == 0 || (colors && texel_index)), S3D_ERR_INVALID, "tex_quantize: null argument");
    S3D_CHECK(n >= 0 && channels >= 1 && texreso >= 1 && texreso <= 16384, S3D_ERR_INVALID, "tex_quantize: bad sizes");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const long long TT = (long long)texreso * texreso;
    S3D_HIP(hipMemsetAsync(image, 0, size_t(TT) * channels, st));
    if (!n) return 0;
    hipLaunchKernelGGL(k_tex_quantize, dim3(tex_blocks(n * channels)), dim3(kTexThreads), 0, st, colors,
                       reinterpret_cast<const long long*>(texel_index), (long long)n, channels, TT, image);
    S3D_HIP(hipGetLastError());
    return 0;
}

int s3d_tex_dilate(const uint8_t* image, const int32_t* face_id, int texreso, int channels, uint8_t* out, void* stream) {
    S3D_CHECK(image && face_id && out && image != out, S3D_ERR_INVALID, "tex_dilate: null or aliased argument");
    S3D_CHECK(channels >= 1 && texreso >= 1 && texreso <= 16384, S3D_ERR_INVALID, "tex_dilate: bad sizes");
    hipLaunchKernelGGL(k_tex_dilate, dim3(tex_blocks((long long)texreso * texreso * channels)), dim3(kTexThreads), 0,
                       static_cast<hipStream_t>(stream), image, face_id, texreso, channels, out);
    S3D_HIP(hipGetLastError());
    return 0;
}

int s3d_tex_normal_texels(const float* grad, const int64_t* texel_index, int64_t n, const float* verts, int64_t n_verts, const int32_t* tris,
                          const int32_t* corner0, int64_t n_faces, int texreso, int cells_per_row, int cell, const float* base_normals,
                          const float* tangents, uint8_t* image, uint8_t* status, void* stream) {
    S3D_CHECK(image && status && (n == 0 || (grad && texel_index)), S3D_ERR_INVALID, "tex_normal_texels: null argument");
    S3D_CHECK(n_faces == 0 || (verts && tris && corner0 && tangents), S3D_ERR_INVALID, "tex_normal_texels: null mesh argument");
    S3D_CHECK(n >= 0 && n_faces >= 0 && n_verts >= 0 && texreso >= 1 && texreso <= 16384, S3D_ERR_INVALID, "tex_normal_texels: bad sizes");
    S3D_CHECK(cell >= 8 && cells_per_row >= 1 && (long long)cells_per_row * cell <= texreso, S3D_ERR_INVALID,
              "tex_normal_texels: %d cells of %d texels per row in a %d texel atlas", cells_per_row, cell, texreso);
    S3D_CHECK(2LL * cells_per_row * cells_per_row >= n_faces, S3D_ERR_INVALID, "tex_normal_texels: %lld faces, %d x %d cells of two",
              (long long)n_faces, cells_per_row, cells_per_row);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const long long TT = (long long)texreso * texreso;
    hipLaunchKernelGGL(k_normal_fill, dim3(tex_blocks(TT)), dim3(kTexThreads), 0, st, TT, image, status);
    S3D_HIP(hipGetLastError());
    if (!n || !n_faces) return 0;
    hipLaunchKernelGGL(k_normal_texels, dim3(tex_blocks(n)), dim3(kTexThreads), 0, st, grad, reinterpret_cast<const long long*>(texel_index),
                       (long long)n, verts, (long long)n_verts, tris, corner0, (long long)n_faces, texreso, cells_per_row, cell, base_normals,
                       tangents, image, status);
    S3D_HIP(hipGetLastError());
    return 0;
}

int s3d_tex_dilate_nearest(const uint8_t* image, const int32_t* face_id, int texreso, int channels, uint8_t* out, void* stream) {
    S3D_CHECK(image && face_id && out && image != out, S3D_ERR_INVALID, "tex_dilate_nearest: null or aliased argument");
    S3D_CHECK(channels >= 1 && texreso >= 1 && texreso <= 16384, S3D_ERR_INVALID, "tex_dilate_nearest: bad sizes");
    hipLaunchKernelGGL(k_tex_dilate_nearest, dim3(tex_blocks((long long)texreso * texreso * channels)), dim3(kTexThreads), 0,
                       static_cast<hipStream_t>(stream), image, face_id, texreso, channels, out);
    S3D_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
