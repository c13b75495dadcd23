// s3d_qem.hip — quadric-error edge collapse (Garland & Heckbert 1997) as parallel rounds of independent collapses: the second
// decimator of the textured mesh export (isosurface.simplify_mesh_quadric).  Sorting, unique and compaction stay with
// the caller (torch); the arithmetic of a round is here, one thread per vertex / edge / face:
//   quadrics   Q_v = sum over the faces at v, in ascending face index, of area * p p^T (p the unit plane), double accumulator
//   cost       per edge: Q_e = Q_u + Q_v, the target (3x3 solve in double, else the cheapest of midpoint, u, v), the fp32 cost
//   valid      per edge: two faces, no frozen endpoint, the link condition, no flipped or collapsed face around it
//   select     an independent set of valid edges by integer minima over closed vertex neighbourhoods
//   apply      move u, add the quadrics, interpolate the attributes, point v at u; then the faces through that map
// Positions are fp32; every quadric is the upper triangle of a symmetric 4x4 matrix as 10 doubles (xx xy xz xw yy yz yw zz zw ww).
// No floating-point atomics: the only atomic is an integer minimum, whose result does not depend on the order, so the same
// input gives the same bits on every run.
#include "s3d_common.h"

namespace s3d {

constexpr int kQemThreads = 256;
static inline unsigned qem_blocks(long long n) { return (unsigned)((n + kQemThreads - 1) / kQemThreads); }

constexpr double kQemDetRel = 1e-6;        // the 3x3 system is solved where |det A| > kQemDetRel * (trace A / 3)^3
constexpr double kQemReach = 2.0;          // ... and the solution lies within kQemReach edge lengths of the midpoint
constexpr double kQemTieRel = 1e-10;       // an endpoint beats the midpoint only by more than kQemTieRel * trace A * (1 + |mid|^2)
constexpr double kQemFlipCos = 0.2;        // a face around a collapse keeps cos(old normal, new normal) above this
constexpr unsigned long long kQemNoKey = 0x7fffffffffffffffULL;

constexpr int QEM_TWO_FACES = 1, QEM_NOT_FROZEN = 2, QEM_LINK = 4, QEM_NO_FLIP = 8, QEM_VALID = 15;

struct D3 { double x, y, z; };
__device__ __forceinline__ D3 ld3(const float* __restrict__ v, long long i) { return {double(v[i * 3]), double(v[i * 3 + 1]), double(v[i * 3 + 2])}; }
__device__ __forceinline__ D3 sub(D3 a, D3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ D3 cross(D3 a, D3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__device__ __forceinline__ double dot(D3 a, D3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }

// ------------------------------------------------------------------ initial quadrics
// One thread per vertex walks its segment of the (vertex, face) list, which the caller sorted: ascending face index.
__global__ void __launch_bounds__(kQemThreads) k_qem_quadrics(const float* __restrict__ verts, long long nv, const int* __restrict__ tris,
                                                              long long nt, const long long* __restrict__ vf_off,
                                                              const int* __restrict__ vf_face, double* __restrict__ Q) {
    const long long v = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= nv) return;
    double q0 = 0, q1 = 0, q2 = 0, q3 = 0, q4 = 0, q5 = 0, q6 = 0, q7 = 0, q8 = 0, q9 = 0;
    const long long b = max(0LL, vf_off[v]), e = min(3 * nt, vf_off[v + 1]);
    for (long long j = b; j < e; ++j) {
        const long long f = vf_face[j];
        if (f < 0 || f >= nt) continue;
        const int ia = tris[f * 3], ib = tris[f * 3 + 1], ic = tris[f * 3 + 2];
        if (ia < 0 || ia >= nv || ib < 0 || ib >= nv || ic < 0 || ic >= nv) continue;
        const D3 a = ld3(verts, ia);
        const D3 n = cross(sub(ld3(verts, ib), a), sub(ld3(verts, ic), a));
        const double len = sqrt(dot(n, n));
        if (!(len > 0.0)) continue;                                  // a face without area has no plane
        const double px = n.x / len, py = n.y / len, pz = n.z / len, pw = -(px * a.x + py * a.y + pz * a.z), w = 0.5 * len;
        q0 += w * px * px; q1 += w * px * py; q2 += w * px * pz; q3 += w * px * pw;
        q4 += w * py * py; q5 += w * py * pz; q6 += w * py * pw;
        q7 += w * pz * pz; q8 += w * pz * pw; q9 += w * pw * pw;
    }
    double* o = Q + v * 10;
    o[0] = q0; o[1] = q1; o[2] = q2; o[3] = q3; o[4] = q4; o[5] = q5; o[6] = q6; o[7] = q7; o[8] = q8; o[9] = q9;
}

// ------------------------------------------------------------------ per-edge cost and target
struct Quadric { double xx, xy, xz, xw, yy, yz, yw, zz, zw, ww; };
__device__ __forceinline__ double qem_eval(const Quadric& q, D3 p) {
    return p.x * (q.xx * p.x + 2.0 * (q.xy * p.y + q.xz * p.z + q.xw)) + p.y * (q.yy * p.y + 2.0 * (q.yz * p.z + q.yw)) +
           p.z * (q.zz * p.z + 2.0 * q.zw) + q.ww;
}

// The two quadrics are added while they are loaded, so a thread holds ten doubles of quadric, six cofactors and three points.
__global__ void __launch_bounds__(kQemThreads) k_qem_edge_cost(const float* __restrict__ verts, long long nv, const double* __restrict__ Q,
                                                               const int* __restrict__ eu, const int* __restrict__ ev, long long ne,
                                                               float* __restrict__ target, float* __restrict__ cost) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ne) return;
    const int u = eu[i], v = ev[i];
    if (u < 0 || u >= nv || v < 0 || v >= nv) {
        target[i * 3] = 0.0f; target[i * 3 + 1] = 0.0f; target[i * 3 + 2] = 0.0f; cost[i] = 0.0f;
        return;
    }
    const double* a = Q + (long long)u * 10;
    const double* b = Q + (long long)v * 10;
    const Quadric q = {a[0] + b[0], a[1] + b[1], a[2] + b[2], a[3] + b[3], a[4] + b[4], a[5] + b[5], a[6] + b[6], a[7] + b[7], a[8] + b[8], a[9] + b[9]};
    const D3 pu = ld3(verts, u), pv = ld3(verts, v);
    const D3 mid = {0.5 * (pu.x + pv.x), 0.5 * (pu.y + pv.y), 0.5 * (pu.z + pv.z)};
    const D3 d = sub(pv, pu);
    const double len2 = dot(d, d);
    // cofactors of the symmetric 3x3 block A; A x = -(xw, yw, zw) minimises x^T A x + 2 (xw, yw, zw) x + ww
    const double c00 = q.yy * q.zz - q.yz * q.yz, c01 = q.xz * q.yz - q.xy * q.zz, c02 = q.xy * q.yz - q.xz * q.yy;
    const double c11 = q.xx * q.zz - q.xz * q.xz, c12 = q.xy * q.xz - q.xx * q.yz, c22 = q.xx * q.yy - q.xy * q.xy;
    const double det = q.xx * c00 + q.xy * c01 + q.xz * c02;
    const double tr = (q.xx + q.yy + q.zz) * (1.0 / 3.0);
    D3 best = mid;
    bool solved = false;
    if (fabs(det) > kQemDetRel * tr * tr * tr) {
        const D3 x = {-(c00 * q.xw + c01 * q.yw + c02 * q.zw) / det, -(c01 * q.xw + c11 * q.yw + c12 * q.zw) / det,
                      -(c02 * q.xw + c12 * q.yw + c22 * q.zw) / det};
        const D3 r = sub(x, mid);
        if (dot(r, r) <= kQemReach * kQemReach * len2) { best = x; solved = true; }
    }
    double c = qem_eval(q, best);
    if (!solved) {
        const double tol = kQemTieRel * 3.0 * tr * (1.0 + dot(mid, mid));
        const double cu = qem_eval(q, pu), cv = qem_eval(q, pv);
        if (cu < c - tol) { c = cu; best = pu; }
        if (cv < c - tol) { c = cv; best = pv; }
    }
    target[i * 3] = float(best.x); target[i * 3 + 1] = float(best.y); target[i * 3 + 2] = float(best.z);
    cost[i] = float(fmax(c, 0.0));
}

// ------------------------------------------------------------------ per-edge validity
// frozen[w] = 1 for both endpoints of every edge whose face count is not 2 (every writer stores the same byte)
__global__ void __launch_bounds__(kQemThreads) k_qem_frozen(const int* __restrict__ eu, const int* __restrict__ ev, const int* __restrict__ ecount,
                                                            long long ne, long long nv, unsigned char* __restrict__ frozen) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ne || ecount[i] == 2) return;
    const int u = eu[i], v = ev[i];
    if (u >= 0 && u < nv) frozen[u] = 1;
    if (v >= 0 && v < nv) frozen[v] = 1;
}

// the faces at vertex `w`, except those that hold both u and v: does the move of w to `x` keep every normal on its side?
// `pair` counts the faces at w that hold both w1 and w2 (the link's common edge, see below)
__device__ __forceinline__ bool qem_fan_ok(const float* __restrict__ verts, long long nv, const int* __restrict__ tris, long long nt,
                                           const long long* __restrict__ vf_off, const int* __restrict__ vf_face, int w, int other, D3 x,
                                           int w1, int w2, int& pair) {
    bool ok = true;
    const long long b = max(0LL, vf_off[w]), e = min(3 * nt, vf_off[w + 1]);
    for (long long j = b; j < e; ++j) {
        const long long f = vf_face[j];
        if (f < 0 || f >= nt) { ok = false; continue; }
        const int i0 = tris[f * 3], i1 = tris[f * 3 + 1], i2 = tris[f * 3 + 2];
        if (i0 < 0 || i0 >= nv || i1 < 0 || i1 >= nv || i2 < 0 || i2 >= nv) { ok = false; continue; }
        if (i0 == other || i1 == other || i2 == other) continue;                     // this face goes away with the edge
        pair += int((i0 == w1 || i1 == w1 || i2 == w1) && (i0 == w2 || i1 == w2 || i2 == w2));
        const D3 p0 = ld3(verts, i0), p1 = ld3(verts, i1), p2 = ld3(verts, i2);
        const D3 n0 = cross(sub(p1, p0), sub(p2, p0));
        const D3 r0 = i0 == w ? x : p0, r1 = i1 == w ? x : p1, r2 = i2 == w ? x : p2;
        const D3 n1 = cross(sub(r1, r0), sub(r2, r0));
        const double l1 = dot(n1, n1);
        ok = ok && l1 > 0.0 && dot(n0, n1) > kQemFlipCos * sqrt(dot(n0, n0) * l1);
    }
    return ok;
}

// flags[e]: QEM_TWO_FACES | QEM_NOT_FROZEN | QEM_LINK | QEM_NO_FLIP, each bit on its own so that a restatement can hold every test
// apart.  The link condition Lk(u) ∩ Lk(v) = Lk(uv) on a surface: u and v have exactly two common neighbours w1, w2 (a merge of
// the two sorted neighbour lists), and the edge w1 w2 does not lie in both links (the faces u w1 w2 and v w1 w2 do not both exist:
// they would become one face twice — the tetrahedron).
__global__ void __launch_bounds__(kQemThreads) k_qem_edge_valid(const float* __restrict__ verts, long long nv, const int* __restrict__ tris,
                                                                long long nt, const int* __restrict__ eu, const int* __restrict__ ev,
                                                                const int* __restrict__ ecount, long long ne,
                                                                const unsigned char* __restrict__ frozen, const long long* __restrict__ nbr_off,
                                                                const int* __restrict__ nbr, long long n_nbr, const long long* __restrict__ vf_off,
                                                                const int* __restrict__ vf_face, const float* __restrict__ target,
                                                                int* __restrict__ flags) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ne) return;
    const int u = eu[i], v = ev[i];
    if (u < 0 || u >= nv || v < 0 || v >= nv || u == v) { flags[i] = 0; return; }
    int fl = 0;
    if (ecount[i] == 2) fl |= QEM_TWO_FACES;
    if (!frozen[u] && !frozen[v]) fl |= QEM_NOT_FROZEN;
    long long a = max(0LL, nbr_off[u]), b = max(0LL, nbr_off[v]);
    const long long ae = min(n_nbr, nbr_off[u + 1]), be = min(n_nbr, nbr_off[v + 1]);
    int common = 0, w1 = -1, w2 = -1;
    while (a < ae && b < be) {
        const int x = nbr[a], y = nbr[b];
        if (x == y) {
            if (common == 0) w1 = x; else if (common == 1) w2 = x;
            ++common; ++a; ++b;
        } else if (x < y) ++a;
        else ++b;
    }
    const D3 x = ld3(target, i);
    int pair_u = 0, pair_v = 0;
    const bool fan_u = qem_fan_ok(verts, nv, tris, nt, vf_off, vf_face, u, v, x, w1, w2, pair_u);
    const bool fan_v = qem_fan_ok(verts, nv, tris, nt, vf_off, vf_face, v, u, x, w1, w2, pair_v);
    if (common == 2 && !(pair_u > 0 && pair_v > 0)) fl |= QEM_LINK;
    if (fan_u && fan_v) fl |= QEM_NO_FLIP;
    flags[i] = fl;
}

// ------------------------------------------------------------------ an independent set of collapses
// key(e) = (bits of the fp32 cost << 32) | mix(e): costs are >= 0, so the order of the keys is the order of (cost, mix(edge index)),
// every key is its own (mix is a bijection of the 32-bit integers), and all lie below kQemNoKey.  The index is mixed because equal
// costs are the rule on flat patches (all 0) and edge indices ascend along the surface: with the plain index a round found a
// handful of local minima there (1057 rounds for 10 240 faces of a box, 8 collapses in the first; 65 rounds with the mixed
// index, profiles/qem.txt).  m1[w] = min key of the valid edges at w; m2[w] = min of m1 over w and its
// neighbours; edge (u, v) is selected iff key == m2[u] == m2[v].
// Why the selected collapses are independent: a selected e = (u, v) has the smallest key among ALL valid edges with an endpoint in
// N[u] ∪ N[v] (the closed neighbourhoods).  Let a second selected edge e' have an endpoint w' with w' = w or w' adjacent to w for an
// endpoint w of e.  Then w' lies in N[w], so key(e) <= key(e'), and w lies in N[w'], so key(e') <= key(e): the keys are equal, and
// e' = e.  So no endpoint of one selected edge equals or neighbours an endpoint of another; a face holds a vertex of at most one
// collapse (two vertices of one face are neighbours); and everything the validity test of e read — the neighbour lists of u and v,
// the faces at u and v and the positions of their corners — is changed by no other collapse of the round.  The tests made on the
// mesh before the round are therefore exact for the whole round.
__device__ __forceinline__ unsigned qem_mix(unsigned i) {              // multiply by odd, xor-shift right: each step is invertible
    i *= 0x9E3779B1u; i ^= i >> 16; i *= 0x85EBCA6Bu; i ^= i >> 13;
    return i;
}

__global__ void __launch_bounds__(kQemThreads) k_qem_fill_keys(unsigned long long* __restrict__ m, long long n) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) m[i] = kQemNoKey;
}

__global__ void __launch_bounds__(kQemThreads) k_qem_vertex_min(const int* __restrict__ eu, const int* __restrict__ ev, const float* __restrict__ cost,
                                                                const int* __restrict__ flags, long long ne, long long nv,
                                                                unsigned long long* __restrict__ keys, unsigned long long* __restrict__ m1) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ne) return;
    const unsigned long long key = ((unsigned long long)(__float_as_uint(fmaxf(cost[i], 0.0f)) & 0x7fffffffu) << 32) | (unsigned long long)qem_mix((unsigned)i);
    keys[i] = key;
    const int u = eu[i], v = ev[i];
    if (flags[i] != QEM_VALID || u < 0 || u >= nv || v < 0 || v >= nv) return;
    atomicMin(m1 + u, key);
    atomicMin(m1 + v, key);
}

__global__ void __launch_bounds__(kQemThreads) k_qem_neighbour_min(const unsigned long long* __restrict__ m1, const long long* __restrict__ nbr_off,
                                                                   const int* __restrict__ nbr, long long n_nbr, long long nv,
                                                                   unsigned long long* __restrict__ m2) {
    const long long w = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= nv) return;
    unsigned long long m = m1[w];
    const long long b = max(0LL, nbr_off[w]), e = min(n_nbr, nbr_off[w + 1]);
    for (long long j = b; j < e; ++j) {
        const int x = nbr[j];
        if (x >= 0 && x < nv) m = min(m, m1[x]);
    }
    m2[w] = m;
}

__global__ void __launch_bounds__(kQemThreads) k_qem_select(const int* __restrict__ eu, const int* __restrict__ ev, const int* __restrict__ flags,
                                                            const unsigned long long* __restrict__ keys, const unsigned long long* __restrict__ m2,
                                                            long long ne, long long nv, unsigned char* __restrict__ selected) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ne) return;
    const int u = eu[i], v = ev[i];
    const bool ok = flags[i] == QEM_VALID && u >= 0 && u < nv && v >= 0 && v < nv;
    selected[i] = (ok && keys[i] == m2[u] && keys[i] == m2[v]) ? 1 : 0;
}

// ------------------------------------------------------------------ apply
// One thread per chosen edge (their endpoints are pairwise different, see above): u moves to the target and takes both quadrics;
// the attributes are those of the point of the segment u v nearest to the target, a = (1 - t) a_u + t a_v with t in [0, 1], kept
// inside [min(a_u, a_v), max(a_u, a_v)] against the rounding of that sum; v points at u.
__global__ void __launch_bounds__(kQemThreads) k_qem_apply(const long long* __restrict__ chosen, long long ns, const int* __restrict__ eu,
                                                           const int* __restrict__ ev, long long ne, const float* __restrict__ target,
                                                           float* __restrict__ verts, long long nv, double* __restrict__ Q,
                                                           float* __restrict__ attrs, int A, int* __restrict__ vmap) {
    const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= ns) return;
    const long long i = chosen[k];
    if (i < 0 || i >= ne) return;
    const int u = eu[i], v = ev[i];
    if (u < 0 || u >= nv || v < 0 || v >= nv || u == v) return;
    const D3 pu = ld3(verts, u), pv = ld3(verts, v), x = ld3(target, i);
    const D3 d = sub(pv, pu);
    const double len2 = dot(d, d);
    const float t = len2 > 0.0 ? float(fmin(fmax(dot(sub(x, pu), d) / len2, 0.0), 1.0)) : 0.0f;
    for (int c = 0; c < A; ++c) {
        const float au = attrs[(long long)u * A + c], av = attrs[(long long)v * A + c];
        attrs[(long long)u * A + c] = fminf(fmaxf((1.0f - t) * au + t * av, fminf(au, av)), fmaxf(au, av));
    }
    verts[(long long)u * 3] = target[i * 3]; verts[(long long)u * 3 + 1] = target[i * 3 + 1]; verts[(long long)u * 3 + 2] = target[i * 3 + 2];
    double* qu = Q + (long long)u * 10;
    const double* qv = Q + (long long)v * 10;
#pragma unroll
    for (int c = 0; c < 10; ++c) qu[c] += qv[c];
    vmap[v] = u;
}

// out = vmap[tris]; keep[f] = 1 unless two of the three are now the same vertex
__global__ void __launch_bounds__(kQemThreads) k_qem_remap_faces(const int* __restrict__ tris, long long nt, const int* __restrict__ vmap, long long nv,
                                                                 int* __restrict__ out, unsigned char* __restrict__ keep) {
    const long long f = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= nt) return;
    const int ia = tris[f * 3], ib = tris[f * 3 + 1], ic = tris[f * 3 + 2];
    const bool ok = ia >= 0 && ia < nv && ib >= 0 && ib < nv && ic >= 0 && ic < nv;
    const int a = ok ? vmap[ia] : 0, b = ok ? vmap[ib] : 0, c = ok ? vmap[ic] : 0;
    out[f * 3] = a; out[f * 3 + 1] = b; out[f * 3 + 2] = c;
    keep[f] = (ok && a != b && b != c && a != c) ? 1 : 0;
}

}  // namespace s3d

using namespace s3d;

extern "C" {

int s3d_mesh_qem_quadrics(const float* verts, int64_t n_verts, const int32_t* tris, int64_t n_tris, const int64_t* vf_off,
                          const int32_t* vf_face, double* quadrics, void* stream) {
    S3D_CHECK(n_verts >= 0 && n_tris >= 0, S3D_ERR_INVALID, "mesh_qem_quadrics: bad sizes");
    S3D_CHECK(n_verts == 0 || (verts && vf_off && quadrics && (n_tris == 0 || (tris && vf_face))), S3D_ERR_INVALID,
              "mesh_qem_quadrics: null argument");
    if (!n_verts) return 0;
    hipLaunchKernelGGL(k_qem_quadrics, dim3(qem_blocks(n_verts)), dim3(kQemThreads), 0, static_cast<hipStream_t>(stream), verts,
                       (long long)n_verts, tris, (long long)n_tris, reinterpret_cast<const long long*>(vf_off), vf_face, quadrics);
    S3D_HIP(hipGetLastError());
    return 0;
}

int s3d_mesh_qem_edge_cost(const float* verts, int64_t n_verts, const double* quadrics, const int32_t* edge_u, const int32_t* edge_v,
                           int64_t n_edges, float* target, float* cost, void* stream) {
    S3D_CHECK(n_verts >= 0 && n_edges >= 0, S3D_ERR_INVALID, "mesh_qem_edge_cost: bad sizes");
    S3D_CHECK(n_edges == 0 || (verts && quadrics && edge_u && edge_v && target && cost), S3D_ERR_INVALID, "mesh_qem_edge_cost: null argument");
    if (!n_edges) return 0;
    hipLaunchKernelGGL(k_qem_edge_cost, dim3(qem_blocks(n_edges)), dim3(kQemThreads), 0, static_cast<hipStream_t>(stream), verts,
                       (long long)n_verts, quadrics, edge_u, edge_v, (long long)n_edges, target, cost);
    S3D_HIP(hipGetLastError());
    return 0;
}

int s3d_mesh_qem_edge_valid(const float* verts, int64_t n_verts, const int32_t* tris, int64_t n_tris, const int32_t* edge_u,
                            const int32_t* edge_v, const int32_t* edge_faces, int64_t n_edges, const int64_t* nbr_off, const int32_t* nbr,
                            int64_t n_nbr, const int64_t* vf_off, const int32_t* vf_face, const float* target, uint8_t* frozen, int32_t* flags,
                            void* stream) {
    S3D_CHECK(n_verts >= 0 && n_tris >= 0 && n_edges >= 0 && n_nbr >= 0, S3D_ERR_INVALID, "mesh_qem_edge_valid: bad sizes");
    S3D_CHECK(n_verts == 0 || frozen, S3D_ERR_INVALID, "mesh_qem_edge_valid: null argument");
    S3D_CHECK(n_edges == 0 || (verts && tris && edge_u && edge_v && edge_faces && nbr_off && nbr && vf_off && vf_face && target && flags),
              S3D_ERR_INVALID, "mesh_qem_edge_valid: null argument");
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (n_verts) S3D_HIP(hipMemsetAsync(frozen, 0, size_t(n_verts), st));
    if (!n_edges) return 0;
    hipLaunchKernelGGL(k_qem_frozen, dim3(qem_blocks(n_edges)), dim3(kQemThreads), 0, st, edge_u, edge_v, edge_faces, (long long)n_edges,
                       (long long)n_verts, frozen);
    hipLaunchKernelGGL(k_qem_edge_valid, dim3(qem_blocks(n_edges)), dim3(kQemThreads), 0, st, verts, (long long)n_verts, tris, (long long)n_tris,
                       edge_u, edge_v, edge_faces, (long long)n_edges, frozen, reinterpret_cast<const long long*>(nbr_off), nbr, (long long)n_nbr,
                       reinterpret_cast<const long long*>(vf_off), vf_face, target, flags);
    S3D_HIP(hipGetLastError());
    return 0;
}

int s3d_mesh_qem_select(const int32_t* edge_u, const int32_t* edge_v, const float* cost, const int32_t* flags, int64_t n_edges,
                        const int64_t* nbr_off, const int32_t* nbr, int64_t n_nbr, int64_t n_verts, int64_t* keys, int64_t* m1, int64_t* m2,
                        uint8_t* selected, void* stream) {
    S3D_CHECK(n_verts >= 0 && n_edges >= 0 && n_nbr >= 0, S3D_ERR_INVALID, "mesh_qem_select: bad sizes");
    S3D_CHECK(n_edges < (1LL << 32), S3D_ERR_UNSUPPORTED, "mesh_qem_select: %lld edges do not fit the 32 index bits of a key", (long long)n_edges);
    S3D_CHECK(n_edges == 0 || (edge_u && edge_v && cost && flags && nbr_off && nbr && keys && m1 && m2 && selected), S3D_ERR_INVALID,
              "mesh_qem_select: null argument");
    if (!n_edges || !n_verts) return 0;
    hipStream_t st = static_cast<hipStream_t>(stream);
    unsigned long long* k = reinterpret_cast<unsigned long long*>(keys);
    unsigned long long* a = reinterpret_cast<unsigned long long*>(m1);
    unsigned long long* b = reinterpret_cast<unsigned long long*>(m2);
    hipLaunchKernelGGL(k_qem_fill_keys, dim3(qem_blocks(n_verts)), dim3(kQemThreads), 0, st, a, (long long)n_verts);
    hipLaunchKernelGGL(k_qem_vertex_min, dim3(qem_blocks(n_edges)), dim3(kQemThreads), 0, st, edge_u, edge_v, cost, flags, (long long)n_edges,
                       (long long)n_verts, k, a);
    hipLaunchKernelGGL(k_qem_neighbour_min, dim3(qem_blocks(n_verts)), dim3(kQemThreads), 0, st, a, reinterpret_cast<const long long*>(nbr_off), nbr,
                       (long long)n_nbr, (long long)n_verts, b);
    hipLaunchKernelGGL(k_qem_select, dim3(qem_blocks(n_edges)), dim3(kQemThreads), 0, st, edge_u, edge_v, flags, k, b, (long long)n_edges,
                       (long long)n_verts, selected);
    S3D_HIP(hipGetLastError());
    return 0;
}

int s3d_mesh_qem_apply(const int64_t* chosen, int64_t n_chosen, const int32_t* edge_u, const int32_t* edge_v, int64_t n_edges,
                       const float* target, float* verts, int64_t n_verts, double* quadrics, float* attrs, int n_attr, int32_t* vmap,
                       void* stream) {
    S3D_CHECK(n_chosen >= 0 && n_edges >= 0 && n_verts >= 0 && n_attr >= 0, S3D_ERR_INVALID, "mesh_qem_apply: bad sizes");
    S3D_CHECK(n_chosen == 0 || (chosen && edge_u && edge_v && target && verts && quadrics && vmap && (n_attr == 0 || attrs)), S3D_ERR_INVALID,
              "mesh_qem_apply: null argument");
    if (!n_chosen) return 0;
    hipLaunchKernelGGL(k_qem_apply, dim3(qem_blocks(n_chosen)), dim3(kQemThreads), 0, static_cast<hipStream_t>(stream),
                       reinterpret_cast<const long long*>(chosen), (long long)n_chosen, edge_u, edge_v, (long long)n_edges, target, verts,
                       (long long)n_verts, quadrics, attrs, n_attr, vmap);
    S3D_HIP(hipGetLastError());
    return 0;
}

int s3d_mesh_qem_remap_faces(const int32_t* tris, int64_t n_tris, const int32_t* vmap, int64_t n_verts, int32_t* out_tris, uint8_t* keep,
                             void* stream) {
    S3D_CHECK(n_tris >= 0 && n_verts >= 0, S3D_ERR_INVALID, "mesh_qem_remap_faces: bad sizes");
    S3D_CHECK(n_tris == 0 || (tris && vmap && out_tris && keep), S3D_ERR_INVALID, "mesh_qem_remap_faces: null argument");
    if (!n_tris) return 0;
    hipLaunchKernelGGL(k_qem_remap_faces, dim3(qem_blocks(n_tris)), dim3(kQemThreads), 0, static_cast<hipStream_t>(stream), tris, (long long)n_tris,
                       vmap, (long long)n_verts, out_tris, keep);
    S3D_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
