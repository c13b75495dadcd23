// s3d_mc_sparse.hip — narrow-band iso-surface extraction: the mesh of s3d_mc.hip from the bricks the surface
// crosses, so that the decoder runs on O(N^2) samples of an N^3 grid and nothing of size N^3 but one brick table exists.
//
// Padded vertex space of the dense path (pad = 1): P = dims + 2, vertex p holds sample p - 1 or pad_value.  Brick b = vertices
// [b B, b B + B) per axis.  The caller keeps the pool [slot][B^3][stride] of the active bricks' samples; table[brick] = slot or -1.
//   k_mcs_seed       one thread per brick: do its eight lattice corners compare differently against iso
//   k_mcs_dilate     26-neighbourhood of the seed flags
//   k_mcs_newflag / scan / k_mcs_assign   slots for the newly marked bricks, ascending brick index (append-only)
//   k_mcs_pending    the unpadded sample coordinates of the new slots, in pool order
//   k_mcs_flags      one block per slot; the brick and its +1 apron staged in LDS (every sample is read up to 8 times).  Mode
//                    BOUNDARY marks the bricks around boundary cut edges; COUNT / EMIT count and append one 64-bit key per kept
//                    vertex (axis * NV + padded linear vertex index) and per cell with triangles (linear index * 8 + count)
//   hipcub::DeviceRadixSort::SortKeys on both lists -> the dense order; the keys are unique, so the sorted lists do not depend
//                    on the order the blocks appended them in
//   k_mcs_verts / k_mcs_tris   the expressions of k_mc_verts / k_mc_tris; a triangle finds its vertices by binary search
// Integer atomics only (counters, append cursors), plain idempotent stores for the marks: same input, same bits.
#include <hipcub/hipcub.hpp>

#include <algorithm>

#include "s3d_common.h"
#include "s3d_mc_tables.h"

namespace s3d {

__constant__ unsigned char d_mcs_edge[12][2];
__constant__ unsigned char d_mcs_edge_axis[12];
__constant__ unsigned char d_mcs_ntri[256];
__constant__ signed char d_mcs_tri[256][15];

struct McsGrid {
    const float* pool;         // [slot][B^3][stride], value in channel 0
    const int* table;          // [nb0][nb1][nb2]: slot or -1
    int stride;
    int X, Y, Z;               // samples
    int Px, Py, Pz;            // padded vertices
    int nbx, nby, nbz;
    int B, lb;                 // brick side and its log2
    float iso, pad_value;
};
enum { MCS_BOUNDARY = 0, MCS_COUNT = 1, MCS_EMIT = 2 };
// counters (unsigned long long): boundary cut edges, kept vertices, cells with triangles, the two append cursors
enum { CTR_BOUNDARY = 0, CTR_NV, CTR_NC, CTR_VCUR, CTR_CCUR, CTR_COUNT };

__device__ __forceinline__ long long mcs_brick_lin(const McsGrid& g, int bx, int by, int bz) {
    return ((long long)bx * g.nby + by) * g.nbz + bz;
}
__device__ __forceinline__ bool mcs_is_pad(const McsGrid& g, int x, int y, int z) {
    return x == 0 || y == 0 || z == 0 || x == g.Px - 1 || y == g.Py - 1 || z == g.Pz - 1;
}
// pool entry of padded vertex (x,y,z) in [0,P), or -1 where its brick is not active
__device__ __forceinline__ long long mcs_entry(const McsGrid& g, int x, int y, int z) {
    const int slot = g.table[mcs_brick_lin(g, x >> g.lb, y >> g.lb, z >> g.lb)];
    if (slot < 0) return -1;
    const int m = g.B - 1;
    return ((long long)slot << (3 * g.lb)) + ((((x & m) << g.lb) | (y & m)) << g.lb | (z & m));
}
// value of padded vertex (x,y,z) in [0,P): pad_value on the shell; a vertex of an inactive brick is never used for a decision and
// reads as pad_value only to stay inside the pool
__device__ __forceinline__ float mcs_value(const McsGrid& g, int x, int y, int z) {
    if (mcs_is_pad(g, x, y, z)) return g.pad_value;
    const long long e = mcs_entry(g, x, y, z);
    return e < 0 ? g.pad_value : g.pool[size_t(e) * g.stride];
}

__global__ __launch_bounds__(256) void k_mcs_seed(McsGrid g, const float* __restrict__ lattice, int ls, unsigned char* __restrict__ seed,
                                                  unsigned char* __restrict__ bsign) {
    const long long NB = (long long)g.nbx * g.nby * g.nbz;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= NB) return;
    const int bz = int(i % g.nbz), by = int((i / g.nbz) % g.nby), bx = int(i / ((long long)g.nbz * g.nby));
    int n_in = 0, first = 0;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const int lx = bx + (c & 1), ly = by + ((c >> 1) & 1), lz = bz + ((c >> 2) & 1);
        // the point l B - 1.5 lies in [-0.5, dims - 0.5] iff 1 <= l B <= dims + 1
        const int vx = lx << g.lb, vy = ly << g.lb, vz = lz << g.lb;
        const bool in_box = vx >= 1 && vy >= 1 && vz >= 1 && vx <= g.X + 1 && vy <= g.Y + 1 && vz <= g.Z + 1;
        const float v = in_box ? lattice[(((size_t)lx * (g.nby + 1) + ly) * (g.nbz + 1) + lz) * ls] : g.pad_value;
        const int in = v < g.iso;
        n_in += in;
        if (c == 0) first = in;
    }
    seed[i] = n_in != 0 && n_in != 8;
    bsign[i] = (unsigned char)first;
}

__global__ __launch_bounds__(256) void k_mcs_dilate(McsGrid g, const unsigned char* __restrict__ in, unsigned char* __restrict__ out) {
    const long long NB = (long long)g.nbx * g.nby * g.nbz;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= NB) return;
    const int bz = int(i % g.nbz), by = int((i / g.nbz) % g.nby), bx = int(i / ((long long)g.nbz * g.nby));
    int any = 0;
    for (int dx = -1; dx <= 1; ++dx)
        for (int dy = -1; dy <= 1; ++dy)
            for (int dz = -1; dz <= 1; ++dz) {
                const int x = bx + dx, y = by + dy, z = bz + dz;
                if (x >= 0 && y >= 0 && z >= 0 && x < g.nbx && y < g.nby && z < g.nbz) any |= in[mcs_brick_lin(g, x, y, z)];
            }
    out[i] = (unsigned char)(any != 0);
}

__global__ __launch_bounds__(256) void k_mcs_fill(unsigned char* __restrict__ p, long long n, unsigned char v) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = v;
}
__global__ __launch_bounds__(256) void k_mcs_fill_int(int* __restrict__ p, long long n, int v) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = v;
}

__global__ __launch_bounds__(256) void k_mcs_newflag(const unsigned char* __restrict__ mark, const int* __restrict__ table, long long NB,
                                                     int* __restrict__ newf) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < NB) newf[i] = mark[i] && table[i] < 0;
}
__global__ __launch_bounds__(256) void k_mcs_assign(const int* __restrict__ newf, const int* __restrict__ off, long long NB, int first_slot,
                                                    int* __restrict__ table, int* __restrict__ slot_brick) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= NB || !newf[i]) return;
    const int slot = first_slot + off[i];
    table[i] = slot;
    slot_brick[slot] = int(i);
}

__global__ __launch_bounds__(256) void k_mcs_pending(McsGrid g, const int* __restrict__ slot_brick, int first_slot, long long n_entries,
                                                     float* __restrict__ coords) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_entries) return;
    const int m = g.B - 1;
    const int l = int(i & ((1 << (3 * g.lb)) - 1));
    const int b = slot_brick[first_slot + int(i >> (3 * g.lb))];
    const int bz = b % g.nbz, by = (b / g.nbz) % g.nby, bx = b / (g.nbz * g.nby);
    const int sx = (bx << g.lb) + (l >> (2 * g.lb)) - 1, sy = (by << g.lb) + ((l >> g.lb) & m) - 1, sz = (bz << g.lb) + (l & m) - 1;
    coords[i * 3] = float(min(max(sx, 0), g.X - 1));
    coords[i * 3 + 1] = float(min(max(sy, 0), g.Y - 1));
    coords[i * 3 + 2] = float(min(max(sz, 0), g.Z - 1));
}

// One block per slot.  s_val: the (B + 1)^3 values of the brick and its +1 apron; s_act: which of the 27 bricks around are active.
__global__ __launch_bounds__(256) void k_mcs_flags(McsGrid g, const int* __restrict__ slot_brick, int mode, unsigned char* __restrict__ mark,
                                                   unsigned long long* __restrict__ ctr, unsigned long long* __restrict__ vkeys,
                                                   unsigned long long* __restrict__ ckeys) {
    extern __shared__ float s_val[];
    __shared__ int s_act[27];
    __shared__ unsigned s_cnt[3];
    __shared__ unsigned long long s_base[2];
    const int tid = threadIdx.x, B = g.B, lb = g.lb, m = B - 1, E = B + 1;
    const int slot = blockIdx.x;
    const int b = slot_brick[slot];
    const int bz = b % g.nbz, by = (b / g.nbz) % g.nby, bx = b / (g.nbz * g.nby);
    const int ox = bx << lb, oy = by << lb, oz = bz << lb;
    if (tid < 27) {
        const int x = bx + tid / 9 - 1, y = by + (tid / 3) % 3 - 1, z = bz + tid % 3 - 1;
        const bool in = x >= 0 && y >= 0 && z >= 0 && x < g.nbx && y < g.nby && z < g.nbz;
        s_act[tid] = in && g.table[mcs_brick_lin(g, x, y, z)] >= 0;
    }
    if (tid < 3) s_cnt[tid] = 0;
    for (int i = tid; i < E * E * E; i += 256) {
        const int lz = i % E, ly = (i / E) % E, lx = i / (E * E);
        const int x = ox + lx, y = oy + ly, z = oz + lz;
        float v = g.pad_value;
        if (x < g.Px && y < g.Py && z < g.Pz && !mcs_is_pad(g, x, y, z)) {
            if (lx < B && ly < B && lz < B) v = g.pool[(((size_t)slot << (3 * lb)) + (((lx << lb) | ly) << lb | lz)) * g.stride];
            else v = mcs_value(g, x, y, z);
        }
        s_val[i] = v;
    }
    __syncthreads();
    const long long NV = (long long)g.Px * g.Py * g.Pz;

    // 0: no such cell, 1: extracted, 2: not extracted.  Cells around this brick's vertices: origin in [o - 1, o + B - 1] per axis
    auto cell_state = [&](int cx, int cy, int cz) -> int {
        if (cx < 0 || cy < 0 || cz < 0 || cx + 1 >= g.Px || cy + 1 >= g.Py || cz + 1 >= g.Pz) return 0;
        const int x0 = (cx >> lb) - bx + 1, x1 = ((cx + 1) >> lb) - bx + 1, y0 = (cy >> lb) - by + 1, y1 = ((cy + 1) >> lb) - by + 1;
        const int z0 = (cz >> lb) - bz + 1, z1 = ((cz + 1) >> lb) - bz + 1;
        const int all = s_act[x0 * 9 + y0 * 3 + z0] & s_act[x0 * 9 + y0 * 3 + z1] & s_act[x0 * 9 + y1 * 3 + z0] & s_act[x0 * 9 + y1 * 3 + z1] &
                        s_act[x1 * 9 + y0 * 3 + z0] & s_act[x1 * 9 + y0 * 3 + z1] & s_act[x1 * 9 + y1 * 3 + z0] & s_act[x1 * 9 + y1 * 3 + z1];
        return all ? 1 : 2;
    };
    // what entry l of the brick contributes: bits 0-2 the kept cut edges, bits 3-5 the triangle count of its cell, bits 8.. the
    // boundary cut edges (BOUNDARY marks the bricks around them as it goes)
    auto entry = [&](int l) -> unsigned {
        const int lx = l >> (2 * lb), ly = (l >> lb) & m, lz = l & m;
        const int x = ox + lx, y = oy + ly, z = oz + lz;
        if (x >= g.Px || y >= g.Py || z >= g.Pz) return 0u;
        const int li = (lx * E + ly) * E + lz;
        const bool in0 = s_val[li] < g.iso;
        unsigned r = 0;
#pragma unroll
        for (int axis = 0; axis < 3; ++axis) {
            const int p1 = axis == 0 ? x + 1 : axis == 1 ? y + 1 : z + 1, lim = axis == 0 ? g.Px : axis == 1 ? g.Py : g.Pz;
            if (p1 >= lim) continue;
            int st[4], cxs[4], cys[4], czs[4], ext = 0, non = 0;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int d0 = q & 1, d1 = q >> 1;
                cxs[q] = axis == 0 ? x : x - d0;
                cys[q] = axis == 1 ? y : (axis == 0 ? y - d0 : y - d1);
                czs[q] = axis == 2 ? z : z - d1;
                st[q] = cell_state(cxs[q], cys[q], czs[q]);
                ext |= st[q] == 1;
                non |= st[q] == 2;
            }
            if (!ext) continue;                                     // (then both ends lie in active bricks)
            const int l1 = li + (axis == 0 ? E * E : axis == 1 ? E : 1);
            if (in0 == (s_val[l1] < g.iso)) continue;
            r |= 1u << axis;
            if (mode == MCS_BOUNDARY && non) {
                r += 1u << 8;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    if (st[q] != 2) continue;
                    for (int c = 0; c < 8; ++c)
                        mark[mcs_brick_lin(g, (cxs[q] + (c & 1)) >> lb, (cys[q] + ((c >> 1) & 1)) >> lb, (czs[q] + ((c >> 2) & 1)) >> lb)] = 1;
                }
            }
        }
        if (mode != MCS_BOUNDARY && cell_state(x, y, z) == 1) {
            int cs = 0;
#pragma unroll
            for (int c = 0; c < 8; ++c) cs |= int(s_val[li + ((c & 1) * E + ((c >> 1) & 1)) * E + ((c >> 2) & 1)] < g.iso) << c;
            r |= unsigned(d_mcs_ntri[cs]) << 3;
        }
        return r;
    };

    unsigned nv = 0, nc = 0, nbd = 0;
    for (int l = tid; l < (1 << (3 * lb)); l += 256) {
        const unsigned r = entry(l);
        nv += __popc(r & 7u);
        nc += ((r >> 3) & 7u) != 0;
        nbd += r >> 8;
    }
    if (mode == MCS_BOUNDARY) {
        if (nbd) atomicAdd(&s_cnt[2], nbd);
        __syncthreads();
        if (tid == 0 && s_cnt[2]) atomicAdd(&ctr[CTR_BOUNDARY], (unsigned long long)s_cnt[2]);
        return;
    }
    // this thread's place among the block's keys (any order: the lists are sorted afterwards)
    const unsigned vo = nv ? atomicAdd(&s_cnt[0], nv) : 0u, co = nc ? atomicAdd(&s_cnt[1], nc) : 0u;
    __syncthreads();
    if (mode == MCS_COUNT) {
        if (tid == 0) {
            if (s_cnt[0]) atomicAdd(&ctr[CTR_NV], (unsigned long long)s_cnt[0]);
            if (s_cnt[1]) atomicAdd(&ctr[CTR_NC], (unsigned long long)s_cnt[1]);
        }
        return;
    }
    if (tid == 0) {
        s_base[0] = s_cnt[0] ? atomicAdd(&ctr[CTR_VCUR], (unsigned long long)s_cnt[0]) : 0ull;
        s_base[1] = s_cnt[1] ? atomicAdd(&ctr[CTR_CCUR], (unsigned long long)s_cnt[1]) : 0ull;
    }
    __syncthreads();
    unsigned long long vp = s_base[0] + vo, cp = s_base[1] + co;
    if (!nv && !nc) return;
    for (int l = tid; l < (1 << (3 * lb)); l += 256) {
        const unsigned r = entry(l);
        if (!(r & 63u)) continue;
        const int x = ox + (l >> (2 * lb)), y = oy + ((l >> lb) & m), z = oz + (l & m);
        const unsigned long long lin = ((unsigned long long)x * g.Py + y) * g.Pz + z;
#pragma unroll
        for (int axis = 0; axis < 3; ++axis)
            if (r & (1u << axis)) vkeys[vp++] = (unsigned long long)axis * NV + lin;
        if ((r >> 3) & 7u) ckeys[cp++] = lin * 8ull + ((r >> 3) & 7u);
    }
}

__global__ __launch_bounds__(256) void k_mcs_cell_ntri(const unsigned long long* __restrict__ ckeys, long long nc, unsigned* __restrict__ nt) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < nc) nt[i] = unsigned(ckeys[i] & 7ull);
}

// vertex o is the edge of the o-th smallest key; positions, t and attributes as k_mc_verts computes them (pad = 1)
__global__ __launch_bounds__(256) void k_mcs_verts(McsGrid g, const unsigned long long* __restrict__ vkeys, long long nv, float* __restrict__ verts,
                                                   float* __restrict__ attrs, int n_attr) {
    const long long o = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (o >= nv) return;
    const long long NV = (long long)g.Px * g.Py * g.Pz;
    const unsigned long long key = vkeys[o];
    const int axis = int(key / (unsigned long long)NV);
    const long long i = (long long)(key % (unsigned long long)NV);
    const int z = int(i % g.Pz), y = int((i / g.Pz) % g.Py), x = int(i / ((long long)g.Pz * g.Py));
    const int x1 = x + (axis == 0), y1 = y + (axis == 1), z1 = z + (axis == 2);
    const float v0 = mcs_value(g, x, y, z), v1 = mcs_value(g, x1, y1, z1);
    const float t = (g.iso - v0) / (v1 - v0);
    float p[3] = {float(x - 1), float(y - 1), float(z - 1)};
    p[axis] += t;
    verts[o * 3] = p[0]; verts[o * 3 + 1] = p[1]; verts[o * 3 + 2] = p[2];
    if (attrs) {
        // a padded end point has no attributes, take the other one's (an edge has at most one end in the shell)
        const bool a_in = !mcs_is_pad(g, x, y, z), b_in = !mcs_is_pad(g, x1, y1, z1);
        const long long ea = a_in ? mcs_entry(g, x, y, z) : mcs_entry(g, x1, y1, z1);
        const long long eb = b_in ? mcs_entry(g, x1, y1, z1) : mcs_entry(g, x, y, z);
        const float* pa = g.pool + size_t(max(ea, 0ll)) * g.stride + 1;
        const float* pb = g.pool + size_t(max(eb, 0ll)) * g.stride + 1;
        for (int k = 0; k < n_attr; ++k) attrs[o * n_attr + k] = pa[k] + t * (pb[k] - pa[k]);
    }
}

__device__ __forceinline__ long long mcs_find(const unsigned long long* __restrict__ keys, long long n, unsigned long long key) {
    long long lo = 0, hi = n;                                    // first index with keys[index] >= key
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (keys[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(256) void k_mcs_tris(McsGrid g, const unsigned long long* __restrict__ ckeys, long long nc, const unsigned* __restrict__ toff,
                                                  const unsigned long long* __restrict__ vkeys, long long nv, int* __restrict__ tris) {
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= nc) return;
    const long long NV = (long long)g.Px * g.Py * g.Pz;
    const long long i = (long long)(ckeys[j] >> 3);
    const int z = int(i % g.Pz), y = int((i / g.Pz) % g.Py), x = int(i / ((long long)g.Pz * g.Py));
    int cs = 0;
#pragma unroll
    for (int c = 0; c < 8; ++c) cs |= int(mcs_value(g, x + (c & 1), y + ((c >> 1) & 1), z + ((c >> 2) & 1)) < g.iso) << c;
    int* out = tris + size_t(toff[j]) * 3;
    const int n = d_mcs_ntri[cs];
    for (int k = 0; k < 3 * n; ++k) {
        const int e = d_mcs_tri[cs][k];
        const int c0 = d_mcs_edge[e][0], axis = d_mcs_edge_axis[e];
        const long long lin = ((long long)(x + (c0 & 1)) * g.Py + (y + ((c0 >> 1) & 1))) * g.Pz + (z + ((c0 >> 2) & 1));
        out[k] = int(mcs_find(vkeys, nv, (unsigned long long)axis * NV + lin));
    }
}

__global__ __launch_bounds__(256) void k_mcs_occupancy(McsGrid g, const unsigned char* __restrict__ bsign, unsigned char* __restrict__ occ) {
    const long long N = (long long)g.X * g.Y * g.Z;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const int z = int(i % g.Z) + 1, y = int((i / g.Z) % g.Y) + 1, x = int(i / ((long long)g.Z * g.Y)) + 1;      // never a pad vertex
    const long long e = mcs_entry(g, x, y, z);
    occ[i] = e >= 0 ? (unsigned char)(g.pool[size_t(e) * g.stride] < g.iso) : bsign[mcs_brick_lin(g, x >> g.lb, y >> g.lb, z >> g.lb)];
}

}  // namespace s3d

using namespace s3d;

struct s3d_mcs {
    DevBuf table, slot_brick, mark, mark2, bsign, newf, off, tmp, ctr, vkeys, ckeys, cnt, toff;
    McsGrid g{};
    long long NB = 0;
    long long n_slots = 0, first_new = 0;          // slots [first_new, n_slots) are the newest
    int64_t nv = -1, nc = 0, nt = -1;
    unsigned long long* vsorted = nullptr;         // the sorted halves of vkeys / ckeys
    unsigned long long* csorted = nullptr;
    bool planned = false, seeded = false, tables = false;
};

namespace {

inline unsigned blocks_of(long long n) { return (unsigned)((n + 255) / 256); }

int bits_for(unsigned long long max_key) {
    int b = 1;
    while (b < 64 && (max_key >> b)) ++b;
    return b;
}

// slots for the bricks of `mark` that have none yet, in ascending brick index; synchronises
int mcs_activate(s3d_mcs* m, const unsigned char* mark, int64_t* n_new, hipStream_t st) {
    const long long NB = m->NB;
    int* newf = static_cast<int*>(m->newf.p); int* off = static_cast<int*>(m->off.p);
    int* table = static_cast<int*>(m->table.p);
    hipLaunchKernelGGL(k_mcs_newflag, dim3(blocks_of(NB)), dim3(256), 0, st, mark, table, NB, newf);
    S3D_HIP(hipGetLastError());
    size_t tb = 0;
    S3D_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, tb, newf, off, int(NB), st));
    S3D_TRY(m->tmp.reserve(tb));
    tb = m->tmp.cap;
    S3D_HIP(hipcub::DeviceScan::ExclusiveSum(m->tmp.p, tb, newf, off, int(NB), st));
    int last[2];
    S3D_HIP(hipMemcpyAsync(&last[0], off + NB - 1, 4, hipMemcpyDeviceToHost, st));
    S3D_HIP(hipMemcpyAsync(&last[1], newf + NB - 1, 4, hipMemcpyDeviceToHost, st));
    S3D_HIP(hipStreamSynchronize(st));
    const long long nn = (long long)last[0] + last[1];
    const long long per = 1ll << (3 * m->g.lb);
    S3D_CHECK((m->n_slots + nn) * per <= (long long)S3D_MCS_MAX_SAMPLES, S3D_ERR_UNSUPPORTED,
              "mcs: %lld active bricks of %d^3 samples exceed the pool limit of %lld samples", m->n_slots + nn, m->g.B,
              (long long)S3D_MCS_MAX_SAMPLES);
    if (nn) {
        hipLaunchKernelGGL(k_mcs_assign, dim3(blocks_of(NB)), dim3(256), 0, st, newf, off, NB, int(m->n_slots), table,
                           static_cast<int*>(m->slot_brick.p));
        S3D_HIP(hipGetLastError());
    }
    m->first_new = m->n_slots;
    m->n_slots += nn;
    *n_new = nn;
    return 0;
}

int mcs_launch_flags(s3d_mcs* m, int mode, hipStream_t st) {
    const int E = m->g.B + 1;
    hipLaunchKernelGGL(k_mcs_flags, dim3((unsigned)m->n_slots), dim3(256), size_t(E) * E * E * sizeof(float), st, m->g,
                       static_cast<const int*>(m->slot_brick.p), mode, static_cast<unsigned char*>(m->mark.p),
                       static_cast<unsigned long long*>(m->ctr.p), static_cast<unsigned long long*>(m->vkeys.p),
                       static_cast<unsigned long long*>(m->ckeys.p));
    S3D_HIP(hipGetLastError());
    return 0;
}

}  // namespace

extern "C" {

int s3d_mcs_create(s3d_mcs** out) {
    S3D_CHECK(out, S3D_ERR_INVALID, "mcs_create: null argument");
    *out = new s3d_mcs();
    return 0;
}
void s3d_mcs_destroy(s3d_mcs* m) { delete m; }

int s3d_mcs_plan(s3d_mcs* m, int X, int Y, int Z, int block, int pad, float pad_value, float iso, int nb[3]) {
    S3D_CHECK(m && nb, S3D_ERR_INVALID, "mcs_plan: null argument");
    S3D_CHECK(X >= 1 && Y >= 1 && Z >= 1 && X <= (1 << 20) && Y <= (1 << 20) && Z <= (1 << 20), S3D_ERR_INVALID, "mcs_plan: bad grid description");
    S3D_CHECK(block == 4 || block == 8 || block == 16, S3D_ERR_INVALID, "mcs_plan: brick size %d, expected 4, 8 or 16", block);
    S3D_CHECK(pad == 1, S3D_ERR_INVALID, "mcs_plan: the narrow-band extraction works on the padded grid (pad = 1)");
    m->planned = m->seeded = false;
    m->nv = m->nt = -1;
    McsGrid& g = m->g;
    g = McsGrid{};
    g.X = X; g.Y = Y; g.Z = Z; g.Px = X + 2; g.Py = Y + 2; g.Pz = Z + 2;
    g.B = block; g.lb = block == 4 ? 2 : block == 8 ? 3 : 4;
    g.nbx = (g.Px + block - 1) / block; g.nby = (g.Py + block - 1) / block; g.nbz = (g.Pz + block - 1) / block;
    g.iso = iso; g.pad_value = pad_value;
    const double nbricks = double(g.nbx) * g.nby * g.nbz;
    S3D_CHECK(nbricks <= double(S3D_MCS_MAX_BRICKS), S3D_ERR_UNSUPPORTED, "mcs_plan: %d x %d x %d bricks exceed the table limit of %d",
              g.nbx, g.nby, g.nbz, S3D_MCS_MAX_BRICKS);
    m->NB = (long long)nbricks;
    nb[0] = g.nbx; nb[1] = g.nby; nb[2] = g.nbz;
    if (!m->tables) {
        S3D_HIP(hipMemcpyToSymbol(HIP_SYMBOL(d_mcs_edge), MC_EDGE, sizeof MC_EDGE));
        S3D_HIP(hipMemcpyToSymbol(HIP_SYMBOL(d_mcs_edge_axis), MC_EDGE_AXIS, sizeof MC_EDGE_AXIS));
        S3D_HIP(hipMemcpyToSymbol(HIP_SYMBOL(d_mcs_ntri), MC_NTRI, sizeof MC_NTRI));
        S3D_HIP(hipMemcpyToSymbol(HIP_SYMBOL(d_mcs_tri), MC_TRI, sizeof MC_TRI));
        m->tables = true;
    }
    S3D_HIP(hipDeviceSynchronize());                         // buffers may still be in use by an earlier extraction
    const size_t NB = size_t(m->NB);
    S3D_TRY(m->table.reserve(NB * 4)); S3D_TRY(m->slot_brick.reserve(NB * 4)); S3D_TRY(m->newf.reserve(NB * 4)); S3D_TRY(m->off.reserve(NB * 4));
    S3D_TRY(m->mark.reserve(NB)); S3D_TRY(m->mark2.reserve(NB)); S3D_TRY(m->bsign.reserve(NB));
    S3D_TRY(m->ctr.reserve(CTR_COUNT * sizeof(unsigned long long)));
    g.table = static_cast<const int*>(m->table.p);
    m->n_slots = m->first_new = 0;
    m->planned = true;
    return 0;
}

int s3d_mcs_seed(s3d_mcs* m, const float* lattice, int lattice_stride, int dilate, int all_active, int64_t* n_seed, int64_t* n_new,
                 void* stream) {
    S3D_CHECK(m && n_seed && n_new, S3D_ERR_INVALID, "mcs_seed: null argument");
    S3D_CHECK(m->planned && !m->seeded, S3D_ERR_INVALID, "mcs_seed: call s3d_mcs_plan first (once per plan)");
    S3D_CHECK(all_active || (lattice && lattice_stride >= 1), S3D_ERR_INVALID, "mcs_seed: no lattice values");
    S3D_CHECK(dilate >= 0 && dilate <= 1024, S3D_ERR_INVALID, "mcs_seed: dilate %d", dilate);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const long long NB = m->NB;
    unsigned char* mark = static_cast<unsigned char*>(m->mark.p);
    unsigned char* mark2 = static_cast<unsigned char*>(m->mark2.p);
    unsigned char* bsign = static_cast<unsigned char*>(m->bsign.p);
    hipLaunchKernelGGL(k_mcs_fill_int, dim3(blocks_of(NB)), dim3(256), 0, st, static_cast<int*>(m->table.p), NB, -1);
    if (all_active) {
        hipLaunchKernelGGL(k_mcs_fill, dim3(blocks_of(NB)), dim3(256), 0, st, mark, NB, (unsigned char)1);
        hipLaunchKernelGGL(k_mcs_fill, dim3(blocks_of(NB)), dim3(256), 0, st, bsign, NB, (unsigned char)0);
        S3D_HIP(hipGetLastError());
        *n_seed = NB;
    } else {
        hipLaunchKernelGGL(k_mcs_seed, dim3(blocks_of(NB)), dim3(256), 0, st, m->g, lattice, lattice_stride, mark, bsign);
        S3D_HIP(hipGetLastError());
        // the seed count: the bricks a scan of the flags would number (the table is still empty)
        int64_t ns = 0;
        {
            int* newf = static_cast<int*>(m->newf.p); int* off = static_cast<int*>(m->off.p);
            hipLaunchKernelGGL(k_mcs_newflag, dim3(blocks_of(NB)), dim3(256), 0, st, mark, static_cast<const int*>(m->table.p), NB, newf);
            size_t tb = 0;
            S3D_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, tb, newf, off, int(NB), st));
            S3D_TRY(m->tmp.reserve(tb));
            tb = m->tmp.cap;
            S3D_HIP(hipcub::DeviceScan::ExclusiveSum(m->tmp.p, tb, newf, off, int(NB), st));
            int last[2];
            S3D_HIP(hipMemcpyAsync(&last[0], off + NB - 1, 4, hipMemcpyDeviceToHost, st));
            S3D_HIP(hipMemcpyAsync(&last[1], newf + NB - 1, 4, hipMemcpyDeviceToHost, st));
            S3D_HIP(hipStreamSynchronize(st));
            ns = int64_t(last[0]) + last[1];
        }
        *n_seed = ns;
        for (int k = 0; k < dilate; ++k) {
            hipLaunchKernelGGL(k_mcs_dilate, dim3(blocks_of(NB)), dim3(256), 0, st, m->g, mark, mark2);
            S3D_HIP(hipGetLastError());
            std::swap(mark, mark2);
        }
    }
    S3D_TRY(mcs_activate(m, mark, n_new, st));
    m->seeded = true;
    return 0;
}

int s3d_mcs_pending(s3d_mcs* m, float* coords, void* stream) {
    S3D_CHECK(m && m->seeded, S3D_ERR_INVALID, "mcs_pending: call s3d_mcs_seed first");
    const long long n = (m->n_slots - m->first_new) << (3 * m->g.lb);
    if (!n) return 0;
    S3D_CHECK(coords, S3D_ERR_INVALID, "mcs_pending: null output");
    hipLaunchKernelGGL(k_mcs_pending, dim3(blocks_of(n)), dim3(256), 0, static_cast<hipStream_t>(stream), m->g,
                       static_cast<const int*>(m->slot_brick.p), int(m->first_new), n, coords);
    S3D_HIP(hipGetLastError());
    return 0;
}

int s3d_mcs_grow(s3d_mcs* m, const float* pool, int stride, int activate, int64_t* n_boundary, int64_t* n_new, void* stream) {
    S3D_CHECK(m && n_boundary && n_new, S3D_ERR_INVALID, "mcs_grow: null argument");
    S3D_CHECK(m->seeded, S3D_ERR_INVALID, "mcs_grow: call s3d_mcs_seed first");
    S3D_CHECK((pool || !m->n_slots) && stride >= 1, S3D_ERR_INVALID, "mcs_grow: no pool");
    hipStream_t st = static_cast<hipStream_t>(stream);
    *n_boundary = 0; *n_new = 0;
    m->first_new = m->n_slots;
    if (!m->n_slots) return 0;
    m->g.pool = pool; m->g.stride = stride;
    S3D_HIP(hipMemsetAsync(m->ctr.p, 0, CTR_COUNT * sizeof(unsigned long long), st));
    S3D_HIP(hipMemsetAsync(m->mark.p, 0, size_t(m->NB), st));
    S3D_TRY(mcs_launch_flags(m, MCS_BOUNDARY, st));
    unsigned long long nb = 0;
    S3D_HIP(hipMemcpyAsync(&nb, static_cast<unsigned long long*>(m->ctr.p) + CTR_BOUNDARY, 8, hipMemcpyDeviceToHost, st));
    S3D_HIP(hipStreamSynchronize(st));
    *n_boundary = int64_t(nb);
    if (!nb || !activate) return 0;
    return mcs_activate(m, static_cast<const unsigned char*>(m->mark.p), n_new, st);
}

int s3d_mcs_count(s3d_mcs* m, const float* pool, int stride, int64_t* n_verts, int64_t* n_tris, void* stream) {
    S3D_CHECK(m && n_verts && n_tris, S3D_ERR_INVALID, "mcs_count: null argument");
    S3D_CHECK(m->seeded, S3D_ERR_INVALID, "mcs_count: call s3d_mcs_seed first");
    S3D_CHECK((pool || !m->n_slots) && stride >= 1, S3D_ERR_INVALID, "mcs_count: no pool");
    hipStream_t st = static_cast<hipStream_t>(stream);
    m->g.pool = pool; m->g.stride = stride;
    m->nv = m->nc = m->nt = 0;
    *n_verts = *n_tris = 0;
    if (!m->n_slots) return 0;
    unsigned long long* ctr = static_cast<unsigned long long*>(m->ctr.p);
    S3D_HIP(hipMemsetAsync(ctr, 0, CTR_COUNT * sizeof(unsigned long long), st));
    S3D_TRY(mcs_launch_flags(m, MCS_COUNT, st));
    unsigned long long h[CTR_COUNT];
    S3D_HIP(hipMemcpyAsync(h, ctr, sizeof h, hipMemcpyDeviceToHost, st));
    S3D_HIP(hipStreamSynchronize(st));
    const unsigned long long nv = h[CTR_NV], nc = h[CTR_NC];
    S3D_CHECK(nv < 2147483648ull && nc < 2147483648ull, S3D_ERR_UNSUPPORTED, "mcs_count: %llu vertices, %llu cells: more than 32-bit indices hold", nv, nc);
    if (!nv && !nc) return 0;
    m->nv = m->nt = -1;
    S3D_CHECK(nv && nc, S3D_ERR_INTERNAL, "mcs_count: %llu vertices but %llu cells with triangles", nv, nc);    // (a kept vertex has an extracted cell)
    S3D_TRY(m->vkeys.reserve(size_t(nv) * 16)); S3D_TRY(m->ckeys.reserve(size_t(nc) * 16));
    S3D_TRY(m->cnt.reserve(size_t(nc) * 4)); S3D_TRY(m->toff.reserve(size_t(nc) * 4));
    unsigned long long* vk = static_cast<unsigned long long*>(m->vkeys.p); unsigned long long* ck = static_cast<unsigned long long*>(m->ckeys.p);
    S3D_TRY(mcs_launch_flags(m, MCS_EMIT, st));
    const unsigned long long NV = (unsigned long long)m->g.Px * m->g.Py * m->g.Pz;
    const int vbits = bits_for(3 * NV), cbits = bits_for(NV * 8);
    size_t t1 = 0, t2 = 0, t3 = 0;
    S3D_HIP(hipcub::DeviceRadixSort::SortKeys(nullptr, t1, vk, vk + nv, int(nv), 0, vbits, st));
    S3D_HIP(hipcub::DeviceRadixSort::SortKeys(nullptr, t2, ck, ck + nc, int(nc), 0, cbits, st));
    unsigned* cnt = static_cast<unsigned*>(m->cnt.p); unsigned* toff = static_cast<unsigned*>(m->toff.p);
    S3D_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, t3, cnt, toff, int(nc), st));
    S3D_TRY(m->tmp.reserve(std::max(t1, std::max(t2, t3))));
    size_t tb = m->tmp.cap;
    S3D_HIP(hipcub::DeviceRadixSort::SortKeys(m->tmp.p, tb, vk, vk + nv, int(nv), 0, vbits, st));
    tb = m->tmp.cap;
    S3D_HIP(hipcub::DeviceRadixSort::SortKeys(m->tmp.p, tb, ck, ck + nc, int(nc), 0, cbits, st));
    m->vsorted = vk + nv; m->csorted = ck + nc;
    hipLaunchKernelGGL(k_mcs_cell_ntri, dim3(blocks_of((long long)nc)), dim3(256), 0, st, m->csorted, (long long)nc, cnt);
    S3D_HIP(hipGetLastError());
    tb = m->tmp.cap;
    S3D_HIP(hipcub::DeviceScan::ExclusiveSum(m->tmp.p, tb, cnt, toff, int(nc), st));
    unsigned last[2];
    S3D_HIP(hipMemcpyAsync(&last[0], toff + nc - 1, 4, hipMemcpyDeviceToHost, st));
    S3D_HIP(hipMemcpyAsync(&last[1], cnt + nc - 1, 4, hipMemcpyDeviceToHost, st));
    S3D_HIP(hipMemcpyAsync(h, ctr, sizeof h, hipMemcpyDeviceToHost, st));
    S3D_HIP(hipStreamSynchronize(st));
    S3D_CHECK(h[CTR_VCUR] == nv && h[CTR_CCUR] == nc, S3D_ERR_INTERNAL, "mcs_count: %llu / %llu keys appended, %llu / %llu counted",
              h[CTR_VCUR], h[CTR_CCUR], nv, nc);
    const unsigned long long nt = (unsigned long long)last[0] + last[1];
    S3D_CHECK(nt < 2147483648ull / 3, S3D_ERR_UNSUPPORTED, "mcs_count: %llu triangles: more than 32-bit offsets hold", nt);
    m->nv = int64_t(nv); m->nc = int64_t(nc); m->nt = int64_t(nt);
    *n_verts = m->nv; *n_tris = m->nt;
    return 0;
}

int s3d_mcs_extract(s3d_mcs* m, float* verts, float* attrs, int n_attr, int32_t* tris, void* stream) {
    S3D_CHECK(m && m->nv >= 0 && m->nt >= 0, S3D_ERR_INVALID, "mcs_extract: call s3d_mcs_count first");
    S3D_CHECK((m->nv == 0 || verts) && (m->nt == 0 || tris), S3D_ERR_INVALID, "mcs_extract: null output");
    S3D_CHECK(!attrs || (n_attr >= 1 && n_attr <= m->g.stride - 1), S3D_ERR_INVALID,
              "mcs_extract: %d attributes requested, the pool has %d channels after the value", n_attr, m->g.stride - 1);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (m->nv) hipLaunchKernelGGL(k_mcs_verts, dim3(blocks_of(m->nv)), dim3(256), 0, st, m->g, m->vsorted, (long long)m->nv, verts, attrs, n_attr);
    if (m->nt) hipLaunchKernelGGL(k_mcs_tris, dim3(blocks_of(m->nc)), dim3(256), 0, st, m->g, m->csorted, (long long)m->nc,
                                  static_cast<const unsigned*>(m->toff.p), m->vsorted, (long long)m->nv, tris);
    S3D_HIP(hipGetLastError());
    return 0;
}

int s3d_mcs_occupancy(s3d_mcs* m, const float* pool, int stride, uint8_t* occ, void* stream) {
    S3D_CHECK(m && occ, S3D_ERR_INVALID, "mcs_occupancy: null argument");
    S3D_CHECK(m->seeded, S3D_ERR_INVALID, "mcs_occupancy: call s3d_mcs_seed first");
    S3D_CHECK((pool || !m->n_slots) && stride >= 1, S3D_ERR_INVALID, "mcs_occupancy: no pool");
    m->g.pool = pool; m->g.stride = stride;
    const long long N = (long long)m->g.X * m->g.Y * m->g.Z;
    S3D_CHECK(N < (1ll << 39), S3D_ERR_UNSUPPORTED, "mcs_occupancy: %lld voxels", N);
    hipLaunchKernelGGL(k_mcs_occupancy, dim3(blocks_of(N)), dim3(256), 0, static_cast<hipStream_t>(stream), m->g,
                       static_cast<const unsigned char*>(m->bsign.p), occ);
    S3D_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
