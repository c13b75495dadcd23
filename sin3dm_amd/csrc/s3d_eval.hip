// s3d_eval.hip — the geometry metrics of the reference's evaluation/patch_utils.py on the device: LP-IoU, LP-F-score and the
// pairwise-IoU diversity.  Every quantity is a function of three integer counts (|g & r|, |g|, |r|), so occupancy is bit-packed
// into 64-bit words (bit t of a patch = voxel (i, j, k) with t = (i * ps + j) * ps + k, word t / 64, bit t % 64, tail bits zero)
// and one pass of AND + population count gives both LP metrics.  DESIGN.md §17.  Compaction, the shuffle and the means stay with
// the caller (torch).  Integer arithmetic, and maxima of non-negative floats taken on their bit patterns: no float atomics on
// sums, results independent of the launch geometry.  The float32 expressions are spelled with __fdiv_rn / __fmul_rn / __fadd_rn
// so that nothing contracts and a float32 restatement gives the same bits.
#include "s3d_common.h"

namespace s3d {

constexpr int kEvalThreads = 256;
constexpr int kEvalWaves = kEvalThreads / 64;
constexpr int kLpGen = 8;                   // generated patches per workgroup of k_eval_lp_max
static inline unsigned eval_blocks(long long n) { return (unsigned)((n + kEvalThreads - 1) / kEvalThreads); }

// per axis: the number of candidate patches of the volume zero-padded by ps / 2 on both sides
__host__ __device__ static inline int eval_axis_count(int n, int ps, int stride) { return (n + 2 * (ps / 2) - ps) / stride + 1; }

// voxel (x, y, z) of the implicitly zero-padded volume, in unpadded coordinates
__device__ static inline bool eval_vox(const unsigned char* __restrict__ vox, int H, int W, int D, int x, int y, int z) {
    if ((unsigned)x >= (unsigned)H || (unsigned)y >= (unsigned)W || (unsigned)z >= (unsigned)D) return false;
    return vox[((long long)x * W + y) * D + z] != 0;
}

// ------------------------------------------------------------------ occupancy pooling
// out[i][j][k] = OR of vox over the adaptive-pooling window [floor(i * in / out), ceil((i + 1) * in / out)) per axis
__global__ void __launch_bounds__(kEvalThreads) k_eval_pool_or(const unsigned char* __restrict__ vox, int H, int W, int D, int oH, int oW, int oD,
                                                               unsigned char* __restrict__ out) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (long long)oH * oW * oD) return;
    const int k = int(t % oD), j = int((t / oD) % oW), i = int(t / ((long long)oD * oW));
    const int x0 = int((long long)i * H / oH), x1 = int(((long long)(i + 1) * H + oH - 1) / oH);
    const int y0 = int((long long)j * W / oW), y1 = int(((long long)(j + 1) * W + oW - 1) / oW);
    const int z0 = int((long long)k * D / oD), z1 = int(((long long)(k + 1) * D + oD - 1) / oD);
    bool any = false;
    for (int x = x0; x < x1 && !any; ++x)
        for (int y = y0; y < y1 && !any; ++y)
            for (int z = z0; z < z1; ++z) any = any || vox[((long long)x * W + y) * D + z] != 0;
    out[t] = any ? 1 : 0;
}

// ------------------------------------------------------------------ patch validity
// flags[(a * nb + b) * nc + c] = the centre cube (side l, from ps / 2 - 1) of candidate (a, b, c) holds an occupied and a free voxel
__global__ void __launch_bounds__(kEvalThreads) k_eval_patch_valid(const unsigned char* __restrict__ vox, int H, int W, int D, int ps, int stride,
                                                                   int na, int nb, int nc, unsigned char* __restrict__ flags) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (long long)na * nb * nc) return;
    const int c = int(t % nc), b = int((t / nc) % nb), a = int(t / ((long long)nc * nb));
    const int l = (ps & 1) ? 3 : 2, o = -1;                 // the centre starts at ps / 2 - 1 in the patch, the patch at -(ps / 2)
    const int x0 = a * stride + o, y0 = b * stride + o, z0 = c * stride + o;
    int occ = 0;
    for (int i = 0; i < l; ++i)
        for (int j = 0; j < l; ++j)
            for (int k = 0; k < l; ++k) occ += eval_vox(vox, H, W, D, x0 + i, y0 + j, z0 + k) ? 1 : 0;
    flags[t] = (occ > 0 && occ < l * l * l) ? 1 : 0;
}

// ------------------------------------------------------------------ patch packing
// One workgroup per listed candidate; a wave builds one word at a time: lane b tests the voxel of bit w * 64 + b and the wave's
// ballot is the word.  words[p * ps_ + w * ws_] (patch-major: ps_ = n_words, ws_ = 1; word-major: ps_ = 1, ws_ = n);
// counts[p] = the patch's population count.  A candidate index outside the grid packs as an empty patch.
__global__ void __launch_bounds__(kEvalThreads) k_eval_pack_patches(const unsigned char* __restrict__ vox, int H, int W, int D, int ps, int stride,
                                                                    int na, int nb, int nc, const long long* __restrict__ cand, long long n,
                                                                    int n_words, long long pstride, long long wstride,
                                                                    unsigned long long* __restrict__ words, int* __restrict__ counts) {
    __shared__ int wave_count[kEvalWaves];
    const long long p = blockIdx.x;
    if (p >= n) return;                                             // workgroup-uniform
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long ci = cand[p];
    const bool ok = ci >= 0 && ci < (long long)na * nb * nc;
    const int c = ok ? int(ci % nc) : 0, b = ok ? int((ci / nc) % nb) : 0, a = ok ? int(ci / ((long long)nc * nb)) : 0;
    const int pad = ps / 2, bits = ps * ps * ps;
    const int x0 = a * stride - pad, y0 = b * stride - pad, z0 = c * stride - pad;
    int cnt = 0;
    for (int w = wave; w < n_words; w += kEvalWaves) {              // wave-uniform: every lane takes part in the ballot
        const int t = w * 64 + lane;
        const int k = t % ps, j = (t / ps) % ps, i = t / (ps * ps);
        const bool on = ok && t < bits && eval_vox(vox, H, W, D, x0 + i, y0 + j, z0 + k);
        const unsigned long long word = __ballot(on);
        cnt += __popcll(word);
        if (lane == 0) words[p * pstride + w * wstride] = word;
    }
    if (lane == 0) wave_count[wave] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        int s = 0;
#pragma unroll
        for (int i = 0; i < kEvalWaves; ++i) s += wave_count[i];
        counts[p] = s;
    }
}

// ------------------------------------------------------------------ LP maxima
// max_iou[g] = max over r of iou(g, r), max_f[g] = max over r of f(g, r).  Grid (ceil(n_ref / 256), ceil(n_gen / kLpGen)): a
// thread owns one reference patch (word-major: a wave reads 64 patches' word w in one coalesced load) and kLpGen generated
// patches (patch-major; their words are workgroup-uniform, so they come through the scalar unit).  The workgroup's maxima are
// reduced over the wave by shuffles, over the waves through LDS, and merged into the outputs (zeroed by the entry point) by an
// atomicMax on the bit pattern: every value is >= 0, where unsigned order is float order, so the result is order-independent.
__device__ static inline float eval_wave_max(float v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = fmaxf(v, __shfl_xor(v, off));
    return v;
}

__global__ void __launch_bounds__(kEvalThreads) k_eval_lp_max(const unsigned long long* __restrict__ gen, const int* __restrict__ gen_count,
                                                              long long n_gen, const unsigned long long* __restrict__ ref,
                                                              const int* __restrict__ ref_count, long long n_ref, int n_words,
                                                              unsigned* __restrict__ max_iou, unsigned* __restrict__ max_f) {
    __shared__ float red[kEvalWaves][kLpGen][2];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long r = (long long)blockIdx.x * kEvalThreads + threadIdx.x;
    const bool live = r < n_ref;
    const long long rr = live ? r : n_ref - 1;                       // a lane past the end re-reads the last patch and adds nothing
    const long long g0 = (long long)blockIdx.y * kLpGen;
    long long gi[kLpGen];
#pragma unroll
    for (int k = 0; k < kLpGen; ++k) gi[k] = min(g0 + k, n_gen - 1);  // a slot past the end repeats the last patch and is not written
    int inter[kLpGen];
#pragma unroll
    for (int k = 0; k < kLpGen; ++k) inter[k] = 0;
    for (int w = 0; w < n_words; ++w) {
        const unsigned long long rw = ref[(long long)w * n_ref + rr];
#pragma unroll
        for (int k = 0; k < kLpGen; ++k) inter[k] += __popcll(rw & gen[gi[k] * n_words + w]);
    }
    const int nr = ref_count[rr];
    const float fnr = float(nr);
#pragma unroll
    for (int k = 0; k < kLpGen; ++k) {
        const int ng = gen_count[gi[k]];
        const float fi = float(inter[k]);
        const float iou = __fdiv_rn(fi, float(ng + nr - inter[k]));
        const float p = __fdiv_rn(fi, float(ng)), q = __fdiv_rn(fi, fnr);
        const float f = __fdiv_rn(__fmul_rn(__fmul_rn(2.0f, p), q), __fadd_rn(__fadd_rn(p, q), 1e-8f));
        const float mi = eval_wave_max(live ? iou : 0.0f), mf = eval_wave_max(live ? f : 0.0f);
        if (lane == 0) { red[wave][k][0] = mi; red[wave][k][1] = mf; }
    }
    __syncthreads();
    if (threadIdx.x < kLpGen * 2) {
        const int k = threadIdx.x >> 1, which = threadIdx.x & 1;
        float m = red[0][k][which];
#pragma unroll
        for (int i = 1; i < kEvalWaves; ++i) m = fmaxf(m, red[i][k][which]);
        if (g0 + k < n_gen) atomicMax((which ? max_f : max_iou) + g0 + k, __float_as_uint(m));
    }
}

// ------------------------------------------------------------------ diversity: whole volumes
// words[v][w] bit b = vols[v][w * 64 + b] != 0 (tail bits zero): one wave per word
__global__ void __launch_bounds__(kEvalThreads) k_eval_pack_volumes(const unsigned char* __restrict__ vols, long long n, long long voxels,
                                                                    long long n_words, unsigned long long* __restrict__ words) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long word = t >> 6;                                   // wave-uniform: blockDim.x is a multiple of 64
    if (word >= n * n_words) return;
    const long long v = word / n_words, w = word - v * n_words;
    const long long e = w * 64 + (threadIdx.x & 63);
    const unsigned long long bits = __ballot(e < voxels && vols[v * voxels + e] != 0);
    if ((threadIdx.x & 63) == 0) words[word] = bits;
}

// inter[i][j] = |v_i & v_j|, uni[i][j] = |v_i | v_j|: one workgroup per pair, fixed-shape integer reduction
__global__ void __launch_bounds__(kEvalThreads) k_eval_pairwise_counts(const unsigned long long* __restrict__ words, int n, long long n_words,
                                                                       long long* __restrict__ inter, long long* __restrict__ uni) {
    __shared__ long long red[kEvalWaves][2];
    const int i = blockIdx.x / n, j = blockIdx.x % n;
    const unsigned long long* a = words + (long long)i * n_words;
    const unsigned long long* b = words + (long long)j * n_words;
    long long si = 0, su = 0;
    for (long long w = threadIdx.x; w < n_words; w += kEvalThreads) {
        const unsigned long long x = a[w], y = b[w];
        si += __popcll(x & y);
        su += __popcll(x | y);
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        si += __shfl_xor(si, off);
        su += __shfl_xor(su, off);
    }
    if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6][0] = si; red[threadIdx.x >> 6][1] = su; }
    __syncthreads();
    if (threadIdx.x < 2) {
        long long s = 0;
#pragma unroll
        for (int k = 0; k < kEvalWaves; ++k) s += red[k][threadIdx.x];
        (threadIdx.x ? uni : inter)[blockIdx.x] = s;
    }
}

static int eval_check_grid(const char* who, const int dims[3], int patch_size, int stride, int n[3]) {
    S3D_CHECK(dims && dims[0] >= 1 && dims[1] >= 1 && dims[2] >= 1 && (long long)dims[0] * dims[1] * dims[2] < (1LL << 31), S3D_ERR_INVALID,
              "%s: volume dims", who);
    S3D_CHECK(patch_size >= 2 && patch_size <= 32, S3D_ERR_INVALID, "%s: patch_size %d, 2..32 are supported", who, patch_size);
    S3D_CHECK(stride >= 1, S3D_ERR_INVALID, "%s: stride %d", who, stride);
    long long total = 1;
    for (int k = 0; k < 3; ++k) {
        n[k] = eval_axis_count(dims[k], patch_size, stride);
        S3D_CHECK(n[k] >= 1, S3D_ERR_INVALID, "%s: a patch of %d does not fit axis %d of %d voxels", who, patch_size, k, dims[k]);
        total *= n[k];
    }
    S3D_CHECK(total < (1LL << 31), S3D_ERR_INVALID, "%s: %lld candidate patches", who, total);
    return 0;
}

}  // namespace s3d

using namespace s3d;

extern "C" {

int s3d_eval_pool_or(const uint8_t* vox, const int in_dims[3], const int out_dims[3], uint8_t* out, void* stream) {
    S3D_CHECK(vox && out && in_dims && out_dims && vox != out, S3D_ERR_INVALID, "eval_pool_or: null or aliased argument");
    long long ni = 1, no = 1;
    for (int k = 0; k < 3; ++k) {
        S3D_CHECK(in_dims[k] >= 1 && out_dims[k] >= 1, S3D_ERR_INVALID, "eval_pool_or: axis %d: %d -> %d", k, in_dims[k], out_dims[k]);
        ni *= in_dims[k];
        no *= out_dims[k];
    }
    S3D_CHECK(ni < (1LL << 31) && no < (1LL << 31), S3D_ERR_INVALID, "eval_pool_or: volume too large");
    hipLaunchKernelGGL(k_eval_pool_or, dim3(eval_blocks(no)), dim3(kEvalThreads), 0, static_cast<hipStream_t>(stream), vox, in_dims[0], in_dims[1],
                       in_dims[2], out_dims[0], out_dims[1], out_dims[2], out);
    S3D_HIP(hipGetLastError());
    return 0;
}

int s3d_eval_patch_counts(const int dims[3], int patch_size, int stride, int counts[3]) {
    S3D_CHECK(counts, S3D_ERR_INVALID, "eval_patch_counts: null argument");
    return eval_check_grid("eval_patch_counts", dims, patch_size, stride, counts);
}

int s3d_eval_patch_valid(const uint8_t* vox, const int dims[3], int patch_size, int stride, uint8_t* flags, void* stream) {
    int n[3];
    S3D_TRY(eval_check_grid("eval_patch_valid", dims, patch_size, stride, n));
    S3D_CHECK(vox && flags, S3D_ERR_INVALID, "eval_patch_valid: null argument");
    hipLaunchKernelGGL(k_eval_patch_valid, dim3(eval_blocks((long long)n[0] * n[1] * n[2])), dim3(kEvalThreads), 0, static_cast<hipStream_t>(stream),
                       vox, dims[0], dims[1], dims[2], patch_size, stride, n[0], n[1], n[2], flags);
    S3D_HIP(hipGetLastError());
    return 0;
}

int s3d_eval_pack_patches(const uint8_t* vox, const int dims[3], int patch_size, int stride, const int64_t* candidates, int64_t n,
                          int word_major, uint64_t* words, int32_t* counts, void* stream) {
    int g[3];
    S3D_TRY(eval_check_grid("eval_pack_patches", dims, patch_size, stride, g));
    S3D_CHECK(n >= 0 && n < (1LL << 31), S3D_ERR_INVALID, "eval_pack_patches: %lld patches", (long long)n);
    S3D_CHECK(vox && (n == 0 || (candidates && words && counts)), S3D_ERR_INVALID, "eval_pack_patches: null argument");
    if (!n) return 0;
    const int n_words = (patch_size * patch_size * patch_size + 63) / 64;
    hipLaunchKernelGGL(k_eval_pack_patches, dim3((unsigned)n), dim3(kEvalThreads), 0, static_cast<hipStream_t>(stream), vox, dims[0], dims[1],
                       dims[2], patch_size, stride, g[0], g[1], g[2], reinterpret_cast<const long long*>(candidates), (long long)n, n_words,
                       word_major ? 1LL : (long long)n_words, word_major ? (long long)n : 1LL,
                       reinterpret_cast<unsigned long long*>(words), counts);
    S3D_HIP(hipGetLastError());
    return 0;
}

int s3d_eval_lp_max(const uint64_t* gen_words, const int32_t* gen_counts, int64_t n_gen, const uint64_t* ref_words, const int32_t* ref_counts,
                    int64_t n_ref, int n_words, float* max_iou, float* max_f, void* stream) {
    S3D_CHECK(n_gen >= 0 && n_ref >= 0 && n_gen < (1LL << 31) && n_ref < (1LL << 31), S3D_ERR_INVALID, "eval_lp_max: bad sizes");
    S3D_CHECK(n_words >= 1 && n_words <= 512, S3D_ERR_INVALID, "eval_lp_max: %d words per patch, 1..512 (patch_size 2..32)", n_words);
    S3D_CHECK(n_gen == 0 || (gen_words && gen_counts && max_iou && max_f), S3D_ERR_INVALID, "eval_lp_max: null argument");
    S3D_CHECK(n_ref == 0 || (ref_words && ref_counts), S3D_ERR_INVALID, "eval_lp_max: null argument");
    if (!n_gen) return 0;
    hipStream_t st = static_cast<hipStream_t>(stream);
    S3D_HIP(hipMemsetAsync(max_iou, 0, size_t(n_gen) * sizeof(float), st));
    S3D_HIP(hipMemsetAsync(max_f, 0, size_t(n_gen) * sizeof(float), st));
    if (!n_ref) return 0;
    const long long gy = (n_gen + kLpGen - 1) / kLpGen;
    S3D_CHECK(gy <= 65535, S3D_ERR_UNSUPPORTED, "eval_lp_max: %lld generated patches, %d at most", (long long)n_gen, 65535 * kLpGen);
    hipLaunchKernelGGL(k_eval_lp_max, dim3(eval_blocks(n_ref), (unsigned)gy), dim3(kEvalThreads), 0, st,
                       reinterpret_cast<const unsigned long long*>(gen_words), gen_counts, (long long)n_gen,
                       reinterpret_cast<const unsigned long long*>(ref_words), ref_counts, (long long)n_ref, n_words,
                       reinterpret_cast<unsigned*>(max_iou), reinterpret_cast<unsigned*>(max_f));
    S3D_HIP(hipGetLastError());
    return 0;
}

int s3d_eval_pack_volumes(const uint8_t* vols, int64_t n, int64_t voxels, uint64_t* words, void* stream) {
    S3D_CHECK(n >= 0 && voxels >= 1 && voxels < (1LL << 31) && n <= 4096, S3D_ERR_INVALID, "eval_pack_volumes: bad sizes");
    S3D_CHECK(n == 0 || (vols && words), S3D_ERR_INVALID, "eval_pack_volumes: null argument");
    if (!n) return 0;
    const long long n_words = (voxels + 63) / 64;
    hipLaunchKernelGGL(k_eval_pack_volumes, dim3(eval_blocks(n * n_words * 64)), dim3(kEvalThreads), 0, static_cast<hipStream_t>(stream), vols,
                       (long long)n, (long long)voxels, n_words, reinterpret_cast<unsigned long long*>(words));
    S3D_HIP(hipGetLastError());
    return 0;
}

int s3d_eval_pairwise_counts(const uint64_t* words, int64_t n, int64_t n_words, int64_t* inter, int64_t* uni, void* stream) {
    S3D_CHECK(n >= 0 && n <= 4096 && n_words >= 1 && n_words < (1LL << 31), S3D_ERR_INVALID, "eval_pairwise_counts: bad sizes");
    S3D_CHECK(n == 0 || (words && inter && uni), S3D_ERR_INVALID, "eval_pairwise_counts: null argument");
    if (!n) return 0;
    hipLaunchKernelGGL(k_eval_pairwise_counts, dim3((unsigned)(n * n)), dim3(kEvalThreads), 0, static_cast<hipStream_t>(stream),
                       reinterpret_cast<const unsigned long long*>(words), int(n), (long long)n_words, reinterpret_cast<long long*>(inter),
                       reinterpret_cast<long long*>(uni));
    S3D_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
