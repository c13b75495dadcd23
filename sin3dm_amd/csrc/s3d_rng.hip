// s3d_rng.hip — torch's CPU noise stream generated on the MI355X.
//
// The reference samples on the CPU: x_T is one `th.randn(*shape)`, every step draws one `th.randn_like(x)`
// (src/diffusion/gaussian_diffusion.py:514, 431, 591), all from torch's default CPU generator.  That generator is MT19937
// and one float32 randn call of n >= 16 elements is
//   1. n tempered 32-bit outputs r_i, u_i = (r_i & 0xFFFFFF) * 2^-24;
//   2. for each full block of 16 (i = 0, 16, ... < n - n % 16), j < 8: u1 = 1 - u[i+j], u2 = u[i+j+8],
//      rad = sqrt(-2 log u1), th = 2 pi u2, out[i+j] = rad cos th, out[i+j+8] = rad sin th, all in float32;
//   3. if n % 16 != 0: 16 more outputs are drawn and out[n-16 : n] is recomputed from them by rule 2.
// Two kernels:
//   k_mt_walk    ONE workgroup.  x[k+624] = x[k+397] ^ twist(x[k], x[k+1]) is a serial recurrence whose nearest dependency
//                lies 227 words back, so a regeneration of the 624 state words is three dependent phases of <= 227 lanes
//                (words 0..226, 227..453, 454..623).  The state lives in LDS, twice (old / new block: a lane reads its
//                neighbour's old word while that neighbour writes its new one), one barrier per phase; every lane tempers the
//                word it has just made and stores it to the raw-word buffer.  Integer arithmetic only: exact.
//   k_mt_normal  chip-filling, elementwise: the 24-bit mask and rules 2 / 3 per call, 16-byte loads and stores, torch's operation
//                order in float32 with correctly rounded log / cos / sin (box_muller; this file is compiled without fast-math).
//   k_mt_uniform rule 1 alone (torch.rand).
#include "s3d_common.h"

namespace s3d {

constexpr int kMtN = 624, kMtM = 397, kMtLag = kMtN - kMtM;      // 227 independent new words per phase
#ifndef S3D_RNG_WALK_THREADS
#define S3D_RNG_WALK_THREADS 256                                  // one lane per word of a phase; 64 = one wave walking a phase in four passes (measured, slower)
#endif
constexpr int kWalkThreads = S3D_RNG_WALK_THREADS;

__device__ __forceinline__ uint32_t mt_temper(uint32_t y) {
    y ^= y >> 11;
    y ^= (y << 7) & 0x9d2c5680u;
    y ^= (y << 15) & 0xefc60000u;
    y ^= y >> 18;
    return y;
}

// key [624]: the state, read at entry and rewritten at exit.  pos: index of the next word (0..624).  The `words` next outputs of
// the stream go to raw[0 .. words).  regens = how many times the state is regenerated on the way = (pos + words - 1) / 624.
__global__ __launch_bounds__(kWalkThreads) void k_mt_walk(uint32_t* __restrict__ key, int pos, long long words, long long regens,
                                                          uint32_t* __restrict__ raw) {
    __shared__ uint32_t s[2][kMtN];
    const int tid = threadIdx.x;
    for (int k = tid; k < kMtN; k += kWalkThreads) s[0][k] = key[k];
    __syncthreads();
    // what is left of the current block
    for (long long k = pos + tid; k < kMtN && k - pos < words; k += kWalkThreads) raw[k - pos] = mt_temper(s[0][k]);
    int cur = 0;
    long long base = kMtN - pos;                                   // raw index of word 0 of the block being generated
    for (long long r = 0; r < regens; ++r, base += kMtN, cur ^= 1) {
        const uint32_t* __restrict__ o = s[cur];
        uint32_t* __restrict__ n = s[cur ^ 1];
#pragma unroll
        for (int ph = 0; ph < 3; ++ph) {
            for (int k = ph * kMtLag + tid; k < (ph + 1) * kMtLag && k < kMtN; k += kWalkThreads) {
                const uint32_t a = o[k];
                const uint32_t b = k == kMtN - 1 ? n[0] : o[k + 1];
                const uint32_t c = ph == 0 ? o[k + kMtM] : n[k - kMtLag];
                const uint32_t y = (a & 0x80000000u) | (b & 0x7fffffffu);
                const uint32_t v = c ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
                n[k] = v;
                if (base + k < words) raw[base + k] = mt_temper(v);
            }
            __syncthreads();
        }
    }
    for (int k = tid; k < kMtN; k += kWalkThreads) key[k] = s[cur][k];
}

__device__ __forceinline__ float mt_unit(uint32_t r) { return float(r & 0x00ffffffu) * 5.9604644775390625e-08f; }   // 2^-24: exact

__device__ __forceinline__ void box_muller(uint32_t r1, uint32_t r2, float& c, float& s) {
    const float u1 = 1.0f - mt_unit(r1);
    const float u2 = mt_unit(r2);
    // log / cos / sin are evaluated in double and rounded once: the correctly rounded float32 value, whatever the float32 library
    // forms of the toolchain do in their last bit.  Against torch's vectorised CPU forms that leaves ~83 % of the outputs bit-equal
    // (float32 library forms sit a few ulp away on more elements); the products and the square root are float32 as in torch.
    const float rad = sqrtf(-2.0f * float(log(double(u1))));
    const float th = 6.283185307179586f * u2;
    double sn, cs;
    sincos(double(th), &sn, &cs);
    c = rad * float(cs);
    s = rad * float(sn);
}

// One thread = four pairs of one block of 16: words [4h, 4h+4) and [4h+8, 4h+12) of the block, h = thread & 1.
// Per call: G = n / 16 full blocks read raw[16 g ..] and write out[16 g ..] below `limit` (= n - 16 when the call has a tail: the
// tail block owns out[n-16 : n)), then the tail block reads raw[n .. n+16) and writes out[n-16 ..).  VEC: n % 4 == 0 and
// both buffers 16-byte aligned.
template <bool VEC>
__global__ __launch_bounds__(256) void k_mt_normal(const uint32_t* __restrict__ raw, float* __restrict__ out, long long n,
                                                   long long words_per_call, long long units_per_call, long long total_units) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total_units) return;
    const long long call = t / units_per_call, u = t - call * units_per_call;
    const long long g = u >> 1, G = n >> 4;
    const int h = int(u & 1);
    const bool tail = g >= G;
    const uint32_t* src = raw + call * words_per_call + (tail ? n : g * 16) + 4 * h;
    const long long e0 = (tail ? n - 16 : g * 16) + 4 * h;          // element index of this thread's first cosine output
    const long long limit = (!tail && (n & 15)) ? n - 16 : n;
    float* dst = out + call * n + e0;
    uint32_t a[4], b[4];
    if (VEC) {
        const uint4 va = *reinterpret_cast<const uint4*>(src), vb = *reinterpret_cast<const uint4*>(src + 8);
        a[0] = va.x; a[1] = va.y; a[2] = va.z; a[3] = va.w;
        b[0] = vb.x; b[1] = vb.y; b[2] = vb.z; b[3] = vb.w;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) { a[j] = src[j]; b[j] = src[j + 8]; }
    }
    float c[4], s[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) box_muller(a[j], b[j], c[j], s[j]);
    if (VEC) {
        // n % 4 == 0: a float4 lies wholly on one side of `limit`
        if (e0 < limit) *reinterpret_cast<float4*>(dst) = make_float4(c[0], c[1], c[2], c[3]);
        if (e0 + 8 < limit) *reinterpret_cast<float4*>(dst + 8) = make_float4(s[0], s[1], s[2], s[3]);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (e0 + j < limit) dst[j] = c[j];
            if (e0 + j + 8 < limit) dst[j + 8] = s[j];
        }
    }
}

__global__ __launch_bounds__(256) void k_mt_uniform(const uint32_t* __restrict__ raw, float* __restrict__ out, long long n, int vec) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long i = t * 4;
    if (i >= n) return;
    if (vec && i + 4 <= n) {
        const uint4 v = *reinterpret_cast<const uint4*>(raw + i);
        *reinterpret_cast<float4*>(out + i) = make_float4(mt_unit(v.x), mt_unit(v.y), mt_unit(v.z), mt_unit(v.w));
    } else {
        for (long long k = i; k < n && k < i + 4; ++k) out[k] = mt_unit(raw[k]);
    }
}

}  // namespace s3d

using namespace s3d;

struct s3d_rng {
    DevBuf key, raw;               // 624 state words; the raw-word workspace
    uint32_t host_key[kMtN];       // staging of set_state (outlives the asynchronous copy)
    int pos = kMtN;
    bool seeded = false;
};

// enqueue the walker for the next `words` outputs and advance the host-side position
static int rng_walk(s3d_rng* r, long long words, hipStream_t st) {
    const long long end = (long long)r->pos + words;
    const long long regens = (end - 1) / kMtN;
    hipLaunchKernelGGL(k_mt_walk, dim3(1), dim3(kWalkThreads), 0, st, static_cast<uint32_t*>(r->key.p), r->pos, words, regens,
                       static_cast<uint32_t*>(r->raw.p));
    S3D_HIP(hipGetLastError());
    r->pos = int(end - regens * kMtN);
    return 0;
}

extern "C" {

int s3d_rng_create(s3d_rng** out) {
    S3D_CHECK(out, S3D_ERR_INVALID, "rng_create: null argument");
    s3d_rng* r = new s3d_rng();
    int rc = r->key.reserve(kMtN * sizeof(uint32_t));
    if (rc) { delete r; return rc; }
    *out = r;
    return 0;
}

void s3d_rng_destroy(s3d_rng* r) { delete r; }

int s3d_rng_set_state(s3d_rng* r, const uint32_t* key, int pos, void* stream) {
    S3D_CHECK(r && key, S3D_ERR_INVALID, "rng_set_state: null argument");
    S3D_CHECK(pos >= 0 && pos <= kMtN, S3D_ERR_INVALID, "rng_set_state: position %d outside 0..624", pos);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (r->seeded) S3D_HIP(hipStreamSynchronize(st));              // an earlier copy may still read the staging words
    memcpy(r->host_key, key, sizeof r->host_key);
    S3D_HIP(hipMemcpyAsync(r->key.p, r->host_key, sizeof r->host_key, hipMemcpyHostToDevice, st));
    r->pos = pos;
    r->seeded = true;
    return 0;
}

int s3d_rng_get_state(s3d_rng* r, uint32_t* key, int* pos, void* stream) {
    S3D_CHECK(r && key && pos, S3D_ERR_INVALID, "rng_get_state: null argument");
    S3D_CHECK(r->seeded, S3D_ERR_INVALID, "rng_get_state: no state was set");
    hipStream_t st = static_cast<hipStream_t>(stream);
    S3D_HIP(hipMemcpyAsync(key, r->key.p, kMtN * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    S3D_HIP(hipStreamSynchronize(st));
    *pos = r->pos;
    return 0;
}

int s3d_rng_reserve(s3d_rng* r, int64_t words) {
    S3D_CHECK(r && words >= 0, S3D_ERR_INVALID, "rng_reserve: bad argument");
    if (size_t(words) * sizeof(uint32_t) <= r->raw.cap) return 0;
    S3D_HIP(hipDeviceSynchronize());                               // launches that read the old workspace may be in flight
    return r->raw.reserve(size_t(words) * sizeof(uint32_t));
}

int s3d_rng_randn(s3d_rng* r, float* out, int64_t n, int n_calls, void* stream) {
    S3D_CHECK(r && out, S3D_ERR_INVALID, "rng_randn: null argument");
    S3D_CHECK(r->seeded, S3D_ERR_INVALID, "rng_randn: no state was set");
    S3D_CHECK(n_calls >= 1, S3D_ERR_INVALID, "rng_randn: n_calls = %d", n_calls);
    S3D_CHECK(n >= 16, S3D_ERR_UNSUPPORTED, "rng_randn: %lld elements per call: torch draws fewer than 16 through a "
              "double-precision path that is not implemented", (long long)n);
    const long long wpc = n + ((n & 15) ? 16 : 0), words = wpc * n_calls;
    S3D_CHECK(size_t(words) * sizeof(uint32_t) <= r->raw.cap, S3D_ERR_INVALID,
              "rng_randn: %lld raw words needed, %zu reserved (s3d_rng_reserve)", words, r->raw.cap / sizeof(uint32_t));
    hipStream_t st = static_cast<hipStream_t>(stream);
    S3D_TRY(rng_walk(r, words, st));
    const long long units = 2 * ((n >> 4) + ((n & 15) ? 1 : 0)), total = units * n_calls;
    const long long blocks = (total + 255) / 256;
    S3D_CHECK(blocks < (1ll << 31), S3D_ERR_INVALID, "rng_randn: %lld elements in one call", (long long)n * n_calls);
    const uint32_t* raw = static_cast<const uint32_t*>(r->raw.p);
    if ((n & 3) == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0)
        hipLaunchKernelGGL(k_mt_normal<true>, dim3((unsigned)blocks), dim3(256), 0, st, raw, out, (long long)n, wpc, units, total);
    else
        hipLaunchKernelGGL(k_mt_normal<false>, dim3((unsigned)blocks), dim3(256), 0, st, raw, out, (long long)n, wpc, units, total);
    S3D_HIP(hipGetLastError());
    return 0;
}

int s3d_rng_rand(s3d_rng* r, float* out, int64_t n, void* stream) {
    S3D_CHECK(r && out, S3D_ERR_INVALID, "rng_rand: null argument");
    S3D_CHECK(r->seeded, S3D_ERR_INVALID, "rng_rand: no state was set");
    S3D_CHECK(n >= 1, S3D_ERR_INVALID, "rng_rand: %lld elements", (long long)n);
    S3D_CHECK(size_t(n) * sizeof(uint32_t) <= r->raw.cap, S3D_ERR_INVALID,
              "rng_rand: %lld raw words needed, %zu reserved (s3d_rng_reserve)", (long long)n, r->raw.cap / sizeof(uint32_t));
    hipStream_t st = static_cast<hipStream_t>(stream);
    S3D_TRY(rng_walk(r, n, st));
    const long long blocks = ((n + 3) / 4 + 255) / 256;
    S3D_CHECK(blocks < (1ll << 31), S3D_ERR_INVALID, "rng_rand: %lld elements in one call", (long long)n);
    hipLaunchKernelGGL(k_mt_uniform, dim3((unsigned)blocks), dim3(256), 0, st, static_cast<const uint32_t*>(r->raw.p), out,
                       (long long)n, int((reinterpret_cast<uintptr_t>(out) & 15) == 0));
    S3D_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
