// s3d_wino24.hip — 3x3 TriplaneConv as a fused MIXED Winograd convolution F(2x4, 3x3) on the fp32 matrix cores:
// F(2,3) along the rows, F(4,3) along the columns.  A 4x6 input patch gives a 2x4 output tile through 24 "frequency"
// GEMMs: 3 multiplies per output instead of 4 (F(2x2,3x3), s3d_wino.hip) or 9 (direct) — 25 % fewer MFMA flops than
// k_conv_wino4 in a k-loop that was already matrix-pipe bound.
//
//   Y = A2^T [ (G2 g G4^T) .* (B2^T d B4) ] A4        B2/G2/A2: F(2,3) (points 0, +-1, inf),  B4/G4/A4: F(4,3) (0, +-1, +-2, inf)
//
// fp32 error against an fp64 direct convolution, measured on this network's layer shapes: 0.9-1.2e-6 relative
// (F(2x2): 2-3e-7, direct fp32: 2.5-4.7e-7, full F(4x4): 3.6-4.9e-6) — three decades inside the 1e-3 gate.
//
// Two blockings of one kernel source (s3d_wino24_block.h), same arithmetic in the same order (bit-identical results):
// k_conv_wino24s (8x16 pixels x 32 output channels per block, three blocks per CU — launches of one or two rounds of blocks) and
// k_conv_wino24w (x 64 output channels, two blocks per CU: one halo fetch + input transform feeds twice the MFMAs — multi-round
// launches); k_conv_wino24s_gnb is the first with the GroupNorm-backward epilogue of the training tier.  Round 2's 16x16-pixel form on
// v_mfma_f32_32x32x2_f32, round 3's persistent multi-tile form and the in-launch rank-1 producers were measured slower and are
// gone (profiles/r02_wino_ubench.txt, r03_wino_persistent.txt, r03_rank1_inline.txt).
#include "s3d_common.h"
#include "s3d_rank1.h"

namespace s3d {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kTabAux = 16;                         // buffer-instruction aux bit 4 = sc1 on the rank-1 table loads
__device__ __forceinline__ int x_edge_variant(int idx, int n) { return n == 1 ? 3 : (idx == 0 ? 1 : (idx == n - 1 ? 2 : 0)); }

// ------------------------------------------------------------------ the kernels: one source, s3d_wino24_block.h
#ifdef W24_TIMING
__device__ unsigned long long* g_w24time;     // tools/wino24_ubench.hip: per-block wall-clock stamps (entry, halo in LDS, first MFMA, last MFMA, images written, exit)
                                              // + the shader-clock counter at the two ends of the k-loop (slots 6, 7; tools/clock_probe.hip)
__device__ unsigned* g_w24id;                 // ... and where the block ran: XCC_ID << 16 | (HW_ID: CU 11:8, SH 12, SE 15:13)
#define W24_WHERE() ((__builtin_amdgcn_s_getreg((4 - 1) << 11 | 0 << 6 | 20) << 16) | (__builtin_amdgcn_s_getreg((16 - 1) << 11 | 0 << 6 | 4) & 0xFFFF))
#ifdef W24_WHERE_ID                           // (its own build: the extra registers at a block's start make k_conv_wino24s spill, 1.5x slower)
#define W24_NOTE_WHERE(k) if ((k) == 0 && g_w24id) g_w24id[blockIdx.x] = W24_WHERE();
#else
#define W24_NOTE_WHERE(k)
#endif
#define W24_STAMP(k) if (threadIdx.x == 0) { W24_NOTE_WHERE(k) g_w24time[size_t(blockIdx.x) * 8 + (k)] = wall_clock64(); \
        if ((k) == 2) g_w24time[size_t(blockIdx.x) * 8 + 6] = clock64(); if ((k) == 3) g_w24time[size_t(blockIdx.x) * 8 + 7] = clock64(); }
#else
#define W24_STAMP(k)
#endif
#ifndef W24W_RING
#define W24W_RING 8                                // weight fragments in flight per wave of the wide kernel (pairs: one per sub-block), each requested W24W_RING / 2 groups of 8 MFMAs ahead
#endif
constexpr int C_KC = 32, C_LD = C_KC + 4;
constexpr int C_TH = 8, C_TW = 16;
constexpr int C_HH = C_TH + 2, C_HW = C_TW + 2;
constexpr int C_ITEMS = C_HH * C_HW * (C_KC / 4);            // 1440 float4 items per chunk
constexpr int C_ITEMS_PT = (C_ITEMS + 255) / 256;            // 6 (the sixth round covers 160 items)
constexpr int C_ABUF = C_HH * C_HW * C_LD;                   // floats per halo buffer (6480)

// the three entry points: name, occupancy and signature here, the body from the one source (which #undefs its two parameters)
#define W24_NSUB 1
#define W24_GNB 0
__global__ __launch_bounds__(256, 3) void k_conv_wino24s(ConvArgs args)
#include "s3d_wino24_block.h"

#define W24_NSUB 1
#define W24_GNB 1
__global__ __launch_bounds__(256, 3) void k_conv_wino24s_gnb(ConvArgs args, GnbArgs gb)
#include "s3d_wino24_block.h"

#define W24_NSUB 2
#define W24_GNB 0
__global__ __launch_bounds__(256, 2) void k_conv_wino24w(ConvArgs args)
#include "s3d_wino24_block.h"

// ------------------------------------------------------------------ host side
static const double kG2[4][3] = {{1, 0, 0}, {0.5, 0.5, 0.5}, {0.5, -0.5, 0.5}, {0, 0, 1}};
static const double kG4[6][3] = {{1.0 / 4, 0, 0}, {-1.0 / 6, -1.0 / 6, -1.0 / 6}, {-1.0 / 6, 1.0 / 6, -1.0 / 6},
                                 {1.0 / 24, 1.0 / 12, 1.0 / 6}, {1.0 / 24, -1.0 / 12, 1.0 / 6}, {0, 0, 1}};

size_t wino24_packed_floats(int cout, int cin) { return size_t((cout + 31) / 32) * (cin / 8) * 24 * 256; }

// U = G2 g G4^T in double (explicit fma: host and device — s3d_pack.hip — round alike); W is OIHW [cout][ctot][3][3], only input
// channels [0, cin) are used (the plane's own channels).
// the small-block kernel's image: [n32][k16][24 freq][2 x 16 couts][64 lanes = 16 * channel quad + cout][4 channels]
size_t pack_wino24s_weights(std::vector<float>& stage, const float* W, int cout, int ctot, int cin) {
    const int k16t = cin / 16;
    const size_t total = wino24_packed_floats(cout, cin);
    const size_t off = push(stage, nullptr, total);
    float* d = stage.data() + off;
    std::fill(d, d + total, 0.f);
    for (int co = 0; co < cout; ++co)
        for (int c = 0; c < cin; ++c) {
            const float* g = W + (size_t(co) * ctot + c) * 9;
            double t[4][3];
            for (int u = 0; u < 4; ++u)
                for (int k = 0; k < 3; ++k) t[u][k] = kG2[u][0] * g[0 * 3 + k] + kG2[u][1] * g[1 * 3 + k] + kG2[u][2] * g[2 * 3 + k];
            const int nt = co >> 5, nb = (co >> 4) & 1, jn = co & 15, k16 = c >> 4, q = (c >> 2) & 3, e = c & 3;
            for (int u = 0; u < 4; ++u)
                for (int v = 0; v < 6; ++v) {
                    const double uv = fma(t[u][0], kG4[v][0], fma(t[u][1], kG4[v][1], t[u][2] * kG4[v][2]));    // explicit fma: host and device (s3d_pack.hip) round alike
                    d[((((size_t(nt) * k16t + k16) * 24 + (u * 6 + v)) * 2 + nb) * 64 + (q * 16 + jn)) * 4 + e] = float(uv);
                }
        }
    return off;
}


// the tiling of a launch, for cout_per_block = 32 / 64 output channels per block: fills the jobs' tile fields, returns the number of blocks
static int wino24s_layout(ConvArgs& a, int cout_per_block, const char* who) {
    int blocks = 0;
    for (int j = 0; j < a.njobs; ++j) {
        ConvJob& J = a.job[j];
        if (size_t(J.h) * J.w * a.cin * 4 >= (size_t(1) << 31)) { set_error("%s: a plane of one sample must stay below 2 GiB", who); return -1; }
        J.tiles_x = (J.w + C_TW - 1) / C_TW;
        J.tiles_per_img = J.tiles_x * ((J.h + C_TH - 1) / C_TH);
        J.n_tiles_n = (a.cout + cout_per_block - 1) / cout_per_block;
        J.block_begin = blocks;
        blocks += J.tiles_per_img * J.n_tiles_n * a.B;
    }
    return blocks;
}

// Which blocking a launch takes.  The two kernels are bit-identical, so the choice may depend on anything, the batch included.
// Measured in steady state on every layer shape x batch 1 / 2 / 4 / 8 (profiles/r04_wino_ubench.txt): the wide form wins from
// 1.5 rounds of its own blocks on (3 x CUs; two blocks per CU) when K >= 256 — that includes the 384 -> 128 layer of the batch-1
// step, 136 -> 127 us — and from 3 rounds on at K = 128 (a tie below); it loses on the one-round half-resolution launches of
// the batch-1 step (384 blocks on 512 slots) and at K = 64 (the k-loop is too short to amortise the 64-channel epilogue).
// S3D_WINO24W=0: never; =1: every launch whose cout is a multiple of 64.
static bool takes_wide(const ConvArgs& a) {
    const int mode = opt(OPT_WINO24W);
    if (mode == 0 || a.cout % 64 != 0) return false;
    if (mode == 1) return true;
    if (a.cin < 128) return false;
    ConvArgs wide = a;                                      // laid out as the wide kernel's launch, for its block count
    return wino24s_layout(wide, 64, "wino24w conv") >= (a.cin >= 256 ? 3 : 6) * device_cus();
}

// One launcher: the tiling for cout_per_block channels per block, the XCD-aware block order + raised priority outside the k-loop
// (xcd_swizzle; were switchable in rounds 1-2: always wins), the kernel's name for the profile, the launch.
// (round 5: an XCD owning one half of the channel blocks of a quarter of the tiles instead — half the weight image per L2, every
// halo fetched twice — measured the same step time and 3 % less traffic on config 3; not kept: profiles/r05_xcd_mapping.txt)
template <typename Kernel, typename... Extra>
static int launch_wino24(ConvArgs& a, hipStream_t st, int cout_per_block, bool args_ok, const char* who, const char* name, Kernel kernel, const Extra&... extra) {
    S3D_CHECK(args_ok && a.cin % C_KC == 0, S3D_ERR_INVALID, "%s: bad arguments", who);
    const int blocks = wino24s_layout(a, cout_per_block, who);
    if (blocks < 0) return S3D_ERR_INVALID;
    if (!blocks) return 0;
    a.xcd_swizzle = 1 | 2;
    conv_note_kernel(name);
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(256), 0, st, a, extra...);
    S3D_HIP(hipGetLastError());
    return 0;
}

int launch_conv_wino24_wide(ConvArgs& a, hipStream_t st) {
    return launch_wino24(a, st, 64, a.njobs >= 1 && a.njobs <= kMaxConvJobs && a.cout % 64 == 0, "wino24w conv",
                         "k_conv_wino24w mixed Winograd F(2x4,3x3), 8x16-pixel x 64-cout blocks", k_conv_wino24w);
}

int launch_conv_wino24_narrow(ConvArgs& a, hipStream_t st) {
    return launch_wino24(a, st, 32, a.njobs >= 1 && a.njobs <= kMaxConvJobs && a.cout % 4 == 0, "wino24s conv",
                         "k_conv_wino24s mixed Winograd F(2x4,3x3), 8x16-pixel blocks", k_conv_wino24s);
}

// the input-gradient convolution that also leaves the following GroupNorm backward's partial sums (k_conv_wino24s_gnb; always the
// 32-output-channel block: the sums' order must not depend on the launch size)
static int launch_conv_wino24_gnb(ConvArgs& a, const GnbArgs& gb, hipStream_t st) {
    return launch_wino24(a, st, 32, a.njobs == 3 && a.cout % 32 == 0 && gb.groups >= 1 && a.cout % gb.groups == 0, "wino24s gnb conv",
                         "k_conv_wino24s_gnb mixed Winograd F(2x4,3x3) + GroupNorm-backward partial sums, 8x16-pixel blocks", k_conv_wino24s_gnb, gb);
}

int launch_conv_wino24s(ConvArgs& a, hipStream_t st) {
    if (a.gnb) return launch_conv_wino24_gnb(a, *a.gnb, st);
    return takes_wide(a) ? launch_conv_wino24_wide(a, st) : launch_conv_wino24_narrow(a, st);
}

}  // namespace s3d
