// s3d_ae.hip — auto-encoder training tier: AutoEncoderGroupSkip encode + decode + losses and
// their backward pass on the MI355X, behind s3d_ae_* (include/sin3dm_hip.h).
//
// Reference: AutoEncoderGroupSkip (src/encoding/networks.py:122-220), TriplaneGroupResnetBlock / DecoderMLPSkipConcat
// (src/encoding/blocks.py:65-91, 189-256), ShapeAutoEncoder._forward_batch / update_network (src/encoding/model.py:178-237).
//
// One training iteration (what `net(input_grid, pts)` + `loss.backward()` do there):
//   encode   the Conv3d + axis means collapse to three 2-D convolutions over projections of the (fixed) input volume
//            (s3d_ae_kernels.hip) -> InstanceNorm2d -> tanh(x/2): the 12-channel triplane latent
//   planes   per feature group (geo 4 ch, tex 8 ch): conv5x5 -> InstanceNorm(affine) -> SiLU -> conv5x5 + 1x1 shortcut
//            on the MFMA convolution kernels (s3d_conv.hip)
//   points   bilinear border-clamped gather of the three planes, summed -> [N][64] per group
//   MLPs     DecoderMLPSkipConcat as 1x1 convolutions over the point list (fp32 MFMA); activations kept for the backward
//   losses   weighted-L1 sdf + masked texture loss (k_loss_*)
//   backward the same operators transposed: MLP dgrad (1x1 conv with W^T), MLP wgrad (k_wgrad_mfma<1>), scatter-add of the
//            point gradients onto the planes (points sorted by plane cell, then a per-pixel gather in that fixed order:
//            no float atomics, unlike PyTorch's grid_sampler backward), 5x5 dgrad / wgrad (k_wgrad_mfma<25>), InstanceNorm backward
//            (the GroupNorm backward with one channel per group), tanh/InstanceNorm backward and the encoder's weight
//            gradient as a 2-D correlation with the projections.
// Parameters: one flat fp32 device vector in the order [geo_encoder, geo_convs, geo_decoder | tex_encoder, tex_convs,
// tex_decoder] — the reference's two AdamW parameter groups (networks.py:146-150) are the two halves.
// Variants (s3d_ae_create_variant, the numbers of s3d_decoder_create_variant): 0 is the net above with 1..8 texture channels (a
// volume of 1 + tex_channels channels; 3 is sdftex, 8 sdfpbr on the skip net), 1 the geometry net alone (use_tex=False: one net,
// a 1-channel volume, no tex group), 2 — the PBR net — is refused there and made by s3d_ae_create_pbr: its iteration is ae_step_pbr
// (two 3x3 texture blocks, the second with an input norm that shares its parameters with the hidden norm, three heads on one gather).
// Every loop over the nets in ae_step runs to a->nnets.
#include <memory>

#include "s3d_ae.h"
#include "s3d_bwd.h"
#include "s3d_model.h"

namespace s3d {

static const char* kAePl[3] = {"xy", "xz", "yz"};

struct AeSpec { std::string name; std::vector<int64_t> shape; size_t numel() const { size_t n = 1; for (auto d : shape) n *= size_t(d); return n; } };

struct AeNet {
    int cin = 0, nout = 0;                                   // real feature channels (4 / 8), outputs (1 / tex_channels)
    size_t f_in_w, f_in_b, f_out_w, f_out_b, f_sc_w, f_sc_b, f_gamma[3], f_beta[3], f_mw[6], f_mb[6];   // flat offsets
    size_t in_dense[3], out_dense[3], sc_dense[3], in_T[3], out_T[3], sc_T[3], mT[5];                   // packed offsets
    int I[6], O[6];
    int ks = 5;                                              // plane-block kernel size (3 for the PBR net's texture blocks)
};
// the PBR net's texture side beyond its first block (which is net[1] at 3x3): tex_convs.1 and the three heads
struct AePbr {
    size_t f_in_w, f_in_b, f_out_w, f_out_b, f_gamma[3], f_beta[3];      // tex_convs.1 (no shortcut parameters)
    size_t in_dense[3], in_T[3], out_dense[3], out_T[3];
    struct Head { size_t f_mw[6], f_mb[6], mT[5]; int nout, ooff; } head[3];   // rgb | mr | normal: pred columns ooff .. ooff + nout
};

}  // namespace s3d

using namespace s3d;

struct s3d_ae {
    s3d_decoder_cfg cfg;
    int variant = 0;                    // s3d_decoder_create_variant's numbers: 0 skip net with texture, 1 geometry only (tex = TC = 0, C = 1, one net)
    int geo, tex, up, hid, TC, C, nnets = 2;
    std::vector<AeSpec> specs;
    std::vector<size_t> flat_off;
    int64_t tex_begin = 0;
    float* flat = nullptr;
    AeNet net[2];
    AePbr pbr;                          // variant 2 only
    size_t f_enc_w[2], f_enc_b[2];
    // packed image
    DevBuf pbuf, descs_dev;
    std::vector<PackDesc> descs;
    int pack_blocks = 0;
    size_t wp_off = 0, encb_off = 0, psize = 0;
    // volume projections
    DevBuf proj;
    EncDesc enc{};
    bool has_volume = false;
    Arena arena;
    // backward pass: weight-gradient launches (no consumer before the optimizer) on a handle-owned low-priority side stream, beside
    // the chain of input gradients — as in the denoiser's backward pass (s3d_train.hip: Bwd::edge / join)
    hipStream_t side = nullptr;
    hipStream_t chain2 = nullptr;       // the texture MLP's backward chain beside the geometry MLP's (the two nets only meet at the scatter)
    std::vector<hipEvent_t> events;
    ~s3d_ae() {
        for (auto e : events) (void)hipEventDestroy(e);
        if (side) (void)hipStreamDestroy(side);
        if (chain2) (void)hipStreamDestroy(chain2);
    }
    const float* P(size_t off) const { return static_cast<const float*>(pbuf.p) + off; }
    size_t off_of(const std::string& n) const {
        for (size_t i = 0; i < specs.size(); ++i) if (specs[i].name == n) return flat_off[i];
        return size_t(-1);
    }
};

namespace s3d {

static void ae_specs(s3d_ae* a) {
    const int up = a->up, hid = a->hid;
    auto add = [&](const std::string& n, std::vector<int64_t> s) { a->specs.push_back({n, std::move(s)}); };
    const char* pre[2] = {"geo", "tex"};
    const int cin[2] = {a->geo, a->tex}, cout[2] = {1, a->TC}, encin[2] = {1, a->C};
    const char* ln[6] = {".first_layers.0", ".first_layers.2", ".first_layers.4", ".second_layers.0", ".second_layers.2", ".second_layers.4"};
    auto mlp = [&](const std::string& ml, int nout) {
        const int I[6] = {up, hid, hid, up + hid, hid, hid}, O[6] = {hid, hid, hid, hid, hid, nout};
        for (int l = 0; l < 6; ++l) { add(ml + ln[l] + ".weight", {O[l], I[l]}); add(ml + ln[l] + ".bias", {O[l]}); }
    };
    for (int k = 0; k < a->nnets; ++k) {
        if (k == 1) { int64_t n = 0; for (auto& s : a->specs) n += int64_t(s.numel()); a->tex_begin = n; }
        const bool pbr = a->variant == 2 && k == 1;          // the PBR net's texture side: two 3x3 blocks, three heads
        const int ks = pbr ? 3 : 5;
        const std::string e = std::string(pre[k]) + "_encoder", cv = std::string(pre[k]) + (pbr ? "_convs.0" : "_convs"), ml = std::string(pre[k]) + "_decoder";
        add(e + ".weight", {cin[k], encin[k], 4, 4, 4}); add(e + ".bias", {cin[k]});
        add(cv + ".in_layers.0.weight", {3 * up, cin[k], ks, ks}); add(cv + ".in_layers.0.bias", {3 * up});
        for (int p = 0; p < 3; ++p) { add(cv + ".norm_" + kAePl[p] + ".weight", {up}); add(cv + ".norm_" + kAePl[p] + ".bias", {up}); }
        add(cv + ".out_layers.1.weight", {3 * up, up, ks, ks}); add(cv + ".out_layers.1.bias", {3 * up});
        add(cv + ".shortcut.weight", {3 * up, cin[k], 1, 1}); add(cv + ".shortcut.bias", {3 * up});
        if (!pbr) { mlp(ml, cout[k]); continue; }
        const std::string c1 = "tex_convs.1";
        add(c1 + ".in_layers.1.weight", {3 * up, up, 3, 3}); add(c1 + ".in_layers.1.bias", {3 * up});
        for (int p = 0; p < 3; ++p) { add(c1 + ".norm_" + kAePl[p] + ".weight", {up}); add(c1 + ".norm_" + kAePl[p] + ".bias", {up}); }
        add(c1 + ".out_layers.1.weight", {3 * up, up, 3, 3}); add(c1 + ".out_layers.1.bias", {3 * up});
        mlp("rgb_decoder", 3); mlp("mr_decoder", 2); mlp("normal_decoder", 3);
    }
    a->flat_off.resize(a->specs.size());
    size_t off = 0;
    for (size_t i = 0; i < a->specs.size(); ++i) { a->flat_off[i] = off; off += a->specs[i].numel(); }
    if (a->nnets == 1) a->tex_begin = int64_t(off);          // no tex group: it begins where the vector ends
}

static int ae_plan(s3d_ae* a) {
    const int up = a->up, hid = a->hid;
    size_t ps = 0;
    auto palloc = [&](size_t n) { size_t o = (ps + 63) & ~size_t(63); ps = o + n; return o; };
    auto add = [&](int kind, size_t src, size_t dst, long long n, int cout = 0, int ctot = 0, int cin = 0, int taps = 0, int slot = 0) {
        PackDesc d{};
        d.kind = kind; d.cout = cout; d.ctot = ctot; d.cin = cin; d.slot = slot; d.taps = taps; d.src = (long long)src; d.dst = (long long)dst; d.n = n;
        a->descs.push_back(d);
    };
    a->descs.clear();
    const char* pre[2] = {"geo", "tex"};
    const int cin[2] = {a->geo, a->tex}, cout[2] = {1, a->TC};
    a->encb_off = palloc(a->geo + a->tex);
    a->wp_off = palloc(size_t(3) * (a->geo + a->tex) * 16 * 4 * a->C);
    const char* ln[6] = {".first_layers.0", ".first_layers.2", ".first_layers.4", ".second_layers.0", ".second_layers.2", ".second_layers.4"};
    for (int k = 0; k < a->nnets; ++k) {
        AeNet& N = a->net[k];
        N.cin = cin[k]; N.nout = cout[k];
        const bool pbr = a->variant == 2 && k == 1;
        const int T = pbr ? 9 : 25;
        N.ks = pbr ? 3 : 5;
        const std::string e = std::string(pre[k]) + "_encoder", cv = std::string(pre[k]) + (pbr ? "_convs.0" : "_convs"), ml = std::string(pre[k]) + "_decoder";
        a->f_enc_w[k] = a->off_of(e + ".weight"); a->f_enc_b[k] = a->off_of(e + ".bias");
        add(PK_COPY, a->f_enc_b[k], a->encb_off + (k == 0 ? 0 : a->geo), cin[k]);
        N.f_in_w = a->off_of(cv + ".in_layers.0.weight"); N.f_in_b = a->off_of(cv + ".in_layers.0.bias");
        N.f_out_w = a->off_of(cv + ".out_layers.1.weight"); N.f_out_b = a->off_of(cv + ".out_layers.1.bias");
        N.f_sc_w = a->off_of(cv + ".shortcut.weight"); N.f_sc_b = a->off_of(cv + ".shortcut.bias");
        for (int p = 0; p < 3; ++p) {
            N.f_gamma[p] = a->off_of(cv + ".norm_" + kAePl[p] + ".weight"); N.f_beta[p] = a->off_of(cv + ".norm_" + kAePl[p] + ".bias");
            const size_t win = N.f_in_w + size_t(p) * up * cin[k] * T, wout = N.f_out_w + size_t(p) * up * up * T, wsc = N.f_sc_w + size_t(p) * up * cin[k];
            N.in_dense[p] = palloc(size_t(T) * up * 32); add(PK_DENSE_PAD, win, N.in_dense[p], (long long)T * up * cin[k], up, cin[k], cin[k], T, 32);
            N.in_T[p] = palloc(size_t(T) * 32 * up);     add(PK_DENSE_T_PAD, win, N.in_T[p], (long long)T * up * cin[k], up, cin[k], cin[k], T, 32);
            N.out_dense[p] = palloc(size_t(T) * up * up); add(PK_DENSE, wout, N.out_dense[p], (long long)up * up, up, up, up, T);
            N.out_T[p] = palloc(size_t(T) * up * up);    add(PK_DENSE_T, wout, N.out_T[p], (long long)up * up, up, up, up, T);
            N.sc_dense[p] = palloc(size_t(up) * 32);      add(PK_DENSE_PAD, wsc, N.sc_dense[p], (long long)up * cin[k], up, cin[k], cin[k], 1, 32);
            N.sc_T[p] = palloc(size_t(32) * up);          add(PK_DENSE_T_PAD, wsc, N.sc_T[p], (long long)up * cin[k], up, cin[k], cin[k], 1, 32);
        }
        const int I[6] = {up, hid, hid, up + hid, hid, hid}, O[6] = {hid, hid, hid, hid, hid, cout[k]};
        for (int l = 0; l < 6; ++l) { N.I[l] = I[l]; N.O[l] = O[l]; }
        if (!pbr) {
            for (int l = 0; l < 6; ++l) {
                N.f_mw[l] = a->off_of(ml + ln[l] + ".weight"); N.f_mb[l] = a->off_of(ml + ln[l] + ".bias");
                if (l < 5) { N.mT[l] = palloc(size_t(I[l]) * O[l]); add(PK_TRANS2D, N.f_mw[l], N.mT[l], (long long)I[l] * O[l], O[l], 0, I[l]); }
            }
            continue;
        }
        AePbr& Q = a->pbr;
        const std::string c1 = "tex_convs.1";
        Q.f_in_w = a->off_of(c1 + ".in_layers.1.weight"); Q.f_in_b = a->off_of(c1 + ".in_layers.1.bias");
        Q.f_out_w = a->off_of(c1 + ".out_layers.1.weight"); Q.f_out_b = a->off_of(c1 + ".out_layers.1.bias");
        for (int p = 0; p < 3; ++p) {
            Q.f_gamma[p] = a->off_of(c1 + ".norm_" + kAePl[p] + ".weight"); Q.f_beta[p] = a->off_of(c1 + ".norm_" + kAePl[p] + ".bias");
            const size_t win = Q.f_in_w + size_t(p) * up * up * 9, wout = Q.f_out_w + size_t(p) * up * up * 9;
            Q.in_dense[p] = palloc(size_t(9) * up * up);  add(PK_DENSE, win, Q.in_dense[p], (long long)up * up, up, up, up, 9);
            Q.in_T[p] = palloc(size_t(9) * up * up);      add(PK_DENSE_T, win, Q.in_T[p], (long long)up * up, up, up, up, 9);
            Q.out_dense[p] = palloc(size_t(9) * up * up); add(PK_DENSE, wout, Q.out_dense[p], (long long)up * up, up, up, up, 9);
            Q.out_T[p] = palloc(size_t(9) * up * up);     add(PK_DENSE_T, wout, Q.out_T[p], (long long)up * up, up, up, up, 9);
        }
        const char* hn[3] = {"rgb_decoder", "mr_decoder", "normal_decoder"};
        const int hout[3] = {3, 2, 3}, hoff[3] = {1, 4, 6};
        for (int j = 0; j < 3; ++j) {
            AePbr::Head& Hd = Q.head[j];
            Hd.nout = hout[j]; Hd.ooff = hoff[j];
            for (int l = 0; l < 6; ++l) {
                Hd.f_mw[l] = a->off_of(std::string(hn[j]) + ln[l] + ".weight"); Hd.f_mb[l] = a->off_of(std::string(hn[j]) + ln[l] + ".bias");
                if (l < 5) { Hd.mT[l] = palloc(size_t(I[l]) * O[l]); add(PK_TRANS2D, Hd.f_mw[l], Hd.mT[l], (long long)I[l] * O[l], O[l], 0, I[l]); }
            }
        }
    }
    a->psize = ps;
    S3D_TRY(a->pbuf.reserve(ps * sizeof(float)));
    S3D_HIP(hipMemset(a->pbuf.p, 0, ps * sizeof(float)));
    S3D_TRY(finalize_pack_plan(a->descs, a->descs_dev, a->pack_blocks));
    return 0;
}

struct AeRun {
    s3d_ae* a; hipStream_t st; float* grads;
    hipStream_t sw = nullptr;             // weight gradients; `side` says whether it is a stream of its own (the caller's stream may be the null stream)
    bool side = false;
    size_t ev_next = 0;
    Arena& ar() { return a->arena; }
    bool meas() { return a->arena.measuring; }
    int edge(hipStream_t from, hipStream_t to) {           // `to` waits for what has been enqueued on `from` so far
        if (!side || from == to) return 0;
        if (ev_next == a->events.size()) {
            hipEvent_t e = nullptr;
            S3D_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
            a->events.push_back(e);
        }
        hipEvent_t e = a->events[ev_next++];
        S3D_HIP(hipEventRecord(e, from));
        S3D_HIP(hipStreamWaitEvent(to, e, 0));
        return 0;
    }
    const float* F(size_t off) const { return a->flat + off; }
    float* G(size_t off) const { return grads ? grads + off : reinterpret_cast<float*>(uintptr_t(256)); }

    int conv(ConvKind kind, int cin, int cout, const Geo& g, float* const in[3], const float* const wgt[3], const float* const bias[3],
             float* const res[3], float* const out[3], int njobs = 3, bool relu = false, hipStream_t on = nullptr, bool use_on = false) {
        if (meas()) return 0;
        ConvArgs ca; memset(&ca, 0, sizeof ca);
        ca.B = 1; ca.cin = cin; ca.cout = cout; ca.njobs = njobs; ca.relu = relu ? 1 : 0;
        for (int p = 0; p < njobs; ++p) {
            ConvJob& J = ca.job[p];
            J.in = in[p]; J.wgt = wgt[p]; J.bias = bias ? bias[p] : nullptr; J.res = res ? res[p] : nullptr; J.out = out[p];
            J.h = g.h[p]; J.w = g.w[p];
        }
        return launch_conv(kind, ca, use_on ? on : st);
    }
    // the point list as up to kMaxConvJobs 1x1 jobs of one launch (the PBR net's four MLPs advance a layer per launch; Geo has three slots)
    int lin_jobs(int cin, int cout, long long Np, int njobs, float* const in[], const float* const wgt[], const float* const bias[],
                 float* const out[], bool relu, hipStream_t on) {
        if (meas()) return 0;
        ConvArgs ca; memset(&ca, 0, sizeof ca);
        ca.B = 1; ca.cin = cin; ca.cout = cout; ca.njobs = njobs; ca.relu = relu ? 1 : 0;
        for (int j = 0; j < njobs; ++j) {
            ConvJob& J = ca.job[j];
            J.in = in[j]; J.wgt = wgt[j]; J.bias = bias ? bias[j] : nullptr; J.out = out[j];
            J.h = int(Np / 64); J.w = 64;
        }
        return launch_conv(CONV_1x1, ca, on);
    }
    // from / use_from: the stream dy was produced on when it is not the caller's (the second MLP chain)
    int wgrad(int taps, int cin, int cin_store, int cout, const Geo& g, float* const dy[3], int a_cstride, float* const act[3],
              float* const dW[3], int nplanes = 3, hipStream_t from = nullptr, bool use_from = false) {
        WgradArgs w;
        w.dy.C = cout; w.a.C = a_cstride; w.dy.g = w.a.g = g;
        for (int p = 0; p < 3; ++p) { w.dy.p[p] = p < nplanes ? dy[p] : nullptr; w.a.p[p] = p < nplanes ? act[p] : nullptr; }
        w.B = 1; w.cin = cin; w.cout = cout; w.ctot = cin_store; w.taps = taps; w.cin_store = cin_store; w.nplanes = nplanes;
        w.ksplit = wgrad_ksplit(g, 1, cin, cout, taps);
        for (int p = 0; p < nplanes; ++p) { w.part[p] = ar().alloc<float>(wgrad_part_floats(w.ksplit, cin, cout, taps)); w.dW[p] = dW[p]; }
        if (meas()) return 0;
        hipStream_t src = use_from ? from : st;
        hipStream_t on = side ? sw : src;
        S3D_TRY(edge(src, on));                            // dy and the activation are final in the order of the stream that produced them
        return launch_wgrad(w, on, &tail);                 // (the split-K partials stay in the arena; every reduction of the pass in ONE launch at its end)
    }
    DeferredTail tail;
};

// encode: projections -> pre-activation planes -> InstanceNorm + tanh.  pre/feat: NHWC [hw][CO] per plane
static int ae_encode(AeRun& R, float* pre[3], float* feat[3], float* mr) {
    s3d_ae* a = R.a;
    if (R.meas()) return 0;
    S3D_TRY(launch_enc_pack(R.F(a->f_enc_w[0]), a->nnets == 2 ? R.F(a->f_enc_w[1]) : nullptr, a->geo, a->tex, a->C, static_cast<float*>(a->pbuf.p) + a->wp_off, R.st));
    S3D_TRY(launch_enc_fwd(a->enc, a->P(a->wp_off), a->P(a->encb_off), pre, R.st));
    return launch_enc_norm(false, pre, feat, mr, nullptr, nullptr, a->enc.g, a->enc.CO, nullptr, R.st);
}

// Forward + (when grads != null) backward of one batch of points.  pred: [N][1+TC] output.
static int ae_step(s3d_ae* a, const float* pts, const float* sdf, const float* tex, long long N, const float aabb[6],
                   const s3d_ae_loss_cfg& lc, bool groups, float* losses, float* pred_out, float* grads, hipStream_t st) {
    AeRun R{a, st, grads};
    Arena& ar = a->arena;
    const bool meas = ar.measuring;
    ar.reset();
    if (!meas && grads && opt_on(OPT_BWD_SIDE)) {
        if (!a->side) {
            int least = 0, greatest = 0;
            (void)hipDeviceGetStreamPriorityRange(&least, &greatest);
            S3D_HIP(hipStreamCreateWithPriority(&a->side, hipStreamNonBlocking, least));
        }
        if (!a->chain2) S3D_HIP(hipStreamCreateWithFlags(&a->chain2, hipStreamNonBlocking));
        R.sw = a->side;
        R.side = true;
    }
    const int up = a->up, hid = a->hid, CO = a->geo + a->tex, S = 1 + a->TC, NN = a->nnets;
    const bool two = NN == 2;                               // (the second chain exists with a second net only)
    const Geo g = a->enc.g;
    const long long Np = (N + 63) / 64 * 64;
    const bool bwd = grads != nullptr || meas;              // the measuring pass sizes the workspace for both
    size_t hw[3];
    for (int p = 0; p < 3; ++p) hw[p] = size_t(g.h[p]) * g.w[p];

    // ---- encode
    float *pre[3], *feat[3];
    for (int p = 0; p < 3; ++p) { pre[p] = ar.alloc<float>(hw[p] * CO); feat[p] = ar.alloc<float>(hw[p] * CO); }
    float* enc_mr = ar.alloc<float>(size_t(3) * CO * 2);
    S3D_TRY(ae_encode(R, pre, feat, enc_mr));

    // ---- plane blocks
    struct NetAct { float *x[3], *a1[3], *y[3], *s[3], *f[3], *mr; double* part[3]; } A[2];
    // (training with the side streams on: the texture net's plane blocks run as a second chain beside the geometry net's — they
    // share nothing but the encoder's feature planes — here, and again in the backward pass)
    if (!meas && R.side && two) S3D_TRY(R.edge(st, a->chain2));
    for (int n = 0; n < NN; ++n) {
        const AeNet& N_ = a->net[n];
        NetAct& T = A[n];
        const bool second = n == 1 && R.side && !meas;
        hipStream_t cs = second ? a->chain2 : st;
        for (int p = 0; p < 3; ++p) {
            T.x[p] = ar.alloc<float>(hw[p] * 32); T.a1[p] = ar.alloc<float>(hw[p] * up); T.y[p] = ar.alloc<float>(hw[p] * up);
            T.s[p] = ar.alloc<float>(hw[p] * up); T.f[p] = ar.alloc<float>(hw[p] * up);
            T.part[p] = ar.alloc<double>(size_t(kInNormChunks) * up * 2);
        }
        T.mr = ar.alloc<float>(size_t(3) * up * 2);
        const float *w_in[3], *b_in[3], *w_out[3], *b_out[3], *w_sc[3], *b_sc[3];
        for (int p = 0; p < 3; ++p) {
            w_in[p] = a->P(N_.in_dense[p]); b_in[p] = R.F(N_.f_in_b + size_t(p) * up);
            w_out[p] = a->P(N_.out_dense[p]); b_out[p] = R.F(N_.f_out_b + size_t(p) * up);
            w_sc[p] = a->P(N_.sc_dense[p]); b_sc[p] = R.F(N_.f_sc_b + size_t(p) * up);
        }
        if (!meas) S3D_TRY(launch_slice_pad_nhwc3(feat, T.x, hw, CO, n == 0 ? 0 : a->geo, N_.cin, cs));
        S3D_TRY(R.conv(CONV_5x5, 32, up, g, T.x, w_in, b_in, nullptr, T.a1, 3, false, cs, true));
        if (!meas) {
            const float *gam[3], *bet[3];
            for (int p = 0; p < 3; ++p) { gam[p] = R.F(N_.f_gamma[p]); bet[p] = R.F(N_.f_beta[p]); }
            S3D_TRY(launch_inorm_silu3(T.a1, T.part, gam, bet, T.y, hw, up, 1e-6f, T.mr, cs));
        }
        S3D_TRY(R.conv(CONV_1x1, 32, up, g, T.x, w_sc, b_sc, nullptr, T.s, 3, false, cs, true));
        S3D_TRY(R.conv(CONV_5x5, up, up, g, T.y, w_out, b_out, T.s, T.f, 3, false, cs, true));
    }
    if (!meas && R.side && two) S3D_TRY(R.edge(a->chain2, st));   // the gather reads both nets' planes
    // (measured and not kept: the backward scatter's point sort — 21 small dependent launches that depend on the points alone —
    // enqueued here on the second chain's stream, beside the MLPs' forward pass: every one of them waits for a slot behind the
    // 8192-block launches of that pass, the chain arrives late at its backward half, 5.00 -> 5.30 ms/iteration)
    PointSet ps; ps.pts = pts; ps.N = N; ps.Np = Np;
    for (int k = 0; k < 6; ++k) ps.aabb[k] = aabb[k];

    // ---- points: gather, MLPs
    float *X0[2] = {nullptr, nullptr}, *H[2][5], *CAT[2];
    for (int n = 0; n < NN; ++n) {
        X0[n] = ar.alloc<float>(size_t(Np) * up);
        for (int l = 0; l < 5; ++l) H[n][l] = ar.alloc<float>(size_t(Np) * hid);
        CAT[n] = ar.alloc<float>(size_t(Np) * (up + hid));
    }
    float* pred = ar.alloc<float>(size_t(Np) * S);
    Geo gp; for (int p = 0; p < 3; ++p) { gp.h[p] = p < NN ? int(Np / 64) : 0; gp.w[p] = p < NN ? 64 : 0; }   // the point list as two "planes" (geo, tex)
    auto lin = [&](int l, float* const in[2], float* const out[2]) -> int {       // both groups in one launch
        const float *w[3], *b[3];
        float *i3[3], *o3[3];
        for (int n = 0; n < NN; ++n) { w[n] = R.F(a->net[n].f_mw[l]); b[n] = R.F(a->net[n].f_mb[l]); i3[n] = in[n]; o3[n] = out[n]; }
        return R.conv(CONV_1x1, a->net[0].I[l], a->net[0].O[l], gp, i3, w, b, nullptr, o3, NN, /*relu=*/true);
    };
    if (!meas) {
        const float* fp[2][3] = {};
        for (int n = 0; n < NN; ++n) for (int p = 0; p < 3; ++p) fp[n][p] = A[n].f[p];
        S3D_TRY(launch_gather(ps, fp, g.h, g.w, up, NN, X0, st));
    }
    {
        float *h0[2], *h1[2], *h2[2], *h3[2], *h4[2];
        for (int n = 0; n < 2; ++n) { const int m = n < NN ? n : 0; h0[n] = H[m][0]; h1[n] = H[m][1]; h2[n] = H[m][2]; h3[n] = H[m][3]; h4[n] = H[m][4]; }
        S3D_TRY(lin(0, X0, h0)); S3D_TRY(lin(1, h0, h1)); S3D_TRY(lin(2, h1, h2));
        if (!meas)
            for (int n = 0; n < NN; ++n) {
                S3D_TRY(launch_copy_slice(X0[n], 1, up, int(Np / 64), 64, CAT[n], up + hid, 0, st));
                S3D_TRY(launch_copy_slice(H[n][2], 1, hid, int(Np / 64), 64, CAT[n], up + hid, up, st));
            }
        S3D_TRY(lin(3, CAT, h3)); S3D_TRY(lin(4, h3, h4));
        if (!meas)
            for (int n = 0; n < NN; ++n)
                S3D_TRY(launch_last_fwd(H[n][4], R.F(a->net[n].f_mw[5]), R.F(a->net[n].f_mb[5]), hid, a->net[n].nout, n == 1, pred, S,
                                        n == 0 ? 0 : 1, N, st));
    }
    if (!meas && pred_out) S3D_HIP(hipMemcpyAsync(pred_out, pred, size_t(N) * S * sizeof(float), hipMemcpyDeviceToDevice, st));

    // ---- losses and d loss / d (pre-activation outputs)
    float* loss_ws = ar.alloc<float>(512);
    float* loss3 = ar.alloc<float>(8);
    float* dout = bwd ? ar.alloc<float>(size_t(Np) * S) : nullptr;
    if (!meas && sdf && groups) {
        // sdfpbr's eight material channels are three means (rgb | metallic-roughness | normal); any other width is one group, none is sdf
        const int gb8[4] = {0, 3, 5, 8}, gb1[4] = {0, a->TC, 0, 0};
        const int ng = a->TC == 8 ? 3 : (a->TC ? 1 : 0);
        S3D_TRY(launch_ae_loss_groups(pred, sdf, tex, N, Np, a->TC, ng, a->TC == 8 ? gb8 : gb1, /*sigm=*/1, lc.sdf_loss, lc.tex_loss,
                                      lc.sdf_threshold * lc.tex_threshold_ratio, lc.tex_weight, loss_ws, loss3, grads ? dout : nullptr, st));
        if (losses) S3D_HIP(hipMemcpyAsync(losses, loss3, 4 * sizeof(float), hipMemcpyDeviceToDevice, st));
    } else if (!meas && sdf) {
        S3D_TRY(launch_ae_loss(pred, sdf, tex, N, Np, a->TC, lc.sdf_loss, lc.tex_loss, lc.sdf_threshold * lc.tex_threshold_ratio,
                               lc.tex_weight, loss_ws, loss3, grads ? dout : nullptr, st));
        if (losses) S3D_HIP(hipMemcpyAsync(losses, loss3, 2 * sizeof(float), hipMemcpyDeviceToDevice, st));
    }
    if (!bwd) return 0;

    // ================================================================= backward
    // ---- MLPs
    float* dX0[2];
    float* cws = ar.alloc<float>(colsum_ws_floats(std::max(hid, up)));
    float* cws2 = ar.alloc<float>(3 * colsum_ws_floats(up));       // the plane blocks' bias sums (side stream, three planes per launch) have a workspace of their own
    // The two MLPs' backward chains are independent until the scatter: the texture net's runs on a second stream beside the
    // geometry net's (side-stream builds only) — each alternates a bandwidth-bound ReLU backward with an MFMA-bound 1x1 dgrad, so
    // the two chains want different things at most times.  Same kernels on the same operands: same bits.
    float* cws_n[2] = {cws, ar.alloc<float>(colsum_ws_floats(std::max(hid, up)))};
    if (!meas && R.side && two) S3D_TRY(R.edge(st, a->chain2));
    // (issued layer by layer for BOTH nets, not net after net: the two chains then advance together however far the host is ahead)
    struct Step { int l; float* act; float* in; int in_stride; float* din; const float* dact; int dstride, coff; };
    Step steps[2][5];
    float *dXa_n[2], *dCAT_n[2];
    hipStream_t cs_n[2];
    for (int n = 0; n < NN; ++n) {
        const AeNet& N_ = a->net[n];
        cs_n[n] = n == 1 && R.side && !meas ? a->chain2 : st;      // this net's chain
        float* dH = ar.alloc<float>(size_t(Np) * hid);            // gradient of a hidden activation (reused)
        float* dCAT = ar.alloc<float>(size_t(Np) * (up + hid));
        float* dXa = ar.alloc<float>(size_t(Np) * up);
        dX0[n] = ar.alloc<float>(size_t(Np) * up);
        dXa_n[n] = dXa; dCAT_n[n] = dCAT;
        float* lws = ar.alloc<float>(last_bwd_ws_floats(hid, N_.nout));
        if (!meas) S3D_TRY(launch_last_bwd(dout, S, n == 0 ? 0 : 1, R.F(N_.f_mw[5]), H[n][4], hid, N_.nout, Np, dH, lws, R.G(N_.f_mw[5]), R.G(N_.f_mb[5]), cs_n[n]));
        // hidden layers 4..0: dP = dH * relu'(H_l) ; db_l = colsum(dP) ; dW_l = dP^T in_l ; d in_l = dP W_l
        const Step st5[5] = {{4, H[n][4], H[n][3], hid, dH, dH, hid, 0},
                             {3, H[n][3], CAT[n], up + hid, dCAT, dH, hid, 0},
                             {2, H[n][2], H[n][1], hid, dH, dCAT, up + hid, up},
                             {1, H[n][1], H[n][0], hid, dH, dH, hid, 0},
                             {0, H[n][0], X0[n], up, dXa, dH, hid, 0}};
        for (int k = 0; k < 5; ++k) steps[n][k] = st5[k];
    }
    for (int kk = 0; kk < 5 * NN; ++kk) {
            const int k = kk / NN, n = kk % NN;
            const AeNet& N_ = a->net[n];
            const Step& s = steps[n][k];
            hipStream_t cs = cs_n[n];
            const int I = N_.I[s.l], O = N_.O[s.l];
            // gradient of the layer's pre-activation: one buffer per layer — the weight gradient that reads it runs on the side
            // stream while this chain has moved on
            float* dP = ar.alloc<float>(size_t(Np) * hid);
            if (!meas) S3D_TRY(launch_relu_bwd(s.dact, s.dstride, s.coff, s.act, dP, Np, O, cws_n[n], R.G(N_.f_mb[s.l]), cs));
            Geo g1; for (int p = 0; p < 3; ++p) { g1.h[p] = p == 0 ? int(Np / 64) : 0; g1.w[p] = p == 0 ? 64 : 0; }
            float* dy3[3] = {dP, nullptr, nullptr}; float* a3[3] = {s.in, nullptr, nullptr}; float* dw3[3] = {R.G(N_.f_mw[s.l]), nullptr, nullptr};
            S3D_TRY(R.wgrad(1, I, I, O, g1, dy3, s.in_stride, a3, dw3, 1, cs, true));
            const float* wT[3] = {a->P(N_.mT[s.l]), nullptr, nullptr};
            float* o3[3] = {s.din, nullptr, nullptr};
            S3D_TRY(R.conv(CONV_1x1, O, I, g1, dy3, wT, nullptr, nullptr, o3, 1, false, cs, true));
        }
    for (int n = 0; n < NN; ++n)
        if (!meas) S3D_TRY(launch_add_slice(dXa_n[n], dCAT_n[n], up + hid, 0, dX0[n], Np, up, cs_n[n]));
    if (!meas && R.side && two) S3D_TRY(R.edge(a->chain2, st));   // the scatter reads both nets' point gradients
    // ---- scatter the point gradients onto the planes
    float* dF[2][3] = {};
    for (int n = 0; n < NN; ++n) for (int p = 0; p < 3; ++p) dF[n][p] = ar.alloc<float>(hw[p] * up);
    char* sws = ar.alloc<char>(scatter_ws_bytes(Np, g.h, g.w));
    if (!meas) {
        const float* dx[2] = {dX0[0], two ? dX0[1] : nullptr};
        S3D_TRY(launch_scatter(ps, dF, g.h, g.w, up, NN, dx, sws, st));
    }
    // ---- plane blocks
    float* dfeat[3];
    for (int p = 0; p < 3; ++p) dfeat[p] = ar.alloc<float>(hw[p] * CO);
    if (!meas && R.side && two) S3D_TRY(R.edge(st, a->chain2));   // (the scatter's plane gradients are final)
    for (int n = 0; n < NN; ++n) {
        const AeNet& N_ = a->net[n];
        NetAct& T = A[n];
        const bool second = n == 1 && R.side && !meas;
        hipStream_t cs = second ? a->chain2 : st;                  // this net's chain (see the forward pass)
        float *d_y[3], *d_xs[3], *d_a1[3], *d_x[3];
        for (int p = 0; p < 3; ++p) {
            d_y[p] = ar.alloc<float>(hw[p] * up); d_xs[p] = ar.alloc<float>(hw[p] * 32);
            d_a1[p] = ar.alloc<float>(hw[p] * up); d_x[p] = ar.alloc<float>(hw[p] * 32);
        }
        const float *w_outT[3], *w_scT[3], *w_inT[3];
        float *dw_out[3], *dw_sc[3], *dw_in[3];
        for (int p = 0; p < 3; ++p) {
            w_outT[p] = a->P(N_.out_T[p]); w_scT[p] = a->P(N_.sc_T[p]); w_inT[p] = a->P(N_.in_T[p]);
            dw_out[p] = R.G(N_.f_out_w + size_t(p) * up * up * 25); dw_sc[p] = R.G(N_.f_sc_w + size_t(p) * up * N_.cin);
            dw_in[p] = R.G(N_.f_in_w + size_t(p) * up * N_.cin * 25);
        }
        // bias gradients are column sums nobody inside the pass reads: side stream (the workspace `cws2` belongs to it in this phase)
        hipStream_t sb = R.side ? R.sw : st;
        if (!meas) {
            S3D_TRY(R.edge(cs, sb));
            float *ob[3], *sb2[3];                     // out conv and shortcut share dy: identical bias gradients, one pass, two outputs
            for (int p = 0; p < 3; ++p) { ob[p] = R.G(N_.f_out_b + size_t(p) * up); sb2[p] = R.G(N_.f_sc_b + size_t(p) * up); }
            S3D_TRY(launch_colsum3(dF[n], hw, up, cws2, ob, sb2, sb));
        }
        S3D_TRY(R.conv(CONV_5x5, up, up, g, dF[n], w_outT, nullptr, nullptr, d_y, 3, false, cs, true));
        S3D_TRY(R.wgrad(25, up, up, up, g, dF[n], up, T.y, dw_out, 3, cs, true));
        S3D_TRY(R.conv(CONV_1x1, up, 32, g, dF[n], w_scT, nullptr, nullptr, d_xs, 3, false, cs, true));
        S3D_TRY(R.wgrad(1, 32, N_.cin, up, g, dF[n], 32, T.x, dw_sc, 3, cs, true));
        {   // InstanceNorm(affine) + SiLU backward = GroupNorm backward with one channel per group
            GnActBwd s;
            s.x.C = s.dy.C = s.dx.C = up; s.x.g = s.dy.g = s.dx.g = g;
            for (int p = 0; p < 3; ++p) {
                s.x.p[p] = T.a1[p]; s.dy.p[p] = d_y[p]; s.dx.p[p] = d_a1[p];
                s.gamma[p] = R.F(N_.f_gamma[p]); s.beta[p] = R.F(N_.f_beta[p]); s.dgamma[p] = R.G(N_.f_gamma[p]); s.dbeta[p] = R.G(N_.f_beta[p]);
            }
            s.rowadd = nullptr; s.coladd = nullptr; s.add = nullptr; s.stats.mr = T.mr; s.film = nullptr; s.dfilm = nullptr; s.film_stride = 0;
            s.B = 1; s.ngroups = up;
            s.ws = ar.alloc<float>(gn_bwd_ws_floats(1, up));
            if (!meas) S3D_TRY(launch_gn_act_bwd(s, cs));
        }
        if (!meas) {
            S3D_TRY(R.edge(cs, sb));                    // d_a1 is final
            float* ib[3];
            for (int p = 0; p < 3; ++p) ib[p] = R.G(N_.f_in_b + size_t(p) * up);
            S3D_TRY(launch_colsum3(d_a1, hw, up, cws2, ib, nullptr, sb));
        }
        S3D_TRY(R.wgrad(25, 32, N_.cin, up, g, d_a1, 32, T.x, dw_in, 3, cs, true));
        S3D_TRY(R.conv(CONV_5x5, up, 32, g, d_a1, w_inT, nullptr, d_xs, d_x, 3, false, cs, true));
        if (!meas)
            S3D_TRY(launch_unslice_nhwc3(d_x, dfeat, hw, CO, n == 0 ? 0 : a->geo, N_.cin, cs));
    }
    if (!meas && R.side && two) S3D_TRY(R.edge(a->chain2, st));   // the encoder's backward reads both nets' slices of dfeat
    // ---- encoder
    float* dpre[3];
    for (int p = 0; p < 3; ++p) dpre[p] = ar.alloc<float>(hw[p] * CO);
    float* ews = ar.alloc<float>(std::max(enc_wgrad_ws_floats(a->C, CO), enc_norm_bwd_ws_bytes(CO) / sizeof(float)));
    if (!meas) {
        S3D_TRY(launch_enc_norm(true, pre, feat, enc_mr, dfeat, dpre, g, CO, ews, st));        // (its chunk sums are consumed before the weight gradient reuses ews)
        S3D_TRY(launch_enc_wgrad(a->enc, dpre, a->geo, a->tex, ews, R.G(a->f_enc_w[0]), R.G(a->f_enc_b[0]), two ? R.G(a->f_enc_w[1]) : nullptr,
                                 two ? R.G(a->f_enc_b[1]) : nullptr, st));
        S3D_TRY(R.tail.flush(R.side ? R.sw : st));        // the 16 weight-gradient reductions (they were 16 launches on the stream the iteration waits for)
        S3D_TRY(R.edge(R.sw, st));                        // every gradient of the pass is final in the order of the caller's stream (no-op in line)
    }
    return 0;
}

// The PBR net's iteration (variant 2; AutoEncoderGroupPBR, networks.py:227-333).  A function of its own: variants 0 and 1 keep
// ae_step's launches.  Geometry side: ae_step's, on the caller's stream.  Texture side on chain2: tex_convs.0 (the plane block at
// 3x3), tex_convs.1 (input norm kept, the same norm_p again on the hidden maps, identity shortcut on the NORMALISED input), ONE
// gather, three heads.  The four MLPs advance a layer per launch in the forward pass (four jobs); in the backward pass the three
// heads share chain2: per layer three ReLU backwards, three weight gradients (side stream) and ONE three-job 1x1 dgrad launch.
// The gradient of the gathered feature is ((rgb) + (mr)) + (normal), each term dXa + dCAT[:, :up], in one launch.  norm_p of
// tex_convs.1 receives its hidden-map gradient first (written) and its input-norm gradient second (added), both on chain2.
static int ae_step_pbr(s3d_ae* a, const float* pts, const float* sdf, const float* tex, long long N, const float aabb[6],
                       const s3d_ae_loss_cfg& lc, float* losses, float* pred_out, float* grads, hipStream_t st) {
    AeRun R{a, st, grads};
    Arena& ar = a->arena;
    const bool meas = ar.measuring;
    ar.reset();
    if (!meas && grads && opt_on(OPT_BWD_SIDE)) {
        if (!a->side) {
            int least = 0, greatest = 0;
            (void)hipDeviceGetStreamPriorityRange(&least, &greatest);
            S3D_HIP(hipStreamCreateWithPriority(&a->side, hipStreamNonBlocking, least));
        }
        if (!a->chain2) S3D_HIP(hipStreamCreateWithFlags(&a->chain2, hipStreamNonBlocking));
        R.sw = a->side;
        R.side = true;
    }
    const int up = a->up, hid = a->hid, CO = a->geo + a->tex, S = 9;
    const Geo g = a->enc.g;
    const long long Np = (N + 63) / 64 * 64;
    const bool bwd = grads != nullptr || meas;
    const AePbr& Q = a->pbr;
    hipStream_t c2 = R.side && !meas ? a->chain2 : st;      // the texture side's chain
    hipStream_t sb = R.side ? R.sw : st;                    // bias column sums: nobody inside the pass reads them
    size_t hw[3];
    for (int p = 0; p < 3; ++p) hw[p] = size_t(g.h[p]) * g.w[p];
    auto planes = [&](float* o[3], int C) { for (int p = 0; p < 3; ++p) o[p] = ar.alloc<float>(hw[p] * C); };
    auto conv3 = [&](ConvKind kind, int cin, int cout, float* const in[3], const size_t w[3], size_t fb, float* const res[3], float* const out[3],
                     hipStream_t on) -> int {                 // fb: flat offset of the [3 * cout] bias, size_t(-1) none
        const float *wp[3], *bp[3];
        for (int p = 0; p < 3; ++p) { wp[p] = a->P(w[p]); bp[p] = fb == size_t(-1) ? nullptr : R.F(fb + size_t(p) * cout); }
        return R.conv(kind, cin, cout, g, in, wp, fb == size_t(-1) ? nullptr : bp, res, out, 3, false, on, true);
    };

    // ---- encode
    float *pre[3], *feat[3];
    for (int p = 0; p < 3; ++p) { pre[p] = ar.alloc<float>(hw[p] * CO); feat[p] = ar.alloc<float>(hw[p] * CO); }
    float* enc_mr = ar.alloc<float>(size_t(3) * CO * 2);
    S3D_TRY(ae_encode(R, pre, feat, enc_mr));

    // ---- plane blocks: geo_convs (5x5) and tex_convs.0 (3x3) are the same block
    struct BlockAct { float *x[3], *a1[3], *y[3], *s[3], *f[3], *mr; double* part[3]; } A[2];
    auto block_fwd = [&](int n, hipStream_t cs) -> int {
        const AeNet& N_ = a->net[n];
        BlockAct& T = A[n];
        const ConvKind kind = N_.ks == 3 ? CONV_3x3 : CONV_5x5;
        planes(T.x, 32); planes(T.a1, up); planes(T.y, up); planes(T.s, up); planes(T.f, up);
        for (int p = 0; p < 3; ++p) T.part[p] = ar.alloc<double>(size_t(kInNormChunks) * up * 2);
        T.mr = ar.alloc<float>(size_t(3) * up * 2);
        if (!meas) S3D_TRY(launch_slice_pad_nhwc3(feat, T.x, hw, CO, n == 0 ? 0 : a->geo, N_.cin, cs));
        S3D_TRY(conv3(kind, 32, up, T.x, N_.in_dense, N_.f_in_b, nullptr, T.a1, cs));
        if (!meas) {
            const float *gam[3], *bet[3];
            for (int p = 0; p < 3; ++p) { gam[p] = R.F(N_.f_gamma[p]); bet[p] = R.F(N_.f_beta[p]); }
            S3D_TRY(launch_inorm_silu3(T.a1, T.part, gam, bet, T.y, hw, up, 1e-6f, T.mr, cs));
        }
        S3D_TRY(conv3(CONV_1x1, 32, up, T.x, N_.sc_dense, N_.f_sc_b, nullptr, T.s, cs));
        return conv3(kind, up, up, T.y, N_.out_dense, N_.f_out_b, T.s, T.f, cs);
    };
    if (!meas && R.side) S3D_TRY(R.edge(st, c2));
    S3D_TRY(block_fwd(0, st));
    S3D_TRY(block_fwd(1, c2));
    // tex_convs.1 on f0 = A[1].f
    float *xn[3], *v[3], *a2[3], *y2[3], *f1[3];
    double* part1[3];
    planes(xn, up); planes(v, up); planes(a2, up); planes(y2, up); planes(f1, up);
    for (int p = 0; p < 3; ++p) part1[p] = ar.alloc<double>(size_t(kInNormChunks) * up * 2);
    float* mr_in = ar.alloc<float>(size_t(3) * up * 2);      // {mean, rstd} of f0 (the input norm) and of a2 (the hidden norm)
    float* mr_hid = ar.alloc<float>(size_t(3) * up * 2);
    const float *gam1[3], *bet1[3];
    for (int p = 0; p < 3; ++p) { gam1[p] = R.F(Q.f_gamma[p]); bet1[p] = R.F(Q.f_beta[p]); }
    if (!meas) S3D_TRY(launch_inorm_keep3(A[1].f, part1, gam1, bet1, xn, v, hw, up, 1e-6f, mr_in, c2));
    S3D_TRY(conv3(CONV_3x3, up, up, v, Q.in_dense, Q.f_in_b, nullptr, a2, c2));
    if (!meas) S3D_TRY(launch_inorm_silu3(a2, part1, gam1, bet1, y2, hw, up, 1e-6f, mr_hid, c2));
    S3D_TRY(conv3(CONV_3x3, up, up, y2, Q.out_dense, Q.f_out_b, xn, f1, c2));
    if (!meas && R.side) S3D_TRY(R.edge(c2, st));           // the gather reads both sides' planes
    PointSet ps; ps.pts = pts; ps.N = N; ps.Np = Np;
    for (int k = 0; k < 6; ++k) ps.aabb[k] = aabb[k];

    // ---- points: ONE gather per side, four MLPs (0 geo, 1 rgb, 2 mr, 3 normal)
    constexpr int M = 4;
    const int I[6] = {up, hid, hid, up + hid, hid, hid};
    const size_t* f_mw[M] = {a->net[0].f_mw, Q.head[0].f_mw, Q.head[1].f_mw, Q.head[2].f_mw};
    const size_t* f_mb[M] = {a->net[0].f_mb, Q.head[0].f_mb, Q.head[1].f_mb, Q.head[2].f_mb};
    const size_t* mT[M] = {a->net[0].mT, Q.head[0].mT, Q.head[1].mT, Q.head[2].mT};
    const int nout[M] = {1, Q.head[0].nout, Q.head[1].nout, Q.head[2].nout}, ooff[M] = {0, Q.head[0].ooff, Q.head[1].ooff, Q.head[2].ooff};
    float *X0[2], *Xm[M], *H[M][5], *CAT[M];
    for (int n = 0; n < 2; ++n) X0[n] = ar.alloc<float>(size_t(Np) * up);
    for (int m = 0; m < M; ++m) {
        Xm[m] = X0[m ? 1 : 0];
        for (int l = 0; l < 5; ++l) H[m][l] = ar.alloc<float>(size_t(Np) * hid);
        CAT[m] = ar.alloc<float>(size_t(Np) * (up + hid));
    }
    float* pred = ar.alloc<float>(size_t(Np) * S);
    if (!meas) {
        const float* fp[2][3];
        for (int p = 0; p < 3; ++p) { fp[0][p] = A[0].f[p]; fp[1][p] = f1[p]; }
        S3D_TRY(launch_gather(ps, fp, g.h, g.w, up, 2, X0, st));
    }
    auto lin = [&](int l, float* const in[M], int lo) -> int {
        const float *w[M], *b[M];
        float* out[M];
        for (int m = 0; m < M; ++m) { w[m] = R.F(f_mw[m][l]); b[m] = R.F(f_mb[m][l]); out[m] = H[m][lo]; }
        return R.lin_jobs(I[l], hid, Np, M, in, w, b, out, true, st);
    };
    {
        float *h0[M], *h1[M], *h3[M];
        for (int m = 0; m < M; ++m) { h0[m] = H[m][0]; h1[m] = H[m][1]; h3[m] = H[m][3]; }
        S3D_TRY(lin(0, Xm, 0)); S3D_TRY(lin(1, h0, 1)); S3D_TRY(lin(2, h1, 2));
        if (!meas)
            for (int m = 0; m < M; ++m) {
                S3D_TRY(launch_copy_slice(Xm[m], 1, up, int(Np / 64), 64, CAT[m], up + hid, 0, st));
                S3D_TRY(launch_copy_slice(H[m][2], 1, hid, int(Np / 64), 64, CAT[m], up + hid, up, st));
            }
        S3D_TRY(lin(3, CAT, 3)); S3D_TRY(lin(4, h3, 4));
        if (!meas)
            for (int m = 0; m < M; ++m)                       // pred = sdf | rgb | mr | normal, no sigmoid on the material columns
                S3D_TRY(launch_last_fwd(H[m][4], R.F(f_mw[m][5]), R.F(f_mb[m][5]), hid, nout[m], /*sigm=*/0, pred, S, ooff[m], N, st));
    }
    if (!meas && pred_out) S3D_HIP(hipMemcpyAsync(pred_out, pred, size_t(N) * S * sizeof(float), hipMemcpyDeviceToDevice, st));

    // ---- losses (sdfpbr's three masked means) and d loss / d pred
    float* loss_ws = ar.alloc<float>(512);
    float* loss3 = ar.alloc<float>(8);
    float* dout = bwd ? ar.alloc<float>(size_t(Np) * S) : nullptr;
    if (!meas && sdf) {
        const int gb8[4] = {0, 3, 5, 8};
        S3D_TRY(launch_ae_loss_groups(pred, sdf, tex, N, Np, 8, 3, gb8, /*sigm=*/0, lc.sdf_loss, lc.tex_loss,
                                      lc.sdf_threshold * lc.tex_threshold_ratio, lc.tex_weight, loss_ws, loss3, grads ? dout : nullptr, st));
        if (losses) S3D_HIP(hipMemcpyAsync(losses, loss3, 4 * sizeof(float), hipMemcpyDeviceToDevice, st));
    }
    if (!bwd) return 0;

    // ================================================================= backward
    // ---- MLPs: the geometry net's chain on the caller's stream, the three heads' on chain2
    float* cws2 = ar.alloc<float>(3 * colsum_ws_floats(up));
    float* cws_c[2] = {ar.alloc<float>(colsum_ws_floats(std::max(hid, up))), ar.alloc<float>(colsum_ws_floats(std::max(hid, up)))};
    if (!meas && R.side) S3D_TRY(R.edge(st, c2));
    struct Step { int l; float* act; float* in; int in_stride; float* din; const float* dact; int dstride, coff; };
    Step steps[M][5];
    float *dXa[M], *dCAT[M];
    for (int m = 0; m < M; ++m) {
        hipStream_t cs = m ? c2 : st;
        float* dH = ar.alloc<float>(size_t(Np) * hid);
        dCAT[m] = ar.alloc<float>(size_t(Np) * (up + hid));
        dXa[m] = ar.alloc<float>(size_t(Np) * up);
        float* lws = ar.alloc<float>(last_bwd_ws_floats(hid, nout[m]));
        if (!meas) S3D_TRY(launch_last_bwd(dout, S, ooff[m], R.F(f_mw[m][5]), H[m][4], hid, nout[m], Np, dH, lws, R.G(f_mw[m][5]), R.G(f_mb[m][5]), cs));
        const Step st5[5] = {{4, H[m][4], H[m][3], hid, dH, dH, hid, 0},
                             {3, H[m][3], CAT[m], up + hid, dCAT[m], dH, hid, 0},
                             {2, H[m][2], H[m][1], hid, dH, dCAT[m], up + hid, up},
                             {1, H[m][1], H[m][0], hid, dH, dH, hid, 0},
                             {0, H[m][0], Xm[m], up, dXa[m], dH, hid, 0}};
        for (int k = 0; k < 5; ++k) steps[m][k] = st5[k];
    }
    Geo g1; for (int p = 0; p < 3; ++p) { g1.h[p] = p == 0 ? int(Np / 64) : 0; g1.w[p] = p == 0 ? 64 : 0; }
    for (int k = 0; k < 5; ++k) {
        const int l = steps[0][k].l, Il = I[l];
        float* dP[M];
        for (int m = 0; m < M; ++m) {
            const Step& s = steps[m][k];
            hipStream_t cs = m ? c2 : st;
            dP[m] = ar.alloc<float>(size_t(Np) * hid);
            if (!meas) S3D_TRY(launch_relu_bwd(s.dact, s.dstride, s.coff, s.act, dP[m], Np, hid, cws_c[m ? 1 : 0], R.G(f_mb[m][l]), cs));
            float* dy3[3] = {dP[m], nullptr, nullptr}; float* a3[3] = {s.in, nullptr, nullptr}; float* dw3[3] = {R.G(f_mw[m][l]), nullptr, nullptr};
            S3D_TRY(R.wgrad(1, Il, Il, hid, g1, dy3, s.in_stride, a3, dw3, 1, cs, true));
        }
        {   // geometry net's dgrad, then the heads' as three jobs of one launch
            const float* wT[1] = {a->P(mT[0][l])};
            float* o[1] = {steps[0][k].din};
            S3D_TRY(R.lin_jobs(hid, Il, Np, 1, dP, wT, nullptr, o, false, st));
            const float* wT3[3] = {a->P(mT[1][l]), a->P(mT[2][l]), a->P(mT[3][l])};
            float* o3[3] = {steps[1][k].din, steps[2][k].din, steps[3][k].din};
            S3D_TRY(R.lin_jobs(hid, Il, Np, 3, dP + 1, wT3, nullptr, o3, false, c2));
        }
    }
    float* dX0[2] = {ar.alloc<float>(size_t(Np) * up), ar.alloc<float>(size_t(Np) * up)};
    if (!meas) {
        S3D_TRY(launch_add_slice(dXa[0], dCAT[0], up + hid, 0, dX0[0], Np, up, st));
        S3D_TRY(launch_add_slices3(dXa + 1, dCAT + 1, up + hid, 0, dX0[1], Np, up, c2));
    }
    if (!meas && R.side) S3D_TRY(R.edge(c2, st));            // the scatter reads both sides' point gradients
    // ---- scatter
    float* dF[2][3] = {};
    for (int n = 0; n < 2; ++n) planes(dF[n], up);
    char* sws = ar.alloc<char>(scatter_ws_bytes(Np, g.h, g.w));
    if (!meas) S3D_TRY(launch_scatter(ps, dF, g.h, g.w, up, 2, dX0, sws, st));
    // ---- plane blocks
    float* dfeat[3];
    planes(dfeat, CO);
    if (!meas && R.side) S3D_TRY(R.edge(st, c2));
    auto gn_bwd = [&](float* const x[3], float* const dy[3], float* const dx[3], const size_t fg[3], const size_t fbeta[3], float* mr,
                      hipStream_t cs) -> int {              // InstanceNorm(affine) + SiLU backward; WRITES dgamma / dbeta
        GnActBwd s;
        s.x.C = s.dy.C = s.dx.C = up; s.x.g = s.dy.g = s.dx.g = g;
        for (int p = 0; p < 3; ++p) {
            s.x.p[p] = x[p]; s.dy.p[p] = dy[p]; s.dx.p[p] = dx[p];
            s.gamma[p] = R.F(fg[p]); s.beta[p] = R.F(fbeta[p]); s.dgamma[p] = R.G(fg[p]); s.dbeta[p] = R.G(fbeta[p]);
        }
        s.rowadd = nullptr; s.coladd = nullptr; s.add = nullptr; s.stats.mr = mr; s.film = nullptr; s.dfilm = nullptr; s.film_stride = 0;
        s.B = 1; s.ngroups = up;
        s.ws = ar.alloc<float>(gn_bwd_ws_floats(1, up));
        return meas ? 0 : launch_gn_act_bwd(s, cs);
    };
    auto colsum_side = [&](float* const x[3], size_t fb, size_t fb2, hipStream_t cs) -> int {
        if (meas) return 0;
        S3D_TRY(R.edge(cs, sb));
        float *o[3], *o2[3];
        for (int p = 0; p < 3; ++p) { o[p] = R.G(fb + size_t(p) * up); o2[p] = fb2 == size_t(-1) ? nullptr : R.G(fb2 + size_t(p) * up); }
        return launch_colsum3(x, hw, up, cws2, o, fb2 == size_t(-1) ? nullptr : o2, sb);
    };
    auto dw3 = [&](size_t f, size_t per, float* o[3]) { for (int p = 0; p < 3; ++p) o[p] = R.G(f + size_t(p) * per); };
    // the block of block_fwd: its output gradient dFn -> its slice of dfeat
    auto block_bwd = [&](int n, float* const dFn[3], hipStream_t cs) -> int {
        const AeNet& N_ = a->net[n];
        BlockAct& T = A[n];
        const int taps = N_.ks * N_.ks;
        const ConvKind kind = N_.ks == 3 ? CONV_3x3 : CONV_5x5;
        float *d_y[3], *d_xs[3], *d_a1[3], *d_x[3], *dw_out[3], *dw_sc[3], *dw_in[3];
        planes(d_y, up); planes(d_xs, 32); planes(d_a1, up); planes(d_x, 32);
        dw3(N_.f_out_w, size_t(up) * up * taps, dw_out); dw3(N_.f_sc_w, size_t(up) * N_.cin, dw_sc); dw3(N_.f_in_w, size_t(up) * N_.cin * taps, dw_in);
        S3D_TRY(colsum_side(dFn, N_.f_out_b, N_.f_sc_b, cs));
        S3D_TRY(conv3(kind, up, up, dFn, N_.out_T, size_t(-1), nullptr, d_y, cs));
        S3D_TRY(R.wgrad(taps, up, up, up, g, dFn, up, T.y, dw_out, 3, cs, true));
        S3D_TRY(conv3(CONV_1x1, up, 32, dFn, N_.sc_T, size_t(-1), nullptr, d_xs, cs));
        S3D_TRY(R.wgrad(1, 32, N_.cin, up, g, dFn, 32, T.x, dw_sc, 3, cs, true));
        S3D_TRY(gn_bwd(T.a1, d_y, d_a1, N_.f_gamma, N_.f_beta, T.mr, cs));
        S3D_TRY(colsum_side(d_a1, N_.f_in_b, size_t(-1), cs));
        S3D_TRY(R.wgrad(taps, 32, N_.cin, up, g, d_a1, 32, T.x, dw_in, 3, cs, true));
        S3D_TRY(conv3(kind, up, 32, d_a1, N_.in_T, size_t(-1), d_xs, d_x, cs));
        return meas ? 0 : launch_unslice_nhwc3(d_x, dfeat, hw, CO, n == 0 ? 0 : a->geo, N_.cin, cs);
    };
    S3D_TRY(block_bwd(0, dF[0], st));
    {   // tex_convs.1: dF1 = dF[1]
        float *d_y2[3], *d_a2[3], *d_u[3], *d_f0[3], *dw_out[3], *dw_in[3];
        planes(d_y2, up); planes(d_a2, up); planes(d_u, up); planes(d_f0, up);
        dw3(Q.f_out_w, size_t(up) * up * 9, dw_out); dw3(Q.f_in_w, size_t(up) * up * 9, dw_in);
        void* iws = ar.alloc<char>(in_norm_bwd_ws_bytes(up));
        S3D_TRY(colsum_side(dF[1], Q.f_out_b, size_t(-1), c2));
        S3D_TRY(conv3(CONV_3x3, up, up, dF[1], Q.out_T, size_t(-1), nullptr, d_y2, c2));
        S3D_TRY(R.wgrad(9, up, up, up, g, dF[1], up, y2, dw_out, 3, c2, true));
        S3D_TRY(gn_bwd(a2, d_y2, d_a2, Q.f_gamma, Q.f_beta, mr_hid, c2));          // first use of norm_p: dgamma / dbeta written
        S3D_TRY(colsum_side(d_a2, Q.f_in_b, size_t(-1), c2));
        S3D_TRY(R.wgrad(9, up, up, up, g, d_a2, up, v, dw_in, 3, c2, true));
        S3D_TRY(conv3(CONV_3x3, up, up, d_a2, Q.in_T, size_t(-1), nullptr, d_u, c2));
        if (!meas) {
            float *dg[3], *db[3];
            for (int p = 0; p < 3; ++p) { dg[p] = R.G(Q.f_gamma[p]); db[p] = R.G(Q.f_beta[p]); }
            S3D_TRY(launch_in_norm_bwd3(A[1].f, mr_in, gam1, bet1, dF[1], d_u, d_f0, dg, db, hw, up, iws, c2));   // second use: added
        }
        S3D_TRY(block_bwd(1, d_f0, c2));
    }
    if (!meas && R.side) S3D_TRY(R.edge(c2, st));            // the encoder's backward reads both slices of dfeat
    // ---- encoder
    float* dpre[3];
    planes(dpre, CO);
    float* ews = ar.alloc<float>(std::max(enc_wgrad_ws_floats(a->C, CO), enc_norm_bwd_ws_bytes(CO) / sizeof(float)));
    if (!meas) {
        S3D_TRY(launch_enc_norm(true, pre, feat, enc_mr, dfeat, dpre, g, CO, ews, st));
        S3D_TRY(launch_enc_wgrad(a->enc, dpre, a->geo, a->tex, ews, R.G(a->f_enc_w[0]), R.G(a->f_enc_b[0]), R.G(a->f_enc_w[1]), R.G(a->f_enc_b[1]), st));
        S3D_TRY(R.tail.flush(R.side ? R.sw : st));
        S3D_TRY(R.edge(R.sw, st));
    }
    return 0;
}

static int ae_run(s3d_ae* a, const float* pts, const float* sdf, const float* tex, long long N, const float aabb[6],
                  const s3d_ae_loss_cfg& lc, bool groups, float* losses, float* pred, float* grads, hipStream_t st) {
    if (a->variant == 2) {                                  // the PBR net: its own iteration, always the grouped losses
        a->arena.measuring = true; a->arena.high = 0;
        int rc = ae_step_pbr(a, pts, sdf, tex, N, aabb, lc, losses, pred, grads, st);
        a->arena.measuring = false;
        if (rc) return rc;
        if (a->arena.high > a->arena.buf.cap) {
            S3D_HIP(hipStreamSynchronize(st));
            S3D_TRY(a->arena.buf.reserve(a->arena.high + (a->arena.high >> 3)));
        }
        return ae_step_pbr(a, pts, sdf, tex, N, aabb, lc, losses, pred, grads, st);
    }
    a->arena.measuring = true; a->arena.high = 0;
    int rc = ae_step(a, pts, sdf, tex, N, aabb, lc, groups, losses, pred, grads, st);
    a->arena.measuring = false;
    if (rc) return rc;
    if (a->arena.high > a->arena.buf.cap) {
        S3D_HIP(hipStreamSynchronize(st));
        S3D_TRY(a->arena.buf.reserve(a->arena.high + (a->arena.high >> 3)));
    }
    return ae_step(a, pts, sdf, tex, N, aabb, lc, groups, losses, pred, grads, st);
}

}  // namespace s3d

extern "C" {

int s3d_ae_create(const s3d_decoder_cfg* cfg, s3d_ae** out) { return s3d_ae_create_variant(cfg, 0, out); }
int s3d_ae_create_variant(const s3d_decoder_cfg* cfg, int variant, s3d_ae** out) {
    S3D_CHECK(cfg && out, S3D_ERR_INVALID, "ae_create: null argument");
    S3D_CHECK(variant >= 0 && variant <= 2, S3D_ERR_INVALID, "ae_create: variant %d (0 skip net, 1 geometry only, 2 PBR net)", variant);
    S3D_CHECK(variant != 2 || cfg->tex_channels == 8, S3D_ERR_UNSUPPORTED, "ae: the PBR net has 8 material channels, got tex_channels=%d",
              cfg->tex_channels);
    S3D_CHECK(variant != 2, S3D_ERR_UNSUPPORTED, "ae training: the PBR net (variant 2) is not built by this call; use s3d_ae_create_pbr");
    const bool tex = variant != 1;
    S3D_CHECK(cfg->mlp_hidden_layers == 4, S3D_ERR_UNSUPPORTED, "ae: mlp_hidden_layers=%d (only the default 4 is built)", cfg->mlp_hidden_layers);
    S3D_CHECK(cfg->feat_channel_up % 32 == 0 && cfg->mlp_hidden_channels % 32 == 0 && cfg->feat_channel_up > 0 && cfg->mlp_hidden_channels > 0,
              S3D_ERR_UNSUPPORTED, "ae training: feat_channel_up=%d and mlp_hidden_channels=%d must be multiples of 32",
              cfg->feat_channel_up, cfg->mlp_hidden_channels);
    const int tfc = tex ? cfg->tex_feat_channels : 0;           // (the geometry-only net ignores the tex_* fields)
    S3D_CHECK(cfg->geo_feat_channels >= 1 && (!tex || tfc >= 1) && cfg->geo_feat_channels + tfc <= 12 &&
              cfg->geo_feat_channels % 4 == 0 && tfc % 4 == 0,
              S3D_ERR_UNSUPPORTED, "ae training: feature groups must be multiples of 4 channels, at most 12 together");
    S3D_CHECK(!tex || (cfg->tex_channels >= 1 && cfg->tex_channels <= 8), S3D_ERR_UNSUPPORTED, "ae: tex_channels must be 1..8, got %d",
              cfg->tex_channels);
    std::unique_ptr<s3d_ae> a(new s3d_ae());
    a->cfg = *cfg;
    a->variant = variant; a->nnets = tex ? 2 : 1;
    a->geo = cfg->geo_feat_channels; a->tex = tfc; a->up = cfg->feat_channel_up; a->hid = cfg->mlp_hidden_channels;
    a->TC = tex ? cfg->tex_channels : 0; a->C = 1 + a->TC;
    ae_specs(a.get());
    *out = a.release();
    return 0;
}
int s3d_ae_create_pbr(const s3d_decoder_cfg* cfg, s3d_ae** out) {
    S3D_CHECK(cfg && out, S3D_ERR_INVALID, "ae_create_pbr: null argument");
    S3D_CHECK(cfg->tex_channels == 8, S3D_ERR_UNSUPPORTED, "ae training: the PBR net has 8 material channels, got tex_channels=%d", cfg->tex_channels);
    S3D_CHECK(cfg->mlp_hidden_layers == 4, S3D_ERR_UNSUPPORTED, "ae: mlp_hidden_layers=%d (only the default 4 is built)", cfg->mlp_hidden_layers);
    S3D_CHECK(cfg->feat_channel_up % 32 == 0 && cfg->mlp_hidden_channels % 32 == 0 && cfg->feat_channel_up > 0 && cfg->mlp_hidden_channels > 0,
              S3D_ERR_UNSUPPORTED, "ae training: feat_channel_up=%d and mlp_hidden_channels=%d must be multiples of 32",
              cfg->feat_channel_up, cfg->mlp_hidden_channels);
    S3D_CHECK(cfg->geo_feat_channels >= 1 && cfg->tex_feat_channels >= 1 && cfg->geo_feat_channels + cfg->tex_feat_channels <= 12 &&
              cfg->geo_feat_channels % 4 == 0 && cfg->tex_feat_channels % 4 == 0,
              S3D_ERR_UNSUPPORTED, "ae training: feature groups must be multiples of 4 channels, at most 12 together; got geo=%d tex=%d",
              cfg->geo_feat_channels, cfg->tex_feat_channels);
    std::unique_ptr<s3d_ae> a(new s3d_ae());
    a->cfg = *cfg;
    a->variant = 2; a->nnets = 2;
    a->geo = cfg->geo_feat_channels; a->tex = cfg->tex_feat_channels; a->up = cfg->feat_channel_up; a->hid = cfg->mlp_hidden_channels;
    a->TC = 8; a->C = 9;
    ae_specs(a.get());
    *out = a.release();
    return 0;
}
void s3d_ae_destroy(s3d_ae* a) { delete a; }
int s3d_ae_out_channels(const s3d_ae* a) { return a ? 1 + a->TC : S3D_ERR_INVALID; }
int s3d_ae_num_params(const s3d_ae* a) { return a ? int(a->specs.size()) : S3D_ERR_INVALID; }
int s3d_ae_param_info(const s3d_ae* a, int i, const char** name, int64_t shape[5], int* ndim, int64_t* offset) {
    S3D_CHECK(a && i >= 0 && i < int(a->specs.size()), S3D_ERR_INVALID, "ae param_info: index %d out of range", i);
    if (name) *name = a->specs[i].name.c_str();
    if (ndim) *ndim = int(a->specs[i].shape.size());
    if (shape) for (size_t k = 0; k < a->specs[i].shape.size(); ++k) shape[k] = a->specs[i].shape[k];
    if (offset) *offset = int64_t(a->flat_off[i]);
    return 0;
}
int64_t s3d_ae_param_numel(const s3d_ae* a, int64_t* tex_group_begin) {
    if (!a) return S3D_ERR_INVALID;
    if (tex_group_begin) *tex_group_begin = a->tex_begin;
    return int64_t(a->flat_off.back() + a->specs.back().numel());
}
int s3d_ae_attach(s3d_ae* a, float* params, int64_t numel) {
    S3D_CHECK(a && params, S3D_ERR_INVALID, "ae_attach: null argument");
    S3D_CHECK(numel == s3d_ae_param_numel(a, nullptr), S3D_ERR_INVALID, "ae_attach: %lld floats given, the model has %lld",
              (long long)numel, (long long)s3d_ae_param_numel(a, nullptr));
    a->flat = params;
    return ae_plan(a);
}
int s3d_ae_repack(s3d_ae* a, void* stream) {
    S3D_CHECK(a && a->flat, S3D_ERR_INVALID, "ae_repack: call s3d_ae_attach first");
    return launch_repack_generic(static_cast<const PackDesc*>(a->descs_dev.p), int(a->descs.size()), a->pack_blocks, a->flat,
                                 static_cast<float*>(a->pbuf.p), static_cast<float*>(a->pbuf.p), static_cast<hipStream_t>(stream));
}
int s3d_ae_set_volume(s3d_ae* a, const float* vol, int C, int X2, int Y2, int Z2, void* stream) {
    S3D_CHECK(a && vol, S3D_ERR_INVALID, "ae_set_volume: null argument");
    S3D_CHECK(C == a->C, S3D_ERR_INVALID, "ae_set_volume: %d channels, the encoder takes %d (sdf, then the texture channels)", C, a->C);
    S3D_CHECK(X2 >= 2 && Y2 >= 2 && Z2 >= 2 && X2 % 2 == 0 && Y2 % 2 == 0 && Z2 % 2 == 0, S3D_ERR_INVALID,
              "ae_set_volume: the volume must be twice the feature-map size, got (%d,%d,%d)", X2, Y2, Z2);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const size_t n[3] = {size_t(X2) * Y2 * 4 * C, size_t(X2) * Z2 * 4 * C, size_t(Y2) * Z2 * 4 * C};
    S3D_HIP(hipStreamSynchronize(st));
    S3D_TRY(a->proj.reserve((n[0] + n[1] + n[2]) * sizeof(float)));
    float* P[3] = {static_cast<float*>(a->proj.p), static_cast<float*>(a->proj.p) + n[0], static_cast<float*>(a->proj.p) + n[0] + n[1]};
    S3D_TRY(launch_project(vol, C, X2, Y2, Z2, P, st));
    const int H = X2 / 2, W = Y2 / 2, D = Z2 / 2;
    a->enc.g = Geo::from_hwd(H, W, D);
    for (int p = 0; p < 3; ++p) a->enc.P[p] = P[p];
    a->enc.inv_len[0] = 1.f / D; a->enc.inv_len[1] = 1.f / W; a->enc.inv_len[2] = 1.f / H;
    a->enc.C = C; a->enc.CO = a->geo + a->tex;
    a->has_volume = true;
    return 0;
}
int s3d_ae_encode(s3d_ae* a, float* xy, float* xz, float* yz, void* stream) {
    S3D_CHECK(a && xy && xz && yz, S3D_ERR_INVALID, "ae_encode: null argument");
    S3D_CHECK(a->flat && a->has_volume, S3D_ERR_INVALID, "ae_encode: attach parameters and set the volume first");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const Geo g = a->enc.g; const int CO = a->enc.CO;
    float* out[3] = {xy, xz, yz};
    for (int pass = 0; pass < 2; ++pass) {
        Arena& ar = a->arena;
        ar.measuring = pass == 0;
        if (pass == 0) ar.high = 0;
        else if (ar.high > ar.buf.cap) { S3D_HIP(hipStreamSynchronize(st)); S3D_TRY(ar.buf.reserve(ar.high)); }
        ar.reset();
        float *pre[3], *feat[3];
        for (int p = 0; p < 3; ++p) { pre[p] = ar.alloc<float>(size_t(g.h[p]) * g.w[p] * CO); feat[p] = ar.alloc<float>(size_t(g.h[p]) * g.w[p] * CO); }
        float* mr = ar.alloc<float>(size_t(3) * CO * 2);
        AeRun R{a, st, nullptr};
        S3D_TRY(ae_encode(R, pre, feat, mr));
        if (pass == 1) for (int p = 0; p < 3; ++p) S3D_TRY(launch_nhwc_to_nchw(feat[p], out[p], 1, CO, g.h[p], g.w[p], st));
    }
    a->arena.measuring = false;
    return 0;
}
int s3d_ae_forward(s3d_ae* a, const float* pts, int64_t N, const float aabb[6], float* pred, void* stream) {
    S3D_CHECK(a && pts && aabb && pred && N >= 1, S3D_ERR_INVALID, "ae_forward: bad argument");
    S3D_CHECK(a->flat && a->has_volume, S3D_ERR_INVALID, "ae_forward: attach parameters and set the volume first");
    s3d_ae_loss_cfg lc{};
    return ae_run(a, pts, nullptr, nullptr, N, aabb, lc, false, nullptr, pred, nullptr, static_cast<hipStream_t>(stream));
}
int s3d_ae_loss_grads(s3d_ae* a, const float* pts, const float* sdf, const float* tex, int64_t N, const float aabb[6],
                      const s3d_ae_loss_cfg* cfg, float* losses, float* pred, float* grads, void* stream) {
    S3D_CHECK(a && pts && sdf && (tex || a->TC == 0) && aabb && cfg && losses && grads && N >= 1, S3D_ERR_INVALID, "ae_loss_grads: bad argument");
    S3D_CHECK(a->flat && a->has_volume, S3D_ERR_INVALID, "ae_loss_grads: attach parameters and set the volume first");
    S3D_CHECK(cfg->sdf_loss >= 0 && cfg->sdf_loss <= 1 && cfg->tex_loss >= 0 && cfg->tex_loss <= 2, S3D_ERR_INVALID, "ae_loss_grads: unknown loss type");
    S3D_CHECK(a->variant != 2, S3D_ERR_INVALID, "ae_loss_grads: the PBR net has four losses; call s3d_ae_loss_grads_groups");
    return ae_run(a, pts, sdf, tex, N, aabb, *cfg, false, losses, pred, grads, static_cast<hipStream_t>(stream));
}
int s3d_ae_loss_grads_groups(s3d_ae* a, const float* pts, const float* sdf, const float* tex, int64_t N, const float aabb[6],
                             const s3d_ae_loss_cfg* cfg, float* losses, float* pred, float* grads, void* stream) {
    S3D_CHECK(a && pts && sdf && (tex || a->TC == 0) && aabb && cfg && losses && grads && N >= 1, S3D_ERR_INVALID, "ae_loss_grads_groups: bad argument");
    S3D_CHECK(a->flat && a->has_volume, S3D_ERR_INVALID, "ae_loss_grads_groups: attach parameters and set the volume first");
    S3D_CHECK(cfg->sdf_loss >= 0 && cfg->sdf_loss <= 1 && cfg->tex_loss >= 0 && cfg->tex_loss <= 2, S3D_ERR_INVALID, "ae_loss_grads_groups: unknown loss type");
    return ae_run(a, pts, sdf, tex, N, aabb, *cfg, true, losses, pred, grads, static_cast<hipStream_t>(stream));
}

}  // extern "C"
