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
// Variants (the numbers of s3d_decoder_create_variant): 0 is the net above with 1..8 texture channels (a volume of 1 + tex_channels
// channels; 3 is sdftex, 8 sdfpbr on the skip net), 1 the geometry net alone (use_tex=False: one net, a 1-channel volume, no tex
// group), 2 the PBR net (AutoEncoderGroupPBR, networks.py:227-333; made by s3d_ae_create_pbr, refused by s3d_ae_create_variant):
// two 3x3 texture blocks, the second with an input norm that shares its parameters with the hidden norm, three heads on one gather.
// All three run the ONE iteration ae_step, which reads the net as data: the description of s3d_aenet.h (the one the inference
// handle reads too: blocks, heads, parameter names) and what this handle computes for it — nnets plane blocks (AeNet), tex_convs.1
// when has_tex1 (tex1) and nmlp MLPs (AeMlp: flat and packed offsets, the chain each runs on).  ae_plan looks the parameters up.
#include <memory>

#include "s3d_ae.h"
#include "s3d_aenet.h"
#include "s3d_bwd.h"
#include "s3d_model.h"

namespace s3d {

constexpr size_t kNone = size_t(-1);                         // "no such parameter" where a flat offset is expected

// a plane block of the description: conv ks x ks -> InstanceNorm(affine) -> SiLU -> conv ks x ks + 1x1 shortcut (geo_convs, tex_convs,
// the PBR net's tex_convs.0).  The PBR net's tex_convs.1 is a different kind of block — an input norm, the SAME norm_p again on the
// hidden maps, the identity shortcut on the normalised input — and leaves the sc fields unset
struct AeNet {
    size_t f_in_w, f_in_b, f_out_w, f_out_b, f_sc_w, f_sc_b, f_gamma[3], f_beta[3];   // flat offsets
    size_t in_dense[3], out_dense[3], sc_dense[3], in_T[3], out_T[3], sc_T[3];        // packed offsets
};
// a DecoderMLPSkipConcat (head m of the description, which says whose gather it reads and where its outputs go)
struct AeMlp {
    int chain;                                               // its backward chain: 0 the caller's stream, 1 chain2 (a side's MLPs share
                                                             // that side's chain, in handle order: ae_step adds their point gradients per chain)
    size_t f_mw[6], f_mb[6], mT[5];                          // flat offsets; packed transposes of the five hidden layers
};

}  // namespace s3d

using namespace s3d;

struct s3d_ae {
    s3d_decoder_cfg cfg;
    int variant = 0;                    // s3d_decoder_create_variant's numbers: 0 skip net with texture, 1 geometry only (tex = TC = 0, C = 1, one net), 2 PBR net
    int geo, tex, up, hid, TC, C, nnets = 2;
    AeNetDesc desc;                     // blocks [0, nnets) are net[], block 2 is tex1; head m is mlp[m]
    std::vector<ParamSpec> specs;
    std::vector<size_t> flat_off;
    int64_t tex_begin = 0;
    float* flat = nullptr;
    AeNet net[2];
    bool has_tex1 = false;              // variant 2: tex_convs.1 follows net[1]
    AeNet tex1;
    AeMlp mlp[4];                       // variant 1: geo | 0: geo, tex | 2: geo, rgb, mr, normal
    int nmlp = 0;
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
    hipStream_t chain2 = nullptr;       // the texture side's chain beside the geometry side's (the two only meet at the gather, the scatter and the encoder)
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

static int ae_plan(s3d_ae* a) {
    const int up = a->up, hid = a->hid;
    size_t ps = 0;
    auto palloc = [&](size_t n) { size_t o = (ps + 63) & ~size_t(63); ps = o + n; return o; };
    auto add = [&](int kind, size_t src, size_t dst, long long n, int cout = 0, int ctot = 0, int cin = 0, int taps = 0, int slot = 0) {
        PackDesc d{};
        d.kind = kind; d.cout = cout; d.ctot = ctot; d.cin = cin; d.slot = slot; d.taps = taps; d.src = (long long)src; d.dst = (long long)dst; d.n = n;
        a->descs.push_back(d);
    };
    auto mlp = [&](int m) {
        AeMlp& M = a->mlp[m];
        const AeHead& H = a->desc.heads[m];
        int I[6], O[6];
        mlp_dims(up, hid, H.nout, I, O);
        for (int l = 0; l < 6; ++l) {
            M.f_mw[l] = a->off_of(std::string(H.name) + kMlpLayer[l] + ".weight"); M.f_mb[l] = a->off_of(std::string(H.name) + kMlpLayer[l] + ".bias");
            if (l < 5) { M.mT[l] = palloc(size_t(I[l]) * O[l]); add(PK_TRANS2D, M.f_mw[l], M.mT[l], (long long)I[l] * O[l], O[l], 0, I[l]); }
        }
    };
    // the dense and the transposed image of plane p's [up][cin][T] slice of a conv weight; pad: cin real channels in a 32-channel tensor
    auto conv = [&](size_t w, int p, int cin, int T, bool pad, size_t& dense, size_t& trans) {
        const size_t src = w + size_t(p) * up * cin * T;
        const int ci = pad ? 32 : cin, slot = pad ? 32 : 0;
        const long long n = (long long)(pad ? T : 1) * up * cin;
        dense = palloc(size_t(T) * up * ci); add(pad ? PK_DENSE_PAD : PK_DENSE, src, dense, n, up, cin, cin, T, slot);
        trans = palloc(size_t(T) * ci * up); add(pad ? PK_DENSE_T_PAD : PK_DENSE_T, src, trans, n, up, cin, cin, T, slot);
    };
    a->descs.clear();
    a->encb_off = palloc(a->geo + a->tex);
    a->wp_off = palloc(size_t(3) * (a->geo + a->tex) * 16 * 4 * a->C);
    for (int k = 0; k < a->nnets; ++k) {
        const std::string e = k == 0 ? "geo_encoder" : "tex_encoder";
        a->f_enc_w[k] = a->off_of(e + ".weight"); a->f_enc_b[k] = a->off_of(e + ".bias");
        add(PK_COPY, a->f_enc_b[k], a->encb_off + (k == 0 ? 0 : a->geo), a->desc.side_channels(k));
        for (const AeBlock& B : a->desc.blocks) {
            if (B.side != k) continue;
            const int T = B.ks * B.ks;
            // the first block of its side is net[k] and reads its slice of the encoder's planes: cin real channels in a 32-channel tensor;
            // the one behind it (AeNetDesc::runnable: at most one, the input-norm block) is tex1 and takes the `up` channels before it
            const bool first = &B == &a->desc.blocks[k];
            AeNet& N = first ? a->net[k] : a->tex1;
            auto off = [&](const std::string& n) { return a->off_of(B.prefix + n); };
            N.f_in_w = a->off_of(B.in_conv() + ".weight"); N.f_in_b = a->off_of(B.in_conv() + ".bias");
            N.f_out_w = off(".out_layers.1.weight"); N.f_out_b = off(".out_layers.1.bias");
            if (B.shortcut) { N.f_sc_w = off(".shortcut.weight"); N.f_sc_b = off(".shortcut.bias"); }
            for (int p = 0; p < 3; ++p) {
                N.f_gamma[p] = off(std::string(".norm_") + kPlane[p] + ".weight"); N.f_beta[p] = off(std::string(".norm_") + kPlane[p] + ".bias");
                conv(N.f_in_w, p, B.cin, T, first, N.in_dense[p], N.in_T[p]);
                conv(N.f_out_w, p, up, T, false, N.out_dense[p], N.out_T[p]);
                if (B.shortcut) conv(N.f_sc_w, p, B.cin, 1, true, N.sc_dense[p], N.sc_T[p]);
            }
        }
        for (int m = 0; m < a->nmlp; ++m) if (a->desc.heads[m].side == k) mlp(m);
    }
    a->psize = ps;
    S3D_TRY(a->pbuf.reserve(ps * sizeof(float)));
    S3D_HIP(hipMemset(a->pbuf.p, 0, ps * sizeof(float)));
    S3D_TRY(finalize_pack_plan(a->descs, a->descs_dev, a->pack_blocks));
    return 0;
}

// what a plane block / tex_convs.1 keeps of its forward pass for the backward
struct BlockAct { float *x[3], *a1[3], *y[3], *s[3], *f[3], *mr; double* part[3]; };
struct Tex1Act { float *xn[3], *v[3], *a2[3], *y2[3], *f1[3], *mr_in, *mr_hid; double* part[3]; };   // mr_*: {mean, rstd} of f0 (the input norm) / of a2 (the hidden norm)

// One pass over the net: the streams and their edges, and the pieces of ae_step that work on the three planes of a side.  Every
// piece allocates from the arena in both passes and launches in the run pass only.
struct AeRun {
    s3d_ae* a; hipStream_t st; float* grads;
    hipStream_t sw = nullptr;             // weight gradients; `side` says whether it is a stream of its own (the caller's stream may be the null stream)
    bool side = false;
    size_t ev_next = 0;
    // set by ae_step before the first piece runs
    Geo g{};
    size_t hw[3] = {};
    int up = 0, CO = 0;
    float *feat[3] = {}, *dfeat[3] = {}, *cws2 = nullptr;   // encoder planes and their gradient; workspace of the bias sums (it belongs to their stream)
    BlockAct A[2];
    Tex1Act B;
    DeferredTail tail;

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
    void planes(float* o[3], int C) { for (int p = 0; p < 3; ++p) o[p] = ar().alloc<float>(hw[p] * C); }
    void dw3(size_t f, size_t per, float* o[3]) const { for (int p = 0; p < 3; ++p) o[p] = G(f + size_t(p) * per); }

    // a side's three planes as the three jobs of one launch.  w: packed offsets; fb: flat offset of the [3 * cout] bias, kNone none
    int conv3(ConvKind kind, int cin, int cout, float* const in[3], const size_t w[3], size_t fb, float* const res[3], float* const out[3],
              hipStream_t on) {
        if (meas()) return 0;
        ConvArgs ca; memset(&ca, 0, sizeof ca);
        ca.B = 1; ca.cin = cin; ca.cout = cout; ca.njobs = 3;
        for (int p = 0; p < 3; ++p) {
            ConvJob& J = ca.job[p];
            J.in = in[p]; J.wgt = a->P(w[p]); J.bias = fb == kNone ? nullptr : F(fb + size_t(p) * cout); J.res = res ? res[p] : nullptr; J.out = out[p];
            J.h = g.h[p]; J.w = g.w[p];
        }
        return launch_conv(kind, ca, on);
    }
    // the point list as up to kMaxConvJobs 1x1 jobs of one launch, each h = Np / 64 rows of w = 64 points: every MLP of the net
    // advances a layer per launch in the forward pass, a chain's MLPs take a dgrad per launch in the backward pass
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
    // from: the stream dy was produced on
    int wgrad(int taps, int cin, int cin_store, int cout, const Geo& wg, float* const dy[3], int a_cstride, float* const act[3],
              float* const dW[3], int nplanes, hipStream_t from) {
        WgradArgs w;
        w.dy.C = cout; w.a.C = a_cstride; w.dy.g = w.a.g = wg;
        for (int p = 0; p < 3; ++p) { w.dy.p[p] = p < nplanes ? dy[p] : nullptr; w.a.p[p] = p < nplanes ? act[p] : nullptr; }
        w.B = 1; w.cin = cin; w.cout = cout; w.ctot = cin_store; w.taps = taps; w.cin_store = cin_store; w.nplanes = nplanes;
        w.ksplit = wgrad_ksplit(wg, 1, cin, cout, taps);
        for (int p = 0; p < nplanes; ++p) { w.part[p] = ar().alloc<float>(wgrad_part_floats(w.ksplit, cin, cout, taps)); w.dW[p] = dW[p]; }
        if (meas()) return 0;
        hipStream_t on = side ? sw : from;
        S3D_TRY(edge(from, on));                           // dy and the activation are final in the order of the stream that produced them
        return launch_wgrad(w, on, &tail);                 // (the split-K partials stay in the arena; every reduction of the pass in ONE launch at its end)
    }
    // InstanceNorm(affine) + SiLU backward = GroupNorm backward with one channel per group; WRITES dgamma / dbeta
    int gn_bwd(float* const x[3], float* const dy[3], float* const dx[3], const size_t fg[3], const size_t fbeta[3], float* mr, hipStream_t cs) {
        GnActBwd s;
        s.x.C = s.dy.C = s.dx.C = up; s.x.g = s.dy.g = s.dx.g = g;
        for (int p = 0; p < 3; ++p) {
            s.x.p[p] = x[p]; s.dy.p[p] = dy[p]; s.dx.p[p] = dx[p];
            s.gamma[p] = F(fg[p]); s.beta[p] = F(fbeta[p]); s.dgamma[p] = G(fg[p]); s.dbeta[p] = G(fbeta[p]);
        }
        s.rowadd = nullptr; s.coladd = nullptr; s.add = nullptr; s.stats.mr = mr; s.film = nullptr; s.dfilm = nullptr; s.film_stride = 0;
        s.B = 1; s.ngroups = up;
        s.ws = ar().alloc<float>(gn_bwd_ws_floats(1, up));
        return meas() ? 0 : launch_gn_act_bwd(s, cs);
    }
    // bias gradients are column sums nobody inside the pass reads: side stream.  fb2: a second bias with the same gradient, or kNone
    int colsum_side(float* const x[3], size_t fb, size_t fb2, hipStream_t cs) {
        if (meas()) return 0;
        hipStream_t sb = side ? sw : st;
        S3D_TRY(edge(cs, sb));
        float *o[3], *o2[3];
        dw3(fb, up, o);
        if (fb2 != kNone) dw3(fb2, up, o2);
        return launch_colsum3(x, hw, up, cws2, o, fb2 == kNone ? nullptr : o2, sb);
    }

    // plane block n on chain cs: its slice of the encoder's planes -> A[n].f
    int block_fwd(int n, hipStream_t cs) {
        const AeNet& N_ = a->net[n];
        const AeBlock& D = a->desc.blocks[n];
        BlockAct& T = A[n];
        const ConvKind kind = D.ks == 3 ? CONV_3x3 : CONV_5x5;
        planes(T.x, 32); planes(T.a1, up); planes(T.y, up); planes(T.s, up); planes(T.f, up);
        for (int p = 0; p < 3; ++p) T.part[p] = ar().alloc<double>(size_t(kInNormChunks) * up * 2);
        T.mr = ar().alloc<float>(size_t(3) * up * 2);
        if (!meas()) S3D_TRY(launch_slice_pad_nhwc3(feat, T.x, hw, CO, n == 0 ? 0 : a->geo, D.cin, cs));
        S3D_TRY(conv3(kind, 32, up, T.x, N_.in_dense, N_.f_in_b, nullptr, T.a1, cs));
        if (!meas()) {
            const float *gam[3], *bet[3];
            for (int p = 0; p < 3; ++p) { gam[p] = F(N_.f_gamma[p]); bet[p] = F(N_.f_beta[p]); }
            S3D_TRY(launch_inorm_silu3(T.a1, T.part, gam, bet, T.y, hw, up, 1e-6f, T.mr, cs));
        }
        S3D_TRY(conv3(CONV_1x1, 32, up, T.x, N_.sc_dense, N_.f_sc_b, nullptr, T.s, cs));
        return conv3(kind, up, up, T.y, N_.out_dense, N_.f_out_b, T.s, T.f, cs);
    }
    // its backward: the block's output gradient dFn -> its slice of dfeat
    int block_bwd(int n, float* const dFn[3], hipStream_t cs) {
        const AeNet& N_ = a->net[n];
        const AeBlock& D = a->desc.blocks[n];
        BlockAct& T = A[n];
        const int taps = D.ks * D.ks;
        const ConvKind kind = D.ks == 3 ? CONV_3x3 : CONV_5x5;
        float *d_y[3], *d_xs[3], *d_a1[3], *d_x[3], *dw_out[3], *dw_sc[3], *dw_in[3];
        planes(d_y, up); planes(d_xs, 32); planes(d_a1, up); planes(d_x, 32);
        dw3(N_.f_out_w, size_t(up) * up * taps, dw_out); dw3(N_.f_sc_w, size_t(up) * D.cin, dw_sc); dw3(N_.f_in_w, size_t(up) * D.cin * taps, dw_in);
        S3D_TRY(colsum_side(dFn, N_.f_out_b, N_.f_sc_b, cs));      // out conv and shortcut share dy: identical bias gradients, one pass, two outputs
        S3D_TRY(conv3(kind, up, up, dFn, N_.out_T, kNone, nullptr, d_y, cs));
        S3D_TRY(wgrad(taps, up, up, up, g, dFn, up, T.y, dw_out, 3, cs));
        S3D_TRY(conv3(CONV_1x1, up, 32, dFn, N_.sc_T, kNone, nullptr, d_xs, cs));
        S3D_TRY(wgrad(1, 32, D.cin, up, g, dFn, 32, T.x, dw_sc, 3, cs));
        S3D_TRY(gn_bwd(T.a1, d_y, d_a1, N_.f_gamma, N_.f_beta, T.mr, cs));
        S3D_TRY(colsum_side(d_a1, N_.f_in_b, kNone, cs));
        S3D_TRY(wgrad(taps, 32, D.cin, up, g, d_a1, 32, T.x, dw_in, 3, cs));
        S3D_TRY(conv3(kind, up, 32, d_a1, N_.in_T, kNone, d_xs, d_x, cs));
        return meas() ? 0 : launch_unslice_nhwc3(d_x, dfeat, hw, CO, n == 0 ? 0 : a->geo, D.cin, cs);
    }
    // tex_convs.1 on f0 = A[1].f -> B.f1
    int tex1_fwd(hipStream_t cs) {
        const AeNet& Q = a->tex1;
        planes(B.xn, up); planes(B.v, up); planes(B.a2, up); planes(B.y2, up); planes(B.f1, up);
        for (int p = 0; p < 3; ++p) B.part[p] = ar().alloc<double>(size_t(kInNormChunks) * up * 2);
        B.mr_in = ar().alloc<float>(size_t(3) * up * 2);
        B.mr_hid = ar().alloc<float>(size_t(3) * up * 2);
        const float *gam[3], *bet[3];
        for (int p = 0; p < 3; ++p) { gam[p] = F(Q.f_gamma[p]); bet[p] = F(Q.f_beta[p]); }
        if (!meas()) S3D_TRY(launch_inorm_keep3(A[1].f, B.part, gam, bet, B.xn, B.v, hw, up, 1e-6f, B.mr_in, cs));
        S3D_TRY(conv3(CONV_3x3, up, up, B.v, Q.in_dense, Q.f_in_b, nullptr, B.a2, cs));
        if (!meas()) S3D_TRY(launch_inorm_silu3(B.a2, B.part, gam, bet, B.y2, hw, up, 1e-6f, B.mr_hid, cs));
        return conv3(CONV_3x3, up, up, B.y2, Q.out_dense, Q.f_out_b, B.xn, B.f1, cs);
    }
    // its backward: dF1 -> d_f0.  norm_p receives its hidden-map gradient first (written) and its input-norm gradient second (added)
    int tex1_bwd(float* const dF1[3], float* d_f0[3], hipStream_t cs) {
        const AeNet& Q = a->tex1;
        float *d_y2[3], *d_a2[3], *d_u[3], *dw_out[3], *dw_in[3];
        planes(d_y2, up); planes(d_a2, up); planes(d_u, up); planes(d_f0, up);
        dw3(Q.f_out_w, size_t(up) * up * 9, dw_out); dw3(Q.f_in_w, size_t(up) * up * 9, dw_in);
        void* iws = ar().alloc<char>(in_norm_bwd_ws_bytes(up));
        S3D_TRY(colsum_side(dF1, Q.f_out_b, kNone, cs));
        S3D_TRY(conv3(CONV_3x3, up, up, dF1, Q.out_T, kNone, nullptr, d_y2, cs));
        S3D_TRY(wgrad(9, up, up, up, g, dF1, up, B.y2, dw_out, 3, cs));
        S3D_TRY(gn_bwd(B.a2, d_y2, d_a2, Q.f_gamma, Q.f_beta, B.mr_hid, cs));      // first use of norm_p: dgamma / dbeta written
        S3D_TRY(colsum_side(d_a2, Q.f_in_b, kNone, cs));
        S3D_TRY(wgrad(9, up, up, up, g, d_a2, up, B.v, dw_in, 3, cs));
        S3D_TRY(conv3(CONV_3x3, up, up, d_a2, Q.in_T, kNone, nullptr, d_u, cs));
        if (meas()) return 0;
        const float *gam[3], *bet[3];
        float *dg[3], *db[3];
        for (int p = 0; p < 3; ++p) { gam[p] = F(Q.f_gamma[p]); bet[p] = F(Q.f_beta[p]); dg[p] = G(Q.f_gamma[p]); db[p] = G(Q.f_beta[p]); }
        return launch_in_norm_bwd3(A[1].f, B.mr_in, gam, bet, dF1, d_u, d_f0, dg, db, hw, up, iws, cs);   // second use: added
    }
};

// encode: projections -> pre-activation planes -> InstanceNorm + tanh.  pre/feat: NHWC [hw][CO] per plane
static int ae_encode(AeRun& R, float* pre[3], float* feat[3], float* mr) {
    s3d_ae* a = R.a;
    if (R.meas()) return 0;
    S3D_TRY(launch_enc_pack(R.F(a->f_enc_w[0]), a->nnets == 2 ? R.F(a->f_enc_w[1]) : nullptr, a->geo, a->tex, a->C, static_cast<float*>(a->pbuf.p) + a->wp_off, R.st));
    S3D_TRY(launch_enc_fwd(a->enc, a->P(a->wp_off), a->P(a->encb_off), pre, R.st));
    return launch_enc_norm(false, pre, feat, mr, nullptr, nullptr, a->enc.g, a->enc.CO, nullptr, R.st);
}

// Forward + (when grads != null) backward of one batch of points, for every variant.  pred: [N][1+TC] output.
// Streams (training with the side streams on; in line everything is the caller's stream, with the same bits): the geometry side on
// the caller's stream, the texture side — its plane blocks, its MLPs' backward — on chain2 beside it (the two sides share nothing
// but the encoder's planes, the gather and the scatter), weight and bias gradients on the low-priority side stream.  With one net
// c2 is the caller's stream and every edge to or from it is a no-op.
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
    const int up = a->up, hid = a->hid, CO = a->geo + a->tex, S = 1 + a->TC, NN = a->nnets, M = a->nmlp;
    const bool two = NN == 2;
    const Geo g = a->enc.g;
    const long long Np = (N + 63) / 64 * 64;
    const bool bwd = grads != nullptr || meas;              // the measuring pass sizes the workspace for both
    hipStream_t c2 = R.side && two ? a->chain2 : st;        // the texture side's chain
    hipStream_t chain[2] = {st, c2};
    R.g = g; R.up = up; R.CO = CO;
    for (int p = 0; p < 3; ++p) R.hw[p] = size_t(g.h[p]) * g.w[p];
    int I[6], O[6];
    mlp_dims(up, hid, 0, I, O);                             // (the hidden layers': the last layer has launchers of its own)
    int mb[3] = {0, 0, 0};                                  // chain c's MLPs are [mb[c], mb[c + 1])
    for (int m = 0; m < M; ++m) for (int c = a->mlp[m].chain; c < 2; ++c) ++mb[c + 1];

    // ---- encode
    float *pre[3];
    R.planes(pre, CO); R.planes(R.feat, CO);
    float* enc_mr = ar.alloc<float>(size_t(3) * CO * 2);
    S3D_TRY(ae_encode(R, pre, R.feat, enc_mr));

    // ---- plane blocks
    S3D_TRY(R.edge(st, c2));
    for (int n = 0; n < NN; ++n) S3D_TRY(R.block_fwd(n, chain[n]));
    if (a->has_tex1) S3D_TRY(R.tex1_fwd(c2));
    S3D_TRY(R.edge(c2, st));                                // the gather reads both sides' planes
    // (measured and not kept: the backward scatter's point sort — 21 small dependent launches that depend on the points alone —
    // enqueued here on the second chain's stream, beside the MLPs' forward pass: every one of them waits for a slot behind the
    // 8192-block launches of that pass, the chain arrives late at its backward half, 5.00 -> 5.30 ms/iteration)
    PointSet ps; ps.pts = pts; ps.N = N; ps.Np = Np;
    for (int k = 0; k < 6; ++k) ps.aabb[k] = aabb[k];

    // ---- points: ONE gather per side, then the MLPs a layer per launch
    float *X0[2] = {nullptr, nullptr}, *Xm[4], *H[5][4], *CAT[4];      // H[l][m]: hidden activation l of MLP m
    for (int n = 0; n < NN; ++n) X0[n] = ar.alloc<float>(size_t(Np) * up);
    for (int m = 0; m < M; ++m) {
        Xm[m] = X0[a->desc.heads[m].side];
        for (int l = 0; l < 5; ++l) H[l][m] = ar.alloc<float>(size_t(Np) * hid);
        CAT[m] = ar.alloc<float>(size_t(Np) * (up + hid));
    }
    float* pred = ar.alloc<float>(size_t(Np) * S);
    if (!meas) {
        const float* fp[2][3] = {};
        for (int n = 0; n < NN; ++n) for (int p = 0; p < 3; ++p) fp[n][p] = n == 1 && a->has_tex1 ? R.B.f1[p] : R.A[n].f[p];
        S3D_TRY(launch_gather(ps, fp, g.h, g.w, up, NN, X0, st));
    }
    auto lin = [&](int l, float* const in[]) -> int {
        const float *w[4], *b[4];
        for (int m = 0; m < M; ++m) { w[m] = R.F(a->mlp[m].f_mw[l]); b[m] = R.F(a->mlp[m].f_mb[l]); }
        return R.lin_jobs(I[l], O[l], Np, M, in, w, b, H[l], true, st);
    };
    S3D_TRY(lin(0, Xm)); S3D_TRY(lin(1, H[0])); S3D_TRY(lin(2, H[1]));
    if (!meas)
        for (int m = 0; m < M; ++m) {
            S3D_TRY(launch_copy_slice(Xm[m], 1, up, int(Np / 64), 64, CAT[m], up + hid, 0, st));
            S3D_TRY(launch_copy_slice(H[2][m], 1, hid, int(Np / 64), 64, CAT[m], up + hid, up, st));
        }
    S3D_TRY(lin(3, CAT)); S3D_TRY(lin(4, H[3]));
    if (!meas)
        for (int m = 0; m < M; ++m) {
            const AeMlp& Q = a->mlp[m];
            const AeHead& D = a->desc.heads[m];
            S3D_TRY(launch_last_fwd(H[4][m], R.F(Q.f_mw[5]), R.F(Q.f_mb[5]), hid, D.nout, D.sigmoid, pred, S, D.col0, N, st));
        }
    if (!meas && pred_out) S3D_HIP(hipMemcpyAsync(pred_out, pred, size_t(N) * S * sizeof(float), hipMemcpyDeviceToDevice, st));

    // ---- losses and d loss / d (pre-activation outputs)
    float* loss_ws = ar.alloc<float>(512);
    float* loss3 = ar.alloc<float>(8);
    float* dout = bwd ? ar.alloc<float>(size_t(Np) * S) : nullptr;
    if (!meas && sdf && groups) {
        // eight material channels are three means (rgb | metallic-roughness | normal); any other width is one group, none is sdf.
        // The skip net's texture columns are sigmoid outputs, the PBR net's heads are not
        const int gb8[4] = {0, 3, 5, 8}, gb1[4] = {0, a->TC, 0, 0};
        const int ng = a->TC == 8 ? 3 : (a->TC ? 1 : 0);
        S3D_TRY(launch_ae_loss_groups(pred, sdf, tex, N, Np, a->TC, ng, a->TC == 8 ? gb8 : gb1, /*sigm=*/a->variant != 2, lc.sdf_loss, lc.tex_loss,
                                      lc.sdf_threshold * lc.tex_threshold_ratio, lc.tex_weight, loss_ws, loss3, grads ? dout : nullptr, st));
        if (losses) S3D_HIP(hipMemcpyAsync(losses, loss3, 4 * sizeof(float), hipMemcpyDeviceToDevice, st));
    } else if (!meas && sdf) {
        S3D_TRY(launch_ae_loss(pred, sdf, tex, N, Np, a->TC, lc.sdf_loss, lc.tex_loss, lc.sdf_threshold * lc.tex_threshold_ratio,
                               lc.tex_weight, loss_ws, loss3, grads ? dout : nullptr, st));
        if (losses) S3D_HIP(hipMemcpyAsync(losses, loss3, 2 * sizeof(float), hipMemcpyDeviceToDevice, st));
    }
    if (!bwd) return 0;

    // ================================================================= backward
    // ---- MLPs.  The two sides' backward chains are independent until the scatter: the texture side's runs on a second stream
    // beside the geometry side's — each alternates a bandwidth-bound ReLU backward with an MFMA-bound 1x1 dgrad, so the two chains
    // want different things at most times.  Same kernels on the same operands: same bits.
    R.cws2 = ar.alloc<float>(3 * colsum_ws_floats(up));
    float* cws_c[2] = {ar.alloc<float>(colsum_ws_floats(std::max(hid, up))), ar.alloc<float>(colsum_ws_floats(std::max(hid, up)))};   // per chain
    S3D_TRY(R.edge(st, c2));
    // hidden layers 4..0: dP = dH * relu'(H_l) ; db_l = colsum(dP) ; dW_l = dP^T in_l ; d in_l = dP W_l
    struct Step { int l; float* act; float* in; int in_stride; float* din; const float* dact; int dstride, coff; };
    Step steps[4][5];
    float *dXa[4], *dCAT[4];
    for (int m = 0; m < M; ++m) {
        const AeMlp& Q = a->mlp[m];
        const AeHead& D = a->desc.heads[m];
        float* dH = ar.alloc<float>(size_t(Np) * hid);            // gradient of a hidden activation (reused)
        dCAT[m] = ar.alloc<float>(size_t(Np) * (up + hid));
        dXa[m] = ar.alloc<float>(size_t(Np) * up);
        float* lws = ar.alloc<float>(last_bwd_ws_floats(hid, D.nout));
        if (!meas) S3D_TRY(launch_last_bwd(dout, S, D.col0, R.F(Q.f_mw[5]), H[4][m], hid, D.nout, Np, dH, lws, R.G(Q.f_mw[5]), R.G(Q.f_mb[5]), chain[Q.chain]));
        const Step st5[5] = {{4, H[4][m], H[3][m], hid, dH, dH, hid, 0},
                             {3, H[3][m], CAT[m], up + hid, dCAT[m], dH, hid, 0},
                             {2, H[2][m], H[1][m], hid, dH, dCAT[m], up + hid, up},
                             {1, H[1][m], H[0][m], hid, dH, dH, hid, 0},
                             {0, H[0][m], Xm[m], up, dXa[m], dH, hid, 0}};
        for (int k = 0; k < 5; ++k) steps[m][k] = st5[k];
    }
    // Issued layer by layer for both chains, not chain after chain: the two then advance together however far the host is ahead.
    // Within a layer chain by chain: each MLP's ReLU backward and weight gradient, then the chain's dgrad with its MLPs as jobs.
    Geo g1; for (int p = 0; p < 3; ++p) { g1.h[p] = p == 0 ? int(Np / 64) : 0; g1.w[p] = p == 0 ? 64 : 0; }
    for (int k = 0; k < 5; ++k)
        for (int c = 0; c < NN; ++c) {
            const int l = steps[0][k].l, m0 = mb[c], nj = mb[c + 1] - m0;
            // gradient of the layer's pre-activation: one buffer per layer — the weight gradient that reads it runs on the side
            // stream while this chain has moved on
            float *dP[3], *din[3];
            const float* wT[3];
            for (int j = 0; j < nj; ++j) {
                const AeMlp& Q = a->mlp[m0 + j];
                const Step& s = steps[m0 + j][k];
                dP[j] = ar.alloc<float>(size_t(Np) * hid);
                if (!meas) S3D_TRY(launch_relu_bwd(s.dact, s.dstride, s.coff, s.act, dP[j], Np, O[l], cws_c[c], R.G(Q.f_mb[l]), chain[c]));
                float* dy3[3] = {dP[j], nullptr, nullptr}; float* a3[3] = {s.in, nullptr, nullptr}; float* dw[3] = {R.G(Q.f_mw[l]), nullptr, nullptr};
                S3D_TRY(R.wgrad(1, I[l], I[l], O[l], g1, dy3, s.in_stride, a3, dw, 1, chain[c]));
                wT[j] = a->P(Q.mT[l]); din[j] = s.din;
            }
            S3D_TRY(R.lin_jobs(O[l], I[l], Np, nj, dP, wT, nullptr, din, false, chain[c]));
        }
    // ---- a side's point gradient: dXa + dCAT[:, :up] of its MLP, or of its three heads as ((rgb) + (mr)) + (normal) in one launch
    float* dX0[2] = {nullptr, nullptr};
    for (int c = 0; c < NN; ++c) dX0[c] = ar.alloc<float>(size_t(Np) * up);
    for (int c = 0; c < NN && !meas; ++c) {
        if (mb[c + 1] - mb[c] == 3) S3D_TRY(launch_add_slices3(dXa + mb[c], dCAT + mb[c], up + hid, 0, dX0[c], Np, up, chain[c]));
        else S3D_TRY(launch_add_slice(dXa[mb[c]], dCAT[mb[c]], up + hid, 0, dX0[c], Np, up, chain[c]));
    }
    S3D_TRY(R.edge(c2, st));                                // the scatter reads both sides' point gradients
    // ---- scatter the point gradients onto the planes
    float* dF[2][3] = {};
    for (int n = 0; n < NN; ++n) R.planes(dF[n], up);
    char* sws = ar.alloc<char>(scatter_ws_bytes(Np, g.h, g.w));
    if (!meas) S3D_TRY(launch_scatter(ps, dF, g.h, g.w, up, NN, dX0, sws, st));
    // ---- plane blocks
    R.planes(R.dfeat, CO);
    S3D_TRY(R.edge(st, c2));                                // (the scatter's plane gradients are final)
    S3D_TRY(R.block_bwd(0, dF[0], st));
    if (two) {
        float* d_f0[3];
        if (a->has_tex1) S3D_TRY(R.tex1_bwd(dF[1], d_f0, c2));
        S3D_TRY(R.block_bwd(1, a->has_tex1 ? d_f0 : dF[1], c2));
    }
    S3D_TRY(R.edge(c2, st));                                // the encoder's backward reads both sides' slices of dfeat
    // ---- encoder
    float* dpre[3];
    R.planes(dpre, CO);
    float* ews = ar.alloc<float>(std::max(enc_wgrad_ws_floats(a->C, CO), enc_norm_bwd_ws_bytes(CO) / sizeof(float)));
    if (!meas) {
        S3D_TRY(launch_enc_norm(true, pre, R.feat, enc_mr, R.dfeat, dpre, g, CO, ews, st));    // (its chunk sums are consumed before the weight gradient reuses ews)
        S3D_TRY(launch_enc_wgrad(a->enc, dpre, a->geo, a->tex, ews, R.G(a->f_enc_w[0]), R.G(a->f_enc_b[0]), two ? R.G(a->f_enc_w[1]) : nullptr,
                                 two ? R.G(a->f_enc_b[1]) : nullptr, st));
        S3D_TRY(R.tail.flush(R.side ? R.sw : st));        // the weight-gradient reductions of the pass (they were 16 launches on the stream the iteration waits for)
        S3D_TRY(R.edge(R.sw, st));                        // every gradient of the pass is final in the order of the caller's stream (no-op in line)
    }
    return 0;
}

static int ae_run(s3d_ae* a, const float* pts, const float* sdf, const float* tex, long long N, const float aabb[6],
                  const s3d_ae_loss_cfg& lc, bool groups, float* losses, float* pred, float* grads, hipStream_t st) {
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

// what every constructor refuses; the geometry-only net (variant 1) ignores the tex_* fields
static int ae_check_cfg(const s3d_decoder_cfg* cfg, int variant) {
    const bool tex = variant != 1;
    const int tfc = tex ? cfg->tex_feat_channels : 0;
    S3D_CHECK(variant != 2 || cfg->tex_channels == 8, S3D_ERR_UNSUPPORTED, "ae training: the PBR net has 8 material channels, got tex_channels=%d",
              cfg->tex_channels);
    S3D_CHECK(cfg->mlp_hidden_layers == 4, S3D_ERR_UNSUPPORTED, "ae: mlp_hidden_layers=%d (only the default 4 is built)", cfg->mlp_hidden_layers);
    S3D_CHECK(cfg->feat_channel_up % 32 == 0 && cfg->mlp_hidden_channels % 32 == 0 && cfg->feat_channel_up > 0 && cfg->mlp_hidden_channels > 0,
              S3D_ERR_UNSUPPORTED, "ae training: feat_channel_up=%d and mlp_hidden_channels=%d must be multiples of 32",
              cfg->feat_channel_up, cfg->mlp_hidden_channels);
    S3D_CHECK(cfg->geo_feat_channels >= 1 && (!tex || tfc >= 1) && cfg->geo_feat_channels + tfc <= 12 &&
              cfg->geo_feat_channels % 4 == 0 && tfc % 4 == 0,
              S3D_ERR_UNSUPPORTED, "ae training: feature groups must be multiples of 4 channels, at most 12 together; got geo=%d tex=%d",
              cfg->geo_feat_channels, tfc);
    S3D_CHECK(!tex || (cfg->tex_channels >= 1 && cfg->tex_channels <= 8), S3D_ERR_UNSUPPORTED, "ae: tex_channels must be 1..8, got %d",
              cfg->tex_channels);
    return 0;
}
static int ae_new(const s3d_decoder_cfg* cfg, int variant, s3d_ae** out) {
    const bool tex = variant != 1;
    std::unique_ptr<s3d_ae> a(new s3d_ae());
    a->cfg = *cfg;
    a->variant = variant; a->nnets = tex ? 2 : 1;
    a->geo = cfg->geo_feat_channels; a->tex = tex ? cfg->tex_feat_channels : 0; a->up = cfg->feat_channel_up; a->hid = cfg->mlp_hidden_channels;
    a->TC = tex ? cfg->tex_channels : 0; a->C = 1 + a->TC;
    a->desc = aenet_describe(*cfg, variant);
    S3D_CHECK(a->desc.runnable(), S3D_ERR_UNSUPPORTED, "ae: ae_step is not written for this description of the net (s3d_aenet.h)");
    a->has_tex1 = a->desc.blocks.size() > size_t(a->nnets);
    a->nmlp = int(a->desc.heads.size());
    for (int m = 0; m < a->nmlp; ++m) a->mlp[m].chain = a->desc.heads[m].side;
    a->specs = aenet_params(a->desc, /*with_encoders=*/true);
    a->flat_off.resize(a->specs.size());
    size_t off = 0;
    for (size_t i = 0; i < a->specs.size(); ++i) { a->flat_off[i] = off; off += a->specs[i].numel(); }
    a->tex_begin = int64_t(a->nnets == 2 ? a->off_of("tex_encoder.weight") : off);      // no tex group: it begins where the vector ends
    *out = a.release();
    return 0;
}

}  // namespace s3d

extern "C" {

int s3d_ae_create(const s3d_decoder_cfg* cfg, s3d_ae** out) { return s3d_ae_create_variant(cfg, 0, out); }
int s3d_ae_create_variant(const s3d_decoder_cfg* cfg, int variant, s3d_ae** out) {
    S3D_CHECK(cfg && out, S3D_ERR_INVALID, "ae_create: null argument");
    S3D_CHECK(variant >= 0 && variant <= 2, S3D_ERR_INVALID, "ae_create: variant %d (0 skip net, 1 geometry only, 2 PBR net)", variant);
    S3D_TRY(ae_check_cfg(cfg, variant));
    S3D_CHECK(variant != 2, S3D_ERR_UNSUPPORTED, "ae training: the PBR net (variant 2) is not built by this call; use s3d_ae_create_pbr");
    return ae_new(cfg, variant, out);
}
int s3d_ae_create_pbr(const s3d_decoder_cfg* cfg, s3d_ae** out) {
    S3D_CHECK(cfg && out, S3D_ERR_INVALID, "ae_create_pbr: null argument");
    S3D_TRY(ae_check_cfg(cfg, 2));
    return ae_new(cfg, 2, out);
}
void s3d_ae_destroy(s3d_ae* a) { delete a; }
int s3d_ae_out_channels(const s3d_ae* a) { return a ? 1 + a->TC : S3D_ERR_INVALID; }
int s3d_ae_num_params(const s3d_ae* a) { return a ? int(a->specs.size()) : S3D_ERR_INVALID; }
int s3d_ae_param_info(const s3d_ae* a, int i, const char** name, int64_t shape[5], int* ndim, int64_t* offset) {
    S3D_TRY(registry_param_info(a ? &a->specs : nullptr, "ae ", i, name, shape, ndim));
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
