// s3d_aenet.h — the ONE description of the auto-encoder net that the inference handle (s3d_decoder.hip) and the training handle
// (s3d_ae.hip) both read.
//
// Reference: AutoEncoderGroupSkip / AutoEncoderGroupPBR (src/encoding/networks.py:122-220, 227-333), TriplaneGroupResnetBlock /
// DecoderMLPSkipConcat (src/encoding/blocks.py:189-256, 65-91).  The description covers names, shapes, state_dict order and what the
// handles pack: a new head or plane block is one line of aenet_describe for those.  How the blocks RUN is not data: each handle's
// forward (and the training handle's backward) is written for one block per side plus at most one input-norm block behind the
// texture side's, and for at most four heads; the constructors hold the description to that (AeNetDesc::runnable), so a net beyond
// it is refused there and has to be taught to the step functions first.
#pragma once
#include "s3d_params.h"

namespace s3d {

// the six Linear layers of a DecoderMLPSkipConcat with mlp_hidden_layers = 4 (ReLUs sit at the odd indices)
static const char* kMlpLayer[6] = {".first_layers.0", ".first_layers.2", ".first_layers.4", ".second_layers.0", ".second_layers.2", ".second_layers.4"};
// layer l of an MLP takes I[l] and gives O[l] channels (the skip concatenation enters layer 3)
inline void mlp_dims(int up, int hid, int nout, int I[6], int O[6]) {
    for (int l = 0; l < 6; ++l) { I[l] = l == 0 ? up : (l == 3 ? up + hid : hid); O[l] = l == 5 ? nout : hid; }
}

// ------------------------------------------------------------------ the auto-encoder net as data
// a TriplaneGroupResnetBlock: [input norm -> SiLU ->] conv ks x ks -> InstanceNorm(affine) -> SiLU -> conv ks x ks + shortcut
struct AeBlock {
    std::string prefix;       // "geo_convs", "tex_convs", "tex_convs.0", "tex_convs.1"
    int side;                 // 0 geo, 1 tex
    int cin, ks;              // real input channels; kernel size
    int conv_idx;             // the conv is in_layers.<conv_idx>: 1 behind the SiLU of a block that activates its input
    bool shortcut;            // has 1x1 shortcut parameters (else the identity)
    bool input_norm;          // normalises its input with the SAME norm_p it uses on the hidden maps (blocks.py:238-239)
    std::string in_conv() const { return prefix + ".in_layers." + std::to_string(conv_idx); }
};
// a DecoderMLPSkipConcat on a side's gathered features, into output columns [col0, col0 + nout)
struct AeHead { const char* name; int side, nout, col0, sigmoid; };
constexpr int kAeMaxHeads = 4;                            // what the handles' fixed arrays hold (s3d_ae::mlp, DecodeArgs::mlp)
struct AeNetDesc {
    int up = 0, hid = 0, nsides = 2;
    int enc_in[2] = {1, 1};   // input channels of a side's encoder: the sdf | the whole volume (sdf + texture channels)
    std::vector<AeBlock> blocks;          // side by side, in forward order
    std::vector<AeHead> heads;            // side by side, in output-column order
    int out_channels() const { return heads.back().col0 + heads.back().nout; }
    int side_channels(int side) const { for (const auto& b : blocks) if (b.side == side) return b.cin; return 0; }
    // what both handles' step functions are written for: a plain block first on every side, at most one input-norm block, behind the texture side's
    bool runnable() const {
        if (int(heads.size()) > kAeMaxHeads || int(blocks.size()) != nsides + (blocks.back().input_norm ? 1 : 0)) return false;
        for (int k = 0; k < nsides; ++k) if (blocks[k].side != k || blocks[k].input_norm || !blocks[k].shortcut) return false;
        return int(blocks.size()) == nsides || (nsides == 2 && blocks[2].side == 1 && !blocks[2].shortcut);
    }
};
// variant: s3d_decoder_create_variant's numbers — 0 skip net with 1..8 texture channels, 1 geometry only, 2 AutoEncoderGroupPBR
inline AeNetDesc aenet_describe(const s3d_decoder_cfg& c, int variant) {
    AeNetDesc n;
    n.up = c.feat_channel_up; n.hid = c.mlp_hidden_channels; n.nsides = variant == 1 ? 1 : 2;
    n.enc_in[1] = 1 + c.tex_channels;
    n.blocks.push_back({"geo_convs", 0, c.geo_feat_channels, 5, 0, true, false});
    n.heads.push_back({"geo_decoder", 0, 1, 0, 0});
    if (variant == 0) {
        n.blocks.push_back({"tex_convs", 1, c.tex_feat_channels, 5, 0, true, false});
        n.heads.push_back({"tex_decoder", 1, c.tex_channels, 1, 1});
    } else if (variant == 2) {                           // networks.py:246-253, no sigmoid (:311-315)
        n.blocks.push_back({"tex_convs.0", 1, c.tex_feat_channels, 3, 0, true, false});
        n.blocks.push_back({"tex_convs.1", 1, n.up, 3, 1, false, true});
        n.heads.push_back({"rgb_decoder", 1, 3, 1, 0});
        n.heads.push_back({"mr_decoder", 1, 2, 4, 0});
        n.heads.push_back({"normal_decoder", 1, 3, 6, 0});
    }
    return n;
}
// the parameters in state_dict order: per side [its encoder,] its blocks, its heads
inline std::vector<ParamSpec> aenet_params(const AeNetDesc& n, bool with_encoders) {
    std::vector<ParamSpec> s;
    const int64_t up = n.up;
    auto add = [&](const std::string& name, std::vector<int64_t> shape) { s.push_back({name, std::move(shape)}); };
    for (int side = 0; side < n.nsides; ++side) {
        if (with_encoders) {
            const std::string e = side == 0 ? "geo_encoder" : "tex_encoder";
            add(e + ".weight", {n.side_channels(side), n.enc_in[side], 4, 4, 4}); add(e + ".bias", {n.side_channels(side)});
        }
        for (const auto& b : n.blocks) {
            if (b.side != side) continue;
            add(b.in_conv() + ".weight", {3 * up, b.cin, b.ks, b.ks}); add(b.in_conv() + ".bias", {3 * up});
            for (int p = 0; p < 3; ++p) { add(b.prefix + ".norm_" + kPlane[p] + ".weight", {up}); add(b.prefix + ".norm_" + kPlane[p] + ".bias", {up}); }
            add(b.prefix + ".out_layers.1.weight", {3 * up, up, b.ks, b.ks}); add(b.prefix + ".out_layers.1.bias", {3 * up});
            if (b.shortcut) { add(b.prefix + ".shortcut.weight", {3 * up, b.cin, 1, 1}); add(b.prefix + ".shortcut.bias", {3 * up}); }
        }
        for (const auto& h : n.heads) {
            if (h.side != side) continue;
            int I[6], O[6];
            mlp_dims(n.up, n.hid, h.nout, I, O);
            for (int l = 0; l < 6; ++l) { add(std::string(h.name) + kMlpLayer[l] + ".weight", {O[l], I[l]}); add(std::string(h.name) + kMlpLayer[l] + ".bias", {O[l]}); }
        }
    }
    return s;
}

}  // namespace s3d
