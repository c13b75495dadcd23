"""Cases, inputs and a float64-capable restatement for the auto-encoder training tier of the PBR network with its material heads
(AutoEncoderGroupPBR with texture, data_type sdfpbr; tests/golden/ae_pbr.npz, written by tests/golden/make_golden_ae_pbr.py from
the reference under autograd).

  pbr         AutoEncoderGroupPBR(4, 8, 64, 256, 4, tex_channels=8)
  pbr.narrow  the same at (4, 8, 32, 64, 4): a compiled decoder form; a width written as a literal shows here
  pbr.offset  case pbr with +3.0 on every element of tex_convs.0.out_layers.1.bias: f0, the input of tex_convs.1's input norm,
              then has a mean far above its spread, which is where the statistics of that norm and its backward lose digits first

Inputs are those of tests/ae_variants_cases.py (feature maps 10 x 14 x 6, volume 20 x 28 x 12, 257 points in +-1.1 x the box, its
batch() recipe with 8 material targets): the smallest shapes at which a tile edge, the border clamp and a partial 64-row tile are
all met.  Weights are sin3dm_amd.testing.synthetic_state_dict(pbr_param_shapes(..., with_encoder=True), 5) and are not stored.

The restatement reuses ae_variants_cases.encode / plane_block / mlp / gather / losses and adds the second 3x3 block and the three
heads; it runs in whatever dtype its inputs have and takes `fault` to inject one deliberate mistake (FAULTS), which
tests/test_ae_pbr_host.py uses to show that the bounds of tests/test_ae_pbr_gpu.py catch each of them."""
from collections import OrderedDict

import ae_variants_cases as V
from ae_variants_cases import AABB, HWD, N_POINTS, PLANES, RATIO, SEED_WEIGHTS, STEPS_HYPER, THR  # noqa: F401  (shared inputs)
from sin3dm_amd import testing as T

CASES = OrderedDict((
    ("pbr", dict(args=(4, 8, 64, 256, 4), offset=0.0)),
    ("pbr.narrow", dict(args=(4, 8, 32, 64, 4), offset=0.0)),
    ("pbr.offset", dict(args=(4, 8, 64, 256, 4), offset=3.0)),
))
TEX_CHANNELS = 8
LOSS_NAMES = ("sdf_loss", "rgb_loss", "mr_loss", "normal_loss")
HEADS = (("rgb_decoder", 3), ("mr_decoder", 2), ("normal_decoder", 3))
FAULTS = ("residual_f0",      # (a) tex_convs.1's residual taken from f0 instead of the normalised xn
          "norm1_out_only",   # (b) the gradients of tex_convs.1.norm_* from the hidden-map use only
          "norm0_on_input",   # (c) the input norm of tex_convs.1 with tex_convs.0's gamma / beta
          "sigmoid",          # (d) a sigmoid on the material columns
          "rgb_point_grad",   # (e) the gathered feature's gradient from the rgb head alone
          "one_mean")         # (f) one l1 mean over the eight material columns

# Bounds per case and quantity.  Rule: the bound of ae_variants_cases.BOUNDS (those of tests/test_hip_ae.py) wherever ten times the
# reference's own float32-versus-float64 gap recorded in the fixture (<case>.gap.<quantity>, in the comment beside each entry)
# stays under it; otherwise ten times that gap, rounded up to two digits.  Written from the fixture's gaps alone.
BOUNDS = {
    "pbr": {
        "encode": 2e-5,          # gap 1.12e-06
        "pred": 2e-5,            # gap 1.04e-06
        "loss": 1e-5,            # gap 6.22e-08
        "grad.norm": 2e-4,       # gap 1.69e-06
        "grad.proj": 5e-4,       # gap 2.09e-06
        "grad.full": 5e-4,       # gap 2.78e-06
        "steps.norm": 5e-3,      # gap 2.34e-04
        "steps.proj": 8.9e-2,    # gap 8.89e-03: ten times it is above the shared 3e-2
    },
    "pbr.narrow": {
        "encode": 2e-5,          # gap 1.12e-06
        "pred": 2e-5,            # gap 1.33e-06
        "loss": 1e-5,            # gap 3.18e-08
        "grad.norm": 2e-4,       # gap 2.12e-06
        "grad.proj": 5e-4,       # gap 1.06e-06
        "grad.full": 5e-4,       # gap 3.97e-06
        "steps.norm": 9.6e-3,    # gap 9.56e-04: ten times it is above the shared 5e-3
        "steps.proj": 9.1e-2,    # gap 9.03e-03: ten times it is above the shared 3e-2
    },
    "pbr.offset": {
        "encode": 2e-5,          # gap 1.12e-06
        "pred": 2e-5,            # gap 1.27e-06
        "loss": 1e-5,            # gap 3.66e-08
        "grad.norm": 2e-4,       # gap 3.29e-06
        "grad.proj": 5e-4,       # gap 1.43e-06
        "grad.full": 5e-4,       # gap 6.30e-06
        "steps.norm": 5e-3,      # gap 2.47e-04
        "steps.proj": 4.2e-2,    # gap 4.14e-03: ten times it is above the shared 3e-2
    },
}
# the losses of the three optimiser steps: |got - want| < STEPS_LOSS * max(1, want), the rule of tests/test_ae_variants_gpu.py
# (largest recorded gap 4.35e-05)
STEPS_LOSS = 5e-4


def shapes(case):
    return T.pbr_param_shapes(*CASES[case]["args"], TEX_CHANNELS, with_encoder=True)


def state_dict(case):
    """the case's weights as float32 torch tensors (synthetic, seed 5; pbr.offset adds its bias offset)"""
    sd = T.synthetic_state_dict(shapes(case), SEED_WEIGHTS)
    if CASES[case]["offset"]:
        sd["tex_convs.0.out_layers.1.bias"] = sd["tex_convs.0.out_layers.1.bias"] + CASES[case]["offset"]
    return sd


def volume(case=None):
    return V.volume("skip8")                                   # 9 channels: sdf and eight materials


def batch(case, seed, n=N_POINTS):
    return V.batch("skip8", seed, n)


# ------------------------------------------------------------------------------------------------ restatement
def tex_block1(sd, f0, fault=None):
    """tex_convs.1 (input_norm, input_act): xn = IN(f0; norm_p); a2 = conv3x3(SiLU(xn)); y2 = SiLU(IN(a2; the SAME norm_p));
    f1 = conv3x3(y2) + xn — the identity shortcut acts on the normalised input"""
    pre = "tex_convs.1"
    up = sd[pre + ".in_layers.1.weight"].shape[0] // 3
    out = []
    for p, (name, x) in enumerate(zip(PLANES, f0)):
        r = slice(p * up, (p + 1) * up)
        g1, b1 = sd[f"{pre}.norm_{name}.weight"], sd[f"{pre}.norm_{name}.bias"]
        gi, bi = g1, b1
        if fault == "norm0_on_input":
            gi, bi = sd[f"tex_convs.0.norm_{name}.weight"], sd[f"tex_convs.0.norm_{name}.bias"]
        elif fault == "norm1_out_only":
            gi, bi = g1.detach(), b1.detach()
        xn = V._inorm(x, gi, bi, eps=1e-6)
        h = V.conv(xn * xn.sigmoid(), sd[pre + ".in_layers.1.weight"][r], sd[pre + ".in_layers.1.bias"][r], 3, fault)
        h = V._inorm(h, g1, b1, eps=1e-6)
        h = V.conv(h * h.sigmoid(), sd[pre + ".out_layers.1.weight"][r], sd[pre + ".out_layers.1.bias"][r], 3, fault)
        out.append(h + (x if fault == "residual_f0" else xn))
    return out


# further faults, which tests/test_ae_variants_f64_host.py holds the bounds of tests/ae_f64_cases.py against: they show at shapes
# and loss modes that the fixture does not have
NEW_FAULTS = ("conv3_short_row",   # the gradients of a 3x3 convolution whose zero padding begins one row early (V.conv)
              "mean_cnt8",         # every group mean divided by rows * 8 (V.losses)
              "normal_point_grad",  # the normal head's gradient never reaches the gathered feature
              "aabb_centred",      # the aabb's centre ignored (V.normalise)
              "band_le")           # the band taken with <= (V.losses)


def decode(sd, pts, fm, aabb, geo_dim=4, fault=None, taps=None):
    """pred = sdf | rgb | mr | normal (no sigmoid); the three heads read ONE gathered feature"""
    import torch
    x = V.normalise(pts, aabb, fault)
    out = [V.mlp(sd, "geo_decoder", V.gather(V.plane_block(sd, "geo_convs", [f[:, :geo_dim] for f in fm]), x), taps)]
    f0 = V.plane_block(sd, "tex_convs.0", [f[:, geo_dim:] for f in fm], ks=3, fault=fault)
    X = V.gather(tex_block1(sd, f0, fault), x)
    for head, _ in HEADS:
        cut = (fault == "rgb_point_grad" and head != "rgb_decoder") or (fault == "normal_point_grad" and head == "normal_decoder")
        out.append(V.mlp(sd, head, X.detach() if cut else X, taps))
    pred = torch.cat(out, dim=1)
    if fault == "sigmoid":
        pred = torch.cat([pred[:, :1], pred[:, 1:].sigmoid()], dim=1)
    return pred


def forward_backward(case, sd, vol, pts, sdf, tex, fault=None, taps=None, aabb=AABB, thr=THR, ratio=RATIO, tex_weight=1.0,
                     sdf_loss="weightedl1", sdf_renorm=False, geo_dim=None):
    """One iteration on a state dict of leaf tensors: (feature maps, pred, losses, {name: gradient of the summed losses}).
    `case` names an entry of CASES, or is such an entry (args)."""
    import torch
    assert fault is None or fault in FAULTS + NEW_FAULTS, fault
    c = CASES[case] if isinstance(case, str) else case
    aabb = torch.tensor(aabb, dtype=vol.dtype)
    with torch.enable_grad():
        p = OrderedDict((k, v.detach().clone().requires_grad_(True)) for k, v in sd.items())
        fm = V.encode(p, vol, "pbr")
        pred = decode(p, pts, fm, aabb, c["args"][0] if geo_dim is None else geo_dim, fault, taps)
        ls = V.losses(pred, sdf, tex, "pbr", thr, ratio, tex_weight, fault if fault in V.LOSS_FAULTS else None, sdf_loss, sdf_renorm)
        grads = torch.autograd.grad(sum(ls.values()), list(p.values()), allow_unused=True)
    named = OrderedDict((k, torch.zeros_like(v) if g is None else g) for (k, v), g in zip(p.items(), grads))
    return [f.detach() for f in fm], pred.detach(), OrderedDict((k, v.detach()) for k, v in ls.items()), named
