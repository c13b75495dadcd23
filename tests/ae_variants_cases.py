"""Cases, inputs and a float64 restatement for the auto-encoder training tier's network variants (tests/golden/ae_variants.npz,
written by tests/golden/make_golden_ae_variants.py from the reference under autograd).

  geo     AutoEncoderGroupSkip(4, 8, 64, 256, 4, use_tex=False)    data_type sdf: 1-channel volume, pred = sdf
  skip8   AutoEncoderGroupSkip(4, 8, 64, 256, 4, tex_channels=8)   data_type sdfpbr on the skip net: 9-channel volume,
                                                                   pred = sdf | sigmoid(8 material channels)

Shared inputs: feature maps H, W, D = 10, 14, 6 (three different sizes, planes smaller than one convolution tile in one
direction), volume 20 x 28 x 12, 257 points (four full 64-row tiles + one) in +-1.1 x the box, so that the border clamp is taken;
sdf samples N(0, 0.04) clipped to +-thr, so that both sides of the texture band |sdf| < 0.999 thr are populated; material
targets uniform in [0, 1].  Weights are sin3dm_amd.testing.synthetic_state_dict(shapes(case), 5) and are not stored.

The restatement is written functionally over a state dict (as oracle/torch_port.py:ae_* is), runs in whatever dtype its inputs
have, and takes `fault` to inject one deliberate mistake, which tests/test_ae_variants_host.py uses to show that the bounds of
tests/test_ae_variants_gpu.py catch it.  The aabb, the texture band, the loss mode and the network's widths are arguments whose
defaults are the fixture's constants; tests/ae_f64_cases.py runs the same functions over its grid of shapes and loss modes."""
from collections import OrderedDict

import numpy as np

from sin3dm_amd import testing as T

PLANES = ("xy", "xz", "yz")
HWD = (10, 14, 6)
N_POINTS = 257
THR = 0.05
RATIO = 0.999
AABB = (-0.7, -1.0, -0.45, 0.7, 1.0, 0.45)
SEED_WEIGHTS, SEED_VOLUME = 5, 1200
STEPS_HYPER = (5e-3, 0.2, 0.1 ** (1 / 10))              # lr, lr_split, ExponentialLR gamma (those of ae_train.npz)

CASES = OrderedDict((
    ("geo", dict(kind="geo", args=(4, 8, 64, 256, 4), tex_channels=0)),
    ("skip8", dict(kind="skip", args=(4, 8, 64, 256, 4), tex_channels=8)),
))
# the bounds of tests/test_hip_ae.py, which tests/test_ae_variants_gpu.py holds every case to
BOUNDS = {"encode": 2e-5, "pred": 2e-5, "loss": 1e-5, "grad.norm": 2e-4, "grad.proj": 5e-4, "grad.full": 5e-4,
          "steps.norm": 5e-3, "steps.proj": 3e-2}


def shapes(case):
    c = CASES[case]
    geo, tex, up, hid, layers = c["args"]
    if c["kind"] == "geo":
        return T.geo_only_param_shapes(geo, up, hid, layers, with_encoder=True)
    return T.ae_param_shapes(geo, tex, up, hid, layers, c["tex_channels"], with_encoder=True)


def volume(case):
    """[1, 1 + tex_channels, 2H, 2W, 2D] float32: a tanh-squashed sdf channel, material channels in [0, 1]"""
    H, W, D = HWD
    C = 1 + CASES[case]["tex_channels"]
    vol = np.tanh(T.synthetic_noise((1, C, 2 * H, 2 * W, 2 * D), SEED_VOLUME))
    vol[:, 1:] = 0.5 * vol[:, 1:] + 0.5
    return np.ascontiguousarray(vol.astype(np.float32))


def batch(case, seed, n=N_POINTS):
    """(pts [n,3], sdf [n,1], tex [n,tex_channels] or None) float32"""
    tc = CASES[case]["tex_channels"]
    rng = np.random.Generator(np.random.PCG64(seed))
    ext = np.asarray(AABB[3:], np.float32)
    pts = rng.uniform(-1.1, 1.1, size=(n, 3)).astype(np.float32) * ext
    sdf = np.clip(rng.normal(0, 0.04, size=(n, 1)), -THR, THR).astype(np.float32)
    tex = rng.uniform(0, 1, size=(n, tc)).astype(np.float32) if tc else None
    return pts, sdf, tex


def loss_names(case):
    return ("sdf_loss",) if CASES[case]["kind"] == "geo" else ("sdf_loss", "rgb_loss", "mr_loss", "normal_loss")


# ------------------------------------------------------------------------------------------------ restatement
def _inorm(x, w=None, b=None, eps=1e-5):
    import torch
    m = x.mean(dim=(2, 3), keepdim=True)
    v = ((x - m) ** 2).mean(dim=(2, 3), keepdim=True)
    y = (x - m) * torch.rsqrt(v + eps)
    return y if w is None else y * w.view(1, -1, 1, 1) + b.view(1, -1, 1, 1)


def encode(sd, vol, kind):
    """Conv3d(k4, s2, p1) of the sdf channel (and of all channels for the texture group), mean over one axis per plane,
    InstanceNorm2d without affine (eps 1e-5), tanh(x / 2)"""
    import torch
    import torch.nn.functional as F
    f = F.conv3d(vol[:, :1], sd["geo_encoder.weight"], sd["geo_encoder.bias"], stride=2, padding=1)
    if kind != "geo":
        f = torch.cat([f, F.conv3d(vol, sd["tex_encoder.weight"], sd["tex_encoder.bias"], stride=2, padding=1)], dim=1)
    return [torch.tanh(0.5 * _inorm(f.mean(dim=d))) for d in (4, 3, 2)]


def conv(x, w, b, ks, fault=None):
    """conv ks x ks, zero padding ks // 2.  fault "conv3_short_row" (3x3 only): the values are right, but the gradients (of the
    input, the weight and the bias) are those of a convolution whose zero padding begins one row early at the lower edge, so that
    the halo row H-1 reads as zero from the output row above it"""
    import torch.nn.functional as F
    y = F.conv2d(x, w, b, padding=ks // 2)
    if fault != "conv3_short_row" or ks != 3 or x.shape[2] < 2:
        return y
    xs = x.clone()
    xs[:, :, -1] = 0
    bad = y.clone()
    bad[:, :, -2] = F.conv2d(xs, w, b, padding=1)[:, :, -2]
    return y.detach() + (bad - bad.detach())


def plane_block(sd, prefix, fm, ks=5, fault=None):
    """per plane: conv ks x ks -> InstanceNorm(affine, eps 1e-6) -> SiLU -> conv ks x ks, plus a 1x1 shortcut of the input"""
    import torch.nn.functional as F
    up = sd[prefix + ".in_layers.0.weight"].shape[0] // 3
    out = []
    for p, (name, x) in enumerate(zip(PLANES, fm)):
        r = slice(p * up, (p + 1) * up)
        h = conv(x, sd[prefix + ".in_layers.0.weight"][r], sd[prefix + ".in_layers.0.bias"][r], ks, fault)
        h = _inorm(h, sd[f"{prefix}.norm_{name}.weight"], sd[f"{prefix}.norm_{name}.bias"], eps=1e-6)
        h = conv(h * h.sigmoid(), sd[prefix + ".out_layers.1.weight"][r], sd[prefix + ".out_layers.1.bias"][r], ks, fault)
        out.append(h + F.conv2d(x, sd[prefix + ".shortcut.weight"][r], sd[prefix + ".shortcut.bias"][r]))
    return out


def mlp(sd, prefix, x, taps=None):
    """three ReLU layers, concat with the input, two ReLU layers, one linear output layer; taps receives the pre-activations"""
    import torch
    import torch.nn.functional as F

    def relu(z):
        if taps is not None:
            taps.append(z)
        return F.relu(z)
    h = x
    for i in (0, 2, 4):
        h = relu(F.linear(h, sd[f"{prefix}.first_layers.{i}.weight"], sd[f"{prefix}.first_layers.{i}.bias"]))
    h = torch.cat([x, h], dim=-1)
    for i in (0, 2):
        h = relu(F.linear(h, sd[f"{prefix}.second_layers.{i}.weight"], sd[f"{prefix}.second_layers.{i}.bias"]))
    return F.linear(h, sd[f"{prefix}.second_layers.4.weight"], sd[f"{prefix}.second_layers.4.bias"])


def gather(planes, x):
    """sum over the three planes of the bilinear, border-clamped sample (pixel centres at half-integers) at (x,y), (x,z), (y,z)"""
    import torch.nn.functional as F
    tot = 0
    for plane, (u, v) in zip(planes, ((0, 1), (0, 2), (1, 2))):
        grid = x[:, [v, u]].view(1, 1, -1, 2)                 # grid_sample wants (column, row)
        tot = tot + F.grid_sample(plane, grid, align_corners=False, padding_mode="border")[0, :, 0, :].t()
    return tot


def normalise(pts, aabb, fault=None):
    """aabb -> [-1, 1] per axis.  fault "aabb_centred": the box's extent about the origin, its centre ignored"""
    if fault == "aabb_centred":
        return 2 * pts / (aabb[3:] - aabb[:3])
    return 2 * (pts - aabb[:3]) / (aabb[3:] - aabb[:3]) - 1


def decode(sd, pts, fm, aabb, kind, geo_dim=4, taps=None, fault=None):
    """fault "chain2_drop": the texture head's gradient never reaches its gathered feature (tex_convs and tex_encoder then get
    no gradient)"""
    import torch
    x = normalise(pts, aabb, fault)
    out = mlp(sd, "geo_decoder", gather(plane_block(sd, "geo_convs", [f[:, :geo_dim] for f in fm]), x), taps)
    if kind == "geo":
        return out
    X = gather(plane_block(sd, "tex_convs", [f[:, geo_dim:] for f in fm]), x)
    tex = mlp(sd, "tex_decoder", X.detach() if fault == "chain2_drop" else X, taps)
    return torch.cat([out, tex.sigmoid()], dim=1)


GROUPS = (("rgb_loss", slice(0, 3)), ("mr_loss", slice(3, 5)), ("normal_loss", slice(5, 8)))
LOSS_FAULTS = ("one_mean", "mean_cnt8", "band_le")


def losses(pred, sdf, tex, kind, thr=THR, ratio=RATIO, tex_weight=1.0, fault=None, sdf_loss="weightedl1", sdf_renorm=False):
    """sdf loss l1 | weightedl1 over all rows; over the rows with |sdf| < float32(band), band = thr * ratio (1.0 * ratio with
    sdf_renorm, where the samples are already divided by thr) and the test made on the float32 sdf samples: for 8 material
    channels three l1 means (columns 0-2, 3-4, 5-7), for any other width one l1 mean (tex_loss); each times tex_weight.
    faults: "one_mean"  ONE mean over the eight columns, reported under rgb_loss (it scales the groups' gradients 3/8 : 2/8 : 3/8
    instead of 1/3 : 1/2 : 1/3); "mean_cnt8"  every group's sum divided by rows * 8 instead of rows * its own columns;
    "band_le"  the band taken with <=."""
    import torch
    ps = pred[:, :1]
    if sdf_loss == "l1":
        out = OrderedDict(sdf_loss=(ps - sdf).abs().mean())
    else:
        assert sdf_loss == "weightedl1", sdf_loss
        w = 1 + 0.5 * torch.sign(sdf) * torch.sign(sdf - ps)
        out = OrderedDict(sdf_loss=((ps - sdf).abs() * w).mean())
    if kind == "geo":
        return out
    band = (1.0 if sdf_renorm else thr) * ratio
    a = sdf[:, 0].float().abs()
    mask = a <= band if fault == "band_le" else a < band
    d = (pred[:, 1:] - tex)[mask].abs()
    if d.shape[1] != 8:
        assert fault in (None, "band_le"), fault
        out["tex_loss"] = d.mean() * tex_weight
        return out
    if fault == "one_mean":
        out["rgb_loss"] = d.mean() * tex_weight
        out["mr_loss"] = out["normal_loss"] = d.sum() * 0
        return out
    assert fault is None or fault in LOSS_FAULTS, fault
    for name, cols in GROUPS:
        out[name] = (d[:, cols].sum() / (d.shape[0] * 8) if fault == "mean_cnt8" else d[:, cols].mean()) * tex_weight
    return out


def forward_backward(case, sd, vol, pts, sdf, tex, fault=None, taps=None, aabb=AABB, thr=THR, ratio=RATIO, tex_weight=1.0,
                     sdf_loss="weightedl1", sdf_renorm=False, geo_dim=None):
    """One iteration on a state dict of leaf tensors: (feature maps, pred, losses, {name: gradient of the summed losses}).
    `case` names an entry of CASES, or is such an entry (kind and args)."""
    import torch
    c = CASES[case] if isinstance(case, str) else case
    kind = c["kind"]
    aabb = torch.tensor(aabb, dtype=vol.dtype)
    with torch.enable_grad():
        p = OrderedDict((k, v.detach().clone().requires_grad_(True)) for k, v in sd.items())
        fm = encode(p, vol, kind)
        pred = decode(p, pts, fm, aabb, kind, c["args"][0] if geo_dim is None else geo_dim, taps,
                      fault if fault in ("aabb_centred", "chain2_drop") else None)
        ls = losses(pred, sdf, tex, kind, thr, ratio, tex_weight, fault if fault in LOSS_FAULTS else None, sdf_loss, sdf_renorm)
        grads = torch.autograd.grad(sum(ls.values()), list(p.values()), allow_unused=True)
    named = OrderedDict((k, torch.zeros_like(v) if g is None else g) for (k, v), g in zip(p.items(), grads))
    return [f.detach() for f in fm], pred.detach(), OrderedDict((k, v.detach()) for k, v in ls.items()), named
