"""A float64 torch restatement of the decode of AutoEncoderGroupPBR, of the geometry-only nets and of the skip net with 8
texture channels (src/encoding/networks.py:192-220, 293-316; blocks.py:65-91, 189-256), plane stage and point stage, for the
shapes tests/golden/pbr_decoder.npz does not cover.  test_pbr_host.py pins it to that golden (the reference's own outputs,
including the intermediate texture planes) at relerr < 1e-5, ten times the reference's own fp32-vs-fp64 gap on those inputs
(6.2e-7 and 1.1e-6); that pin is what would catch, say, a residual on f0 instead of the normalised xn in block 1.

Written from the module definitions with per-plane convolutions: the reference's grouped conv on channel-wise composed,
zero-padded planes equals three independent zero-padded convs (SiLU(0) = 0 keeps the padding zero)."""
import numpy as np
import torch
import torch.nn.functional as F

from sin3dm_amd import testing as T

KINDS = ("pbr", "geo", "skip", "skip8")          # skip = the 3-channel net of variant 0 (for the shared geo column)
AABB = (-0.7, -1.0, -0.45, 0.7, 1.0, 0.45)


def shapes_of(kind, up, hid, geo=4, tex=8):
    if kind == "pbr":
        return T.pbr_param_shapes(geo, tex, up, hid, 4, 8)
    if kind == "geo":
        return T.geo_only_param_shapes(geo, up, hid, 4)
    return T.ae_param_shapes(geo, tex, up, hid, 4, 8 if kind == "skip8" else 3)


def weights(kind, up, hid, seed=5, dtype=torch.float64):
    return {k: v.to(dtype) for k, v in T.synthetic_state_dict(shapes_of(kind, up, hid), seed).items()}


def _silu(x):
    return x * torch.sigmoid(x)


def _block(xs, sd, prefix, ks, conv_idx, input_norm):
    """TriplaneGroupResnetBlock on three [1,C,h,w] planes."""
    up = sd[f"{prefix}.out_layers.1.bias"].shape[0] // 3
    outs = []
    for p, (name, x) in enumerate(zip(T.PLANES, xs)):
        gamma, beta = sd[f"{prefix}.norm_{name}.weight"], sd[f"{prefix}.norm_{name}.bias"]
        sl = slice(p * up, (p + 1) * up)
        if input_norm:                                     # input_norm=True comes with input_act=True (tex_convs.1)
            x = F.instance_norm(x, weight=gamma, bias=beta, eps=1e-6)
            h = _silu(x)
        else:
            h = x
        h = F.conv2d(h, sd[f"{prefix}.in_layers.{conv_idx}.weight"][sl], sd[f"{prefix}.in_layers.{conv_idx}.bias"][sl], padding=ks // 2)
        h = _silu(F.instance_norm(h, weight=gamma, bias=beta, eps=1e-6))          # the same norm_p again
        h = F.conv2d(h, sd[f"{prefix}.out_layers.1.weight"][sl], sd[f"{prefix}.out_layers.1.bias"][sl], padding=ks // 2)
        if f"{prefix}.shortcut.weight" in sd:
            h = h + F.conv2d(x, sd[f"{prefix}.shortcut.weight"][sl], sd[f"{prefix}.shortcut.bias"][sl])
        else:
            h = h + x                                      # Identity shortcut on the block's x = the NORMALISED input
        outs.append(h)
    return outs


def plane_stage(kind, sd, fm, geo=4):
    """fm: three [1,C,h,w] float64 planes -> {"geo": [...], "tex0": [...], "tex": [...]} as far as the net has them."""
    out = {"geo": _block([f[:, :geo] for f in fm], sd, "geo_convs", 5, 0, False)}
    if kind == "pbr":
        out["tex0"] = _block([f[:, geo:] for f in fm], sd, "tex_convs.0", 3, 0, False)
        out["tex"] = _block(out["tex0"], sd, "tex_convs.1", 3, 1, True)
    elif kind != "geo":
        out["tex"] = _block([f[:, geo:] for f in fm], sd, "tex_convs", 5, 0, False)
    return out


def _gather(planes, x, padding_mode="border", align_corners=False):
    """sum over the three planes of grid_sample(border, align_corners=False) at coords [[0,1],[0,2],[1,2]]."""
    h = 0
    for fmap, (i, j) in zip(planes, ((0, 1), (0, 2), (1, 2))):
        uv = torch.stack([x[:, j], x[:, i]], dim=-1).view(1, 1, -1, 2)            # grid_sample wants (x = column, y = row)
        h = h + F.grid_sample(fmap, uv, align_corners=align_corners, padding_mode=padding_mode)[0, :, 0, :].t()
    return h


def _mlp(sd, prefix, x):
    h = x
    for i in (0, 2, 4):
        h = torch.relu(F.linear(h, sd[f"{prefix}.first_layers.{i}.weight"], sd[f"{prefix}.first_layers.{i}.bias"]))
    h = torch.cat([x, h], dim=-1)
    for i in (0, 2):
        h = torch.relu(F.linear(h, sd[f"{prefix}.second_layers.{i}.weight"], sd[f"{prefix}.second_layers.{i}.bias"]))
    return F.linear(h, sd[f"{prefix}.second_layers.4.weight"], sd[f"{prefix}.second_layers.4.bias"])


def decode(kind, sd, pts, fm, aabb, feats=None, dtype=torch.float64, **gather):
    """pts [N,3], fm three [1,C,h,w] planes, aabb [6] -> [N, 9 | 1 | 4 | 9] (unclamped), evaluated in `dtype` throughout (sd
    must hold that dtype: weights(.., dtype=)).  gather: padding_mode / align_corners other than the network's, for tests that
    need a wrong sampler."""
    pts = torch.as_tensor(pts, dtype=dtype)
    aabb = torch.as_tensor(aabb, dtype=dtype)
    fm = [torch.as_tensor(f, dtype=dtype) for f in fm]
    feats = feats or plane_stage(kind, sd, fm)
    x = 2 * (pts - aabb[:3]) / (aabb[3:] - aabb[:3]) - 1
    cols = [_mlp(sd, "geo_decoder", _gather(feats["geo"], x, **gather))]
    if kind == "pbr":
        ht = _gather(feats["tex"], x, **gather)
        cols += [_mlp(sd, "rgb_decoder", ht), _mlp(sd, "mr_decoder", ht), _mlp(sd, "normal_decoder", ht)]
    elif kind != "geo":
        cols.append(torch.sigmoid(_mlp(sd, "tex_decoder", _gather(feats["tex"], x, **gather))))
    return torch.cat(cols, dim=1)


def grid_points(aabb, reso):
    """sample_grid_points_aabb (src/encoding/utils3d.py:13-25) in float32, as the reference computes it."""
    aabb = torch.as_tensor(aabb, dtype=torch.float32)
    size = aabb[3:] - aabb[:3]
    res = (reso * size / size.max()).long()
    axes = [torch.linspace(0.5, float(r) - 0.5, int(r)) / r * size[i] + aabb[i] for i, r in enumerate(res)]
    return torch.stack(torch.meshgrid(*axes, indexing="ij"), dim=-1).reshape(-1, 3), tuple(int(r) for r in res)


def synthetic_planes(H, W, D, C=12, seed=40):
    return [0.8 * np.tanh(T.synthetic_noise(s, seed + i)) for i, s in enumerate(((1, C, H, W), (1, C, H, D), (1, C, W, D)))]
