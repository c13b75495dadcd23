"""PyTorch-CPU functional port of the Sin3DM denoising step.  TEST / BASELINE INFRASTRUCTURE ONLY.

A second CPU restatement next to oracle/sin3dm_oracle.c: it runs the reference's algorithm through the very
ATen/oneDNN CPU ops the reference itself dispatches to (F.conv2d, F.group_norm, F.avg_pool2d,
F.interpolate), assembled functionally from a plain state_dict.  bench.py times it as the `cpu_baseline`
("port": the reference cannot travel to the GPU box) because it is the fastest honest CPU path we have —
4-5x faster than the plain-C oracle.  Pinned against the golden vectors in tests/test_oracle_golden.py.
Nothing under sin3dm_amd/ imports this file.
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

PLANES = ("xy", "xz", "yz")


def timestep_embedding(t, dim, dtype=torch.float32):
    """src/diffusion/nn.py:103-121; dtype: the reference's float32, or the parameters' dtype for a float64 evaluation."""
    half = dim // 2
    freqs = torch.exp(-math.log(10000) * torch.arange(half, dtype=dtype, device=t.device) / half)
    args = t[:, None].to(dtype) * freqs[None]
    emb = torch.cat([torch.cos(args), torch.sin(args)], dim=-1)
    if dim % 2:
        emb = torch.cat([emb, torch.zeros_like(emb[:, :1])], dim=-1)
    return emb


def silu(x):
    return x * torch.sigmoid(x)


def tconv(sd, prefix, fm, pad, rollout):
    """TriplaneConv.forward, src/diffusion/unet_triplane.py:31-60"""
    xy, xz, yz = fm
    if rollout:
        xy_in = torch.cat([xy, yz.mean(-1, keepdim=True).transpose(-1, -2).expand_as(xy),
                           xz.mean(-1, keepdim=True).expand_as(xy)], 1)
        xz_in = torch.cat([xz, xy.mean(-1, keepdim=True).expand_as(xz), yz.mean(-2, keepdim=True).expand_as(xz)], 1)
        yz_in = torch.cat([yz, xy.mean(-2, keepdim=True).transpose(-1, -2).expand_as(yz),
                           xz.mean(-2, keepdim=True).expand_as(yz)], 1)
        fm = (xy_in, xz_in, yz_in)
    return tuple(F.conv2d(x, sd[f"{prefix}.conv_{p}.weight"], sd[f"{prefix}.conv_{p}.bias"], padding=pad)
                 for p, x in zip(PLANES, fm))


def tnorm(sd, prefix, fm):
    """TriplaneNorm = GroupNorm32(32, C) per plane, src/diffusion/unet_triplane.py:63-84"""
    return tuple(F.group_norm(x, 32, sd[f"{prefix}.norm_{p}.weight"], sd[f"{prefix}.norm_{p}.bias"], 1e-5)
                 for p, x in zip(PLANES, fm))


def resblock(sd, prefix, fm, emb, ssn, rollout):
    """TriplaneResBlock._forward, src/diffusion/unet_triplane.py:269-311"""
    h = tconv(sd, prefix + ".in_layers.2", tuple(silu(x) for x in tnorm(sd, prefix + ".in_layers.0", fm)), 1, rollout)
    e = F.linear(silu(emb), sd[prefix + ".emb_layers.1.weight"], sd[prefix + ".emb_layers.1.bias"])[..., None, None]
    if ssn:
        scale, shift = torch.chunk(e, 2, dim=1)
        h = tuple(x * (1 + scale) + shift for x in tnorm(sd, prefix + ".out_layers.0", h))
    else:
        h = tnorm(sd, prefix + ".out_layers.0", tuple(x + e for x in h))
    h = tconv(sd, prefix + ".out_layers.2", tuple(silu(x) for x in h), 1, rollout)
    skip = tconv(sd, prefix + ".skip_connection", fm, 0, False) if prefix + ".skip_connection.conv_xy.weight" in sd else fm
    return tuple(a + b for a, b in zip(h, skip))


def unet_forward(sd, x, t, H, W, D, model_channels, channel_mult=(1, 2), use_scale_shift_norm=True, rollout=True):
    """TriplaneUNetModelSmall.forward, src/diffusion/unet_triplane.py:465-510.  Follows the dtype of the parameters (the
    timestep embedding included): float64 parameters and inputs give a float64 evaluation."""
    emb = timestep_embedding(t, model_channels, sd["time_embed.0.weight"].dtype)
    emb = F.linear(silu(F.linear(emb, sd["time_embed.0.weight"], sd["time_embed.0.bias"])),
                   sd["time_embed.2.weight"], sd["time_embed.2.bias"])
    fm = (x[..., :H, :W], x[..., :H, W:], x[..., H:, :W].transpose(-1, -2))
    h = tconv(sd, "in_conv.0", fm, 0, False)
    hs = []
    for level in range(len(channel_mult)):
        if level:
            h = tuple(F.avg_pool2d(a, 2, 2) for a in h)
        h = resblock(sd, f"input_blocks.{level}.{0 if level == 0 else 1}", h, emb, use_scale_shift_norm, rollout)
        hs.append(h)
    for oi in range(len(channel_mult)):
        level = len(channel_mult) - 1 - oi
        if oi == 0:
            h = hs.pop()
        else:
            sk = hs.pop()
            h = tuple(a if a.shape[2:] == s.shape[2:] else F.interpolate(a, size=s.shape[2:], mode="bilinear", align_corners=False)
                      for a, s in zip(h, sk))
            h = tuple(torch.cat([a, s], 1) for a, s in zip(h, sk))
        h = resblock(sd, f"output_blocks.{oi}.0", h, emb, use_scale_shift_norm, rollout)
        if level > 0:
            h = tuple(F.interpolate(a, scale_factor=2, mode="bilinear", align_corners=False) for a in h)
    xy, xz, yz = tconv(sd, "out.2", tuple(silu(a) for a in tnorm(sd, "out.0", h)), 0, False)
    out = x.new_zeros(x.shape[0], xy.shape[1], H + D, W + D)
    out[..., :H, :W], out[..., :H, W:], out[..., H:, :W] = xy, xz, yz.transpose(-1, -2)
    return out


def p_sample_update(model_out, x, eps, tab, t):
    """p_mean_variance (START_X, FIXED_LARGE, clip) + p_sample, src/diffusion/gaussian_diffusion.py:233-327, 396-440.
    tab: the float64 [8,T] table of oracle.schedule_tables()."""
    x0 = model_out.clamp(-1, 1)
    mean = float(tab[6][t]) * x0 + float(tab[7][t]) * x
    var = tab[5][1] if t == 0 else tab[0][t]
    return mean + (0.0 if t == 0 else 1.0) * math.exp(0.5 * math.log(var)) * eps, x0


# ---------------------------------------------------------------------------------------------- training tier
def q_sample(x0, noise, sqrt_ac, sqrt_1mac, t):
    """src/diffusion/gaussian_diffusion.py:189-207; sqrt_ac / sqrt_1mac: float64 numpy tables, t: int64 [B].  The
    coefficients are rounded to x0's dtype (the reference's float32; float64 keeps the tables as they are)."""
    a = torch.from_numpy(sqrt_ac).to(x0.device)[t].to(x0.dtype)[:, None, None, None]
    b = torch.from_numpy(sqrt_1mac).to(x0.device)[t].to(x0.dtype)[:, None, None, None]
    return a * x0 + b * noise


def training_losses(sd, x0, t, noise, tabs, H, W, D, predict_xstart=True, weights=None, **unet_kw):
    """training_losses with MSE (gaussian_diffusion.py:771-856): per-plane mean-squared errors summed; the target is x0
    (ModelMeanType.START_X) or, with predict_xstart=False, the noise (EPSILON, :829-835).
    sd tensors may require grad; returns {"mse_xy","mse_xz","mse_yz","loss"} each [B], and x_t.  Everything runs in the dtype of
    x0 (float64 x0, noise and parameters: a float64 evaluation, x_t formed in float64 from the float64 tables).
    weights [B] (TrainLoop.forward_backward, train_util.py:205-236): terms also holds "objective" = (loss * weights).mean(),
    the scalar the training loop differentiates."""
    x_t = q_sample(x0, noise, tabs["sqrt_alphas_cumprod"], tabs["sqrt_one_minus_alphas_cumprod"], t)
    out = unet_forward(sd, x_t, t.to(x0.dtype), H, W, D, **unet_kw)
    terms = {}
    for name, tgt, o in zip(PLANES, _decompose(x0 if predict_xstart else noise, H, W, D), _decompose(out, H, W, D)):
        terms["mse_" + name] = ((tgt - o) ** 2).flatten(1).mean(1)
    terms["loss"] = terms["mse_xy"] + terms["mse_xz"] + terms["mse_yz"]
    if weights is not None:
        terms["objective"] = (terms["loss"] * weights.to(x0.dtype)).mean()
    return terms, x_t


def _decompose(c, H, W, D):
    return c[..., :H, :W], c[..., :H, W:], c[..., H:, :W].transpose(-1, -2)


def adamw_ema_step(params, grads, m, v, ema, step, lr, wd, ema_rate, b1=0.9, b2=0.999, eps=1e-8):
    """One torch.optim.AdamW step (decoupled decay, bias-corrected) followed by update_ema (src/diffusion/nn.py:55-65),
    in place on lists of tensors; `step` counts from 1."""
    c1, c2 = 1 - b1 ** step, 1 - b2 ** step
    for p, g, mi, vi, e in zip(params, grads, m, v, ema if ema else [None] * len(params)):
        p.mul_(1 - lr * wd)
        mi.mul_(b1).add_(g, alpha=1 - b1)
        vi.mul_(b2).addcmul_(g, g, value=1 - b2)
        denom = (vi.sqrt() / math.sqrt(c2)).add_(eps)
        p.addcdiv_(mi, denom, value=-lr / c1)
        if e is not None:
            e.mul_(ema_rate).add_(p, alpha=1 - ema_rate)


# ---------------------------------------------------------------------------------------------- auto-encoder tier
def _inorm(x, w=None, b=None, eps=1e-5):
    return F.instance_norm(x, weight=w, bias=b, eps=eps)


def ae_encode(sd, vol, geo_dim=4):
    """AutoEncoderGroupSkip.encode, src/encoding/networks.py:164-180: Conv3d(k4,s2,p1) -> axis means -> InstanceNorm2d
    -> tanh(0.5 x).  vol: [1, 1+tex_channels, 2H, 2W, 2D]."""
    geo = F.conv3d(vol[:, :1], sd["geo_encoder.weight"], sd["geo_encoder.bias"], stride=2, padding=1)
    tex = F.conv3d(vol, sd["tex_encoder.weight"], sd["tex_encoder.bias"], stride=2, padding=1)
    f = torch.cat([geo, tex], dim=1)
    return [(_inorm(f.mean(dim=d)) * 0.5).tanh() for d in (4, 3, 2)]


def ae_plane_block(sd, prefix, fm):
    """TriplaneGroupResnetBlock(ks=5, input_norm=False, input_act=False), src/encoding/blocks.py:189-256: the grouped
    conv is three independent per-plane convs (rows p*up:(p+1)*up of the weight)."""
    out = []
    up = sd[prefix + ".in_layers.0.weight"].shape[0] // 3
    for p, (name, x) in enumerate(zip(PLANES, fm)):
        rows = slice(p * up, (p + 1) * up)
        h = F.conv2d(x, sd[prefix + ".in_layers.0.weight"][rows], sd[prefix + ".in_layers.0.bias"][rows], padding=2)
        h = _inorm(h, sd[f"{prefix}.norm_{name}.weight"], sd[f"{prefix}.norm_{name}.bias"], eps=1e-6)
        h = F.conv2d(silu(h), sd[prefix + ".out_layers.1.weight"][rows], sd[prefix + ".out_layers.1.bias"][rows], padding=2)
        out.append(h + F.conv2d(x, sd[prefix + ".shortcut.weight"][rows], sd[prefix + ".shortcut.bias"][rows]))
    return out


def _mlp(sd, prefix, x, n_hidden_layers=4, taps=None):
    """DecoderMLPSkipConcat, src/encoding/blocks.py:65-91.  taps: a list that receives every hidden pre-activation."""
    n = n_hidden_layers // 2

    def relu(z):
        if taps is not None:
            taps.append(z)
        return F.relu(z)
    h = x
    for i in range(n + 1):
        h = relu(F.linear(h, sd[f"{prefix}.first_layers.{2 * i}.weight"], sd[f"{prefix}.first_layers.{2 * i}.bias"]))
    h = torch.cat([x, h], dim=-1)
    for i in range(n):
        h = relu(F.linear(h, sd[f"{prefix}.second_layers.{2 * i}.weight"], sd[f"{prefix}.second_layers.{2 * i}.bias"]))
    return F.linear(h, sd[f"{prefix}.second_layers.{2 * n}.weight"], sd[f"{prefix}.second_layers.{2 * n}.bias"])


def ae_decode(sd, pts, fm, aabb, geo_dim=4, taps=None):
    """AutoEncoderGroupSkip.decode, src/encoding/networks.py:192-220.  taps: as in _mlp, for both MLPs ([N, hidden] each)."""
    x = 2 * (pts - aabb[:3]) / (aabb[3:] - aabb[:3]) - 1

    def sample(plane, xy):
        g = xy.view(1, 1, -1, 2).flip(-1)
        return F.grid_sample(plane, g, align_corners=False, padding_mode="border")[0, :, 0, :].transpose(0, 1)

    coords = ([0, 1], [0, 2], [1, 2])
    geo = ae_plane_block(sd, "geo_convs", [f[:, :geo_dim] for f in fm])
    tex = ae_plane_block(sd, "tex_convs", [f[:, geo_dim:] for f in fm])
    h_geo = sum(sample(geo[i], x[..., coords[i]]) for i in range(3))
    h_tex = sum(sample(tex[i], x[..., coords[i]]) for i in range(3))
    return torch.cat([_mlp(sd, "geo_decoder", h_geo, taps=taps), _mlp(sd, "tex_decoder", h_tex, taps=taps).sigmoid()], dim=1)


def ae_losses(pred, sdf, tex, sdf_threshold, tex_threshold_ratio=0.999, tex_weight=1.0, sdf_loss="weightedl1", tex_loss="l1",
              sdf_renorm=False):
    """ShapeAutoEncoder._forward_batch for data_type "sdftex", src/encoding/model.py:186-225: sdf loss `l1` | `weightedl1`
    over all rows; texture loss `l1` | `l2` (mse) | `huber` (delta 0.1), times tex_weight, over the rows whose |sdf| lies in
    the band sdf_threshold * ratio (1.0 * ratio with sdf_renorm, where the sdf samples are already divided by the threshold).
    The band test is the reference's: a float32 sdf tensor against a Python float, i.e. |sdf| < fl32(thr * ratio) with
    the product taken in double.  It is made on the float32 sdf even when the rest runs in float64 (sdf promoted from
    float32 converts back exactly), so a float64 port selects the rows the reference selects."""
    ps = pred[..., :1]
    if sdf_loss == "l1":
        l_sdf = F.l1_loss(ps, sdf)
    elif sdf_loss == "weightedl1":
        weight = 1 + 0.5 * torch.sign(sdf) * torch.sign(sdf - ps)
        l_sdf = ((ps - sdf).abs() * weight).mean()
    else:
        raise ValueError(f"sdf_loss {sdf_loss!r}")
    band = (1.0 if sdf_renorm else float(sdf_threshold)) * float(tex_threshold_ratio)
    mask = sdf.squeeze(1).float().abs() < band
    pt, gt = pred[..., 1:][mask], tex[mask]
    if tex_loss == "l1":
        l_tex = F.l1_loss(pt, gt)
    elif tex_loss == "l2":
        l_tex = F.mse_loss(pt, gt)
    elif tex_loss == "huber":
        l_tex = F.huber_loss(pt, gt, delta=0.1)
    else:
        raise ValueError(f"tex_loss {tex_loss!r}")
    return {"sdf_loss": l_sdf, "tex_loss": l_tex * tex_weight}


def ae_param_groups(names):
    """geo_parameters / tex_parameters of AutoEncoderGroupSkip (networks.py:146-150) as name lists."""
    geo = [n for n in names if n.startswith(("geo_encoder", "geo_convs", "geo_decoder"))]
    tex = [n for n in names if n.startswith(("tex_encoder", "tex_convs", "tex_decoder"))]
    return geo, tex
