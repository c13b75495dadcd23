#!/usr/bin/env python3
"""Generate tests/golden/ae_pbr.npz by IMPORTING the reference (PyTorch-CPU, autograd): the training iteration of
AutoEncoderGroupPBR with texture (data_type sdfpbr, --enc_net_type pbr) — cases, inputs and sizes are those of
tests/ae_pbr_cases.py.

Data only (make_golden.py's rules): the reference's outputs.  Inputs and weights are NOT stored: they are regenerated from
tests/ae_pbr_cases.py (volume, batch, state_dict); this script asserts that the manifest equals the reference module's own
state_dict.  Only the batch seeds it picked are stored.

    python tests/golden/make_golden_ae_pbr.py

Per case: `encode` (xy, xz, yz), `pred`, the four losses, the digest of every parameter gradient (make_golden.grad_digest; the
gradients of tex_encoder.weight, tex_convs.0.shortcut.weight and tex_convs.1.norm_* in full) and three optimiser iterations
(`steps.*`: AdamW in two groups, geo at lr * split, weight_decay 0.01, ExponentialLR).  A batch is taken only if no hidden ReLU
pre-activation of any of the FOUR MLPs lies within 2e-6 of zero (pick_batch's rule), and no |pred - target| of a loss term —
the material residuals are taken without a sigmoid — lies within 1e-6 of zero.

Every compared quantity is also evaluated with the reference in float64; `<case>.gap.<quantity>` is the reference's own
float32-versus-float64 difference in the metric of the test (conftest.relerr / digest_errors).
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden import grad_digest, quiet, save  # noqa: E402  (puts the reference on sys.path)

import ae_pbr_cases as P  # noqa: E402
from ae_variants_cases import BOUNDS as V_BOUNDS  # noqa: E402
from conftest import digest_errors, relerr  # noqa: E402
from encoding.networks import AutoEncoderGroupPBR  # noqa: E402


class Files(dict):
    """a dict that looks like an opened .npz to conftest.digest_errors"""
    @property
    def files(self):
        return list(self)


def make(case, dtype=torch.float32):
    net = quiet(AutoEncoderGroupPBR, *P.CASES[case]["args"], use_tex=True, tex_channels=P.TEX_CHANNELS)
    shapes = P.shapes(case)
    ref = {k: tuple(v.shape) for k, v in net.state_dict().items() if k != "aabb"}
    assert list(ref) == list(shapes) and all(ref[k] == tuple(shapes[k]) for k in ref), sorted(set(ref) ^ set(shapes))
    missing, unexpected = net.load_state_dict(P.state_dict(case), strict=False)
    assert not unexpected and missing == ["aabb"], (missing, unexpected)
    quiet(net.reset_aabb, torch.tensor(P.AABB))
    return net.train().to(dtype)


def ref_losses(pred, sdf, tex):
    """ShapeAutoEncoder._forward_batch (src/encoding/model.py:186-237) with sdf_loss weightedl1, tex_loss l1, sdf_renorm 0 for
    data_type sdfpbr — restated, as in make_golden.ae_losses, because encoding.model does not import here."""
    ps = pred[..., :1]
    weight = 1 + 0.5 * torch.sign(sdf) * torch.sign(sdf - ps)
    out = {"sdf_loss": ((ps - sdf).abs() * weight).mean()}
    mask = sdf.squeeze(1).float().abs() < P.THR * P.RATIO
    pt, gt = pred[..., 1:], tex
    out["rgb_loss"] = torch.nn.functional.l1_loss(pt[mask, :3], gt[mask, :3])
    out["mr_loss"] = torch.nn.functional.l1_loss(pt[mask, 3:5], gt[mask, 3:5])
    out["normal_loss"] = torch.nn.functional.l1_loss(pt[mask, 5:], gt[mask, 5:])
    return out


def tensors(case, seed, dtype):
    return [torch.from_numpy(a).to(dtype) for a in P.batch(case, seed)]


def well_conditioned(case, net, vol, seed):
    pts, sdf, tex = tensors(case, seed, torch.float32)
    margins = []
    relus = [m for m in net.modules() if isinstance(m, torch.nn.ReLU)]
    assert len(relus) >= 4                                            # the geometry MLP and the three heads
    hooks = [m.register_forward_hook(lambda mod, i, o: margins.append(float(i[0].abs().min()))) for m in relus]
    with torch.no_grad():
        pred = net(vol, pts)
    for h in hooks:
        h.remove()
    assert len(margins) >= 4 * 5, len(margins)                        # five hidden layers of each of the four MLPs
    mask = sdf.squeeze(1).abs() < P.THR * P.RATIO
    resid = torch.minimum((pred[:, :1] - sdf).abs().min(), (pred[:, 1:] - tex)[mask].abs().min())     # (no sigmoid on the materials)
    inside = float(mask.float().mean())
    assert 0.1 <= inside <= 0.9, inside                               # both sides of the texture band are populated
    return min(margins) > 2e-6 and float(resid) > 1e-6


def pick_batch(case, net, vol, seed0):
    for seed in range(seed0, seed0 + 50):
        if well_conditioned(case, net, vol, seed):
            return seed
    raise RuntimeError("no well-conditioned batch found")


def iteration(case, net, vol, seed):
    dtype = next(net.parameters()).dtype
    pts, sdf, tex = tensors(case, seed, dtype)
    with torch.enable_grad():
        fm = net.encode(vol)
        pred = net(vol, pts)
        ls = ref_losses(pred, sdf, tex)
        net.zero_grad()
        sum(ls.values()).backward()
    grads = {k: (p.grad if p.grad is not None else torch.zeros_like(p)).detach().clone() for k, p in net.named_parameters()}
    return [f.detach() for f in fm], pred.detach(), torch.stack([ls[k].detach() for k in P.LOSS_NAMES]), grads


def three_steps(case, net, vol, seeds=None, seed0=0):
    """seeds None: every batch is picked with the network as it stands at that step (make_golden.gen_ae_train)"""
    lr, split, decay = P.STEPS_HYPER
    opt = torch.optim.AdamW([{"params": net.geo_parameters(), "lr": lr * split}, {"params": net.tex_parameters(), "lr": lr}], lr)
    sched = torch.optim.lr_scheduler.ExponentialLR(opt, decay)
    init = {k: p.detach().clone() for k, p in net.named_parameters()}
    dtype = next(net.parameters()).dtype
    ls_all, used = [], []
    for step in range(3):
        seed = seeds[step] if seeds is not None else pick_batch(case, net, vol, seed0 + 30 * step)
        used.append(seed)
        pts, sdf, tex = tensors(case, seed, dtype)
        with torch.enable_grad():
            ls = ref_losses(net(vol, pts), sdf, tex)
            opt.zero_grad()
            sum(ls.values()).backward()
        opt.step()
        sched.step()
        ls_all.append([float(ls[k]) for k in P.LOSS_NAMES])
    return used, np.asarray(ls_all), {k: p.detach() - init[k] for k, p in net.named_parameters()}


def main():
    out = {}
    for ci, case in enumerate(P.CASES):
        vol = torch.from_numpy(P.volume(case))
        net = make(case)
        assert sum(p.numel() for p in net.geo_parameters()) + sum(p.numel() for p in net.tex_parameters()) == \
            sum(p.numel() for p in net.parameters())
        seed = pick_batch(case, net, vol, 3300 + 100 * ci)
        fm, pred, ls, grads = iteration(case, net, vol, seed)
        full = tuple(k for k in grads if k in ("tex_encoder.weight", "tex_convs.0.shortcut.weight") or k.startswith("tex_convs.1.norm_"))
        out[f"{case}.seed"] = np.asarray(seed)
        out[f"{case}.xy"], out[f"{case}.xz"], out[f"{case}.yz"] = fm
        out[f"{case}.pred"], out[f"{case}.losses"] = pred, ls
        grad_digest(grads, f"{case}.grad", out, full_max=512, full_names=full)

        # the same iteration with the reference in float64: its own float32 round-off in the metrics of the test
        net64 = make(case, torch.float64)
        fm64, pred64, ls64, grads64 = iteration(case, net64, vol.double(), seed)
        g64 = Files()
        grad_digest(grads64, "g", g64, full_max=512, full_names=full)
        g64 = Files((k, v.numpy() if isinstance(v, torch.Tensor) else v) for k, v in g64.items())
        w = digest_errors({k: v.numpy() for k, v in grads.items()}, g64, "g")
        gap = {"encode": max(relerr(a.numpy(), b.numpy()) for a, b in zip(fm, fm64)), "pred": relerr(pred.numpy(), pred64.numpy()),
               "loss": float((ls.double() - ls64).abs().max()), "grad.norm": w["norm"], "grad.proj": w["proj"], "grad.full": w["full"]}

        # three optimiser iterations on batches that are well conditioned where the float32 run meets them
        seeds, sl, dparam = three_steps(case, make(case), vol, None, 3400 + 100 * ci)
        out[f"{case}.steps.seeds"], out[f"{case}.steps.losses"] = np.asarray(seeds), sl
        out[f"{case}.steps.hyper"] = np.asarray(P.STEPS_HYPER)
        grad_digest(dparam, f"{case}.steps.dparam", out, full_max=64)
        _, sl64, dparam64 = three_steps(case, make(case, torch.float64), vol.double(), seeds)
        d64 = Files()
        grad_digest(dparam64, "d", d64, full_max=64)
        d64 = Files((k, v.numpy() if isinstance(v, torch.Tensor) else v) for k, v in d64.items())
        skip = {k for k, g in grads64.items() if float(g.norm()) < 1e-6 * max(float(x.norm()) for x in grads64.values())}
        w = digest_errors({k: v.numpy() for k, v in dparam.items()}, d64, "d", skip)
        gap["steps.norm"], gap["steps.proj"] = w["norm"], w["proj"]
        gap["steps.loss"] = float(np.abs(sl - sl64).max())
        for k, v in gap.items():
            out[f"{case}.gap.{k}"] = np.asarray(v)
        print(case, "seed", seed, "steps", seeds, "losses", ls.numpy(), "\n   fp32-vs-fp64 gaps:",
              " ".join(f"{k} {v:.2e}" for k, v in gap.items()))
        for k, v in gap.items():
            if k in P.BOUNDS[case] and 10 * v > V_BOUNDS[k]:
                print(f"   note: 10 x the reference's own gap of {k} ({v:.2e}) exceeds the shared bound {V_BOUNDS[k]:.0e}")
    save("ae_pbr", **out)


if __name__ == "__main__":
    main()
