#!/usr/bin/env python3
"""What known-region sampling costs per step at the scored size (128-ch UNet, 128^3 triplane, batch 1, DDPM-1000): the plain loop,
the loop with `known=`, and the loop with `known=` and `resample=2` (per model evaluation: its re-noise launches and the steps
that cannot carry the next in_conv are in the figure).  One process, the three variants interleaved round by round, timed by
device events around `--evals` consecutive evaluations of each loop; synthetic weights (same arithmetic).  Prints one JSON line;
profiles/edit.txt keeps it.

    python tools/bench_edit.py [--evals 200] [--rounds 5] [--mc 128] [--size 128]
"""
import argparse, json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from sin3dm_amd import testing as T
from sin3dm_amd.diffusion.gaussian_diffusion import KnownRegion
from sin3dm_amd.diffusion.script_util import create_gaussian_diffusion
from sin3dm_amd.diffusion.unet_triplane import TriplaneUNetModelSmall

ap = argparse.ArgumentParser()
ap.add_argument("--evals", type=int, default=200, help="model evaluations per timed window")
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--warmup", type=int, default=40, help="untimed evaluations at the start of every window's loop")
ap.add_argument("--mc", type=int, default=128)
ap.add_argument("--size", type=int, default=128)
a = ap.parse_args()
dev = torch.device("cuda:0")
H = W = D = a.size
shape = (1, 12, H + D, W + D)
model = TriplaneUNetModelSmall(12, a.mc, 12, use_scale_shift_norm=True)
model.load_state_dict(T.synthetic_state_dict(T.unet_param_shapes(model_channels=a.mc), 0)); model.to(dev).eval()
diffusion = create_gaussian_diffusion(steps=1000, predict_xstart=True, timestep_respacing="")
y0 = torch.tanh(torch.randn(shape[1:], device=dev))
mask = torch.zeros(shape[1:], device=dev); mask[:, : H // 2, :] = 1                    # the low-x half of xy and xz
known = KnownRegion(y0, mask)
variants = {"plain": {}, "known": dict(known=known), "known_resample2": dict(known=known, resample=2)}


def window(kw):
    it = diffusion.p_sample_loop_progressive(model, shape, model_kwargs=dict(H=H, W=W, D=D), device=dev, **kw)
    for _ in range(a.warmup):
        next(it)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.evals):
        next(it)
    e1.record(); torch.cuda.synchronize()
    it.close()
    return e0.elapsed_time(e1) / a.evals


window({})                                                                              # clocks, workspace, caches
ms = {k: [] for k in variants}
for _ in range(a.rounds):
    for k, kw in variants.items():
        ms[k].append(window(kw))
out = {"what": "ms per model evaluation, DDPM, batch 1", "mc": a.mc, "hwd": [H, W, D], "evals": a.evals, "rounds": a.rounds}
for k, v in ms.items():
    out[k] = {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
out["known_minus_plain_us"] = round(1e3 * (out["known"]["median"] - out["plain"]["median"]), 2)
out["resample2_minus_plain_us"] = round(1e3 * (out["known_resample2"]["median"] - out["plain"]["median"]), 2)
print(json.dumps(out))
