#!/usr/bin/env python3
"""What the DPM-Solver++ multistep update costs per model evaluation at the scored size (128-ch UNet, 128^3
triplane, batch 1): the DDIM loop (eta = 0), dpmpp2m and dpmpp2m_sde.  One process, the three loops interleaved round by round, timed
by device events around `--evals` consecutive evaluations of each; synthetic weights (same arithmetic); all three on the full
1000-step schedule so that a window is one stretch of a loop (the per-evaluation work does not depend on the spacing).  The new step
reads one more x-sized tensor than DDIM (x0_prev); the DDIM figure of the same run is what to read it against.
Then the gaps of the loop tests (tests/test_multistep_gpu.py) at their shapes: dpmpp2m at logsnr10 and dpmpp2m_sde at "20" against the
same loop on the CPU port, dpmpp1 against ddim_sample_loop(eta = 0) — max|a - b| / max|b|, to be read against 2e-4.
Prints one JSON line; profiles/multistep.txt keeps it.

    python tools/bench_multistep.py [--evals 150] [--rounds 5] [--mc 128] [--size 128] [--no-gaps]
"""
import argparse, json, os, statistics, sys
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np
import torch
from sin3dm_amd import testing as T
from sin3dm_amd.diffusion.script_util import create_gaussian_diffusion
from sin3dm_amd.diffusion.unet_triplane import TriplaneUNetModelSmall

ap = argparse.ArgumentParser()
ap.add_argument("--evals", type=int, default=150, help="model evaluations per timed window")
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--warmup", type=int, default=40, help="untimed evaluations at the start of every window's loop")
ap.add_argument("--mc", type=int, default=128)
ap.add_argument("--size", type=int, default=128)
ap.add_argument("--no-gaps", action="store_true")
a = ap.parse_args()
dev = torch.device("cuda:0")


def make_model(mc):
    m = TriplaneUNetModelSmall(12, mc, 12, use_scale_shift_norm=True)
    m.load_state_dict(T.synthetic_state_dict(T.unet_param_shapes(model_channels=mc), 0))
    return m.to(dev).eval()


H = W = D = a.size
shape = (1, 12, H + D, W + D)
model = make_model(a.mc)
diffusion = create_gaussian_diffusion(steps=1000, predict_xstart=True, timestep_respacing="")
kw = dict(model_kwargs=dict(H=H, W=W, D=D), device=dev)
variants = {"ddim": lambda: diffusion.ddim_sample_loop_progressive(model, shape, eta=0.0, **kw),
            "dpmpp2m": lambda: diffusion.multistep_sample_loop_progressive(model, shape, order=2, sde=False, **kw),
            "dpmpp2m_sde": lambda: diffusion.multistep_sample_loop_progressive(model, shape, order=2, sde=True, **kw)}


def window(make):
    it = make()
    for _ in range(a.warmup):
        next(it)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.evals):
        next(it)
    e1.record(); torch.cuda.synchronize()
    it.close()
    return e0.elapsed_time(e1) / a.evals


window(variants["ddim"])                                                                # clocks, workspace, caches
ms = {k: [] for k in variants}
for _ in range(a.rounds):
    for k, make in variants.items():
        ms[k].append(window(make))
out = {"what": "ms per model evaluation, batch 1", "mc": a.mc, "hwd": [H, W, D], "evals": a.evals, "rounds": a.rounds}
for k, v in ms.items():
    out[k] = {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
out["dpmpp2m_minus_ddim_us"] = round(1e3 * (out["dpmpp2m"]["median"] - out["ddim"]["median"]), 2)
out["dpmpp2m_sde_minus_ddim_us"] = round(1e3 * (out["dpmpp2m_sde"]["median"] - out["ddim"]["median"]), 2)

if not a.no_gaps:
    sys.path.insert(0, os.path.join(REPO, "oracle"))
    import torch_port as tp
    relerr = lambda x, y: float((x - y).abs().max() / y.abs().max())
    mc, (h, w, d), B = 32, (10, 14, 6), 2
    shp = (B, 12, h + d, w + d)
    small = make_model(mc)
    sd = T.synthetic_state_dict(T.unet_param_shapes(model_channels=mc), 0)
    xT = torch.from_numpy(T.synthetic_noise(shp, 7)).to(dev)
    gaps = {}
    for name, order, sde, resp in (("dpmpp2m_logsnr10_vs_cpu_port", 2, False, "logsnr10"), ("dpmpp2m_sde_20_vs_cpu_port", 2, True, "20")):
        diff = create_gaussian_diffusion(steps=1000, predict_xstart=True, timestep_respacing=resp)
        eps = [torch.from_numpy(T.synthetic_noise(shp, 100 + k)).to(dev) for k in range(diff.num_timesteps)]
        it = iter(eps)
        diff.noise_fn = lambda like: next(it)
        got = diff.multistep_sample_loop(small, shp, order=order, sde=sde, noise=xT, model_kwargs=dict(H=h, W=w, D=d)).cpu()
        tab64, orders = diff.multistep_tables(order, sde)
        tab = torch.from_numpy(tab64.astype(np.float32))
        x, x0_prev = xT.cpu(), None
        with torch.no_grad():
            for i in range(diff.num_timesteps - 1, -1, -1):
                x0 = tp.unet_forward(sd, x, torch.full((B,), float(diff.timestep_map[i])), h, w, d, mc).clamp(-1, 1)
                s = tab[0, i] * x + tab[1, i] * x0
                if orders[i] == 2:
                    s = s + tab[2, i] * x0_prev
                if sde:
                    s = s + tab[3, i] * eps[diff.num_timesteps - 1 - i].cpu()
                x, x0_prev = s, x0
        gaps[name] = float(f"{relerr(got, x):.3e}")
    diff = create_gaussian_diffusion(steps=1000, predict_xstart=True, timestep_respacing="logsnr10")
    lk = dict(noise=xT, model_kwargs=dict(H=h, W=w, D=d))
    gaps["dpmpp1_vs_ddim_eta0_logsnr10"] = float(f"{relerr(diff.multistep_sample_loop(small, shp, order=1, **lk).cpu(), diff.ddim_sample_loop(small, shp, eta=0.0, **lk).cpu()):.3e}")
    out["loop_gaps_relerr"] = gaps
print(json.dumps(out))
