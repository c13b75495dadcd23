#!/usr/bin/env python3
"""Step time of the auto-encoder training iteration for the network variants the training tier covers, interleaved in ONE
process (round-robin, so that clock drift falls on all of them alike): sdftex (skip net, 3 colour channels), geo (geometry
only, data_type sdf), skip8 (skip net, 8 material channels, data_type sdfpbr) and pbr (the PBR net with its three material
heads, data_type sdfpbr with --enc_net_type pbr).  128^3 feature maps, 65 536 points per step,
AdamW included — the configuration of tools/bench_ae_train.py, whose default is the sdftex line.  Not the scored bench line.

    python tools/bench_ae_variants.py [--fm 128 128 128] [--points 65536] [--rounds 5] [--steps 10] [--only geo]

Prints one JSON line: ms per iteration (median over the rounds) per variant, its ratio to sdftex, and the ratio its FLOP count
predicts (forward flops as executed: the plane blocks with their input channels padded to 32, the MLPs per point; for pbr
one 5x5 and two 3x3 blocks and four MLPs), also relative to skip8 for pbr."""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import torch  # noqa: E402

from sin3dm_amd import testing as T  # noqa: E402
from sin3dm_amd.encoding.model import FlatGroupAdamW, ae_loss_cfg  # noqa: E402
from sin3dm_amd.encoding.networks import AutoEncoderGroupPBR, AutoEncoderGroupSkip  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--fm", type=int, nargs=3, default=(128, 128, 128))
ap.add_argument("--points", type=int, default=65536)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--only", default=None, help="one variant (for a kernel trace of its own); sdftex is always the base of the ratios otherwise")
args = ap.parse_args()
H, W, D = args.fm
N = args.points
dev = torch.device("cuda:0")
UP, HID = 64, 256
VARIANTS = {"sdftex": dict(use_tex=True, tc=3), "geo": dict(use_tex=False, tc=0), "skip8": dict(use_tex=True, tc=8),
            "pbr": dict(use_tex=True, tc=8, pbr=True)}


def flops(v):
    """forward flops of one iteration as executed here: per net a 5x5 block on 32-padded inputs and a 64 -> 64 5x5 conv per plane
    pixel, and the six-layer MLP per point (the projected encoder is 0.1 % of it)"""
    nets = 2 if v["use_tex"] else 1
    hw = H * W + H * D + W * D
    mlp = 2 * (UP * HID + 2 * HID * HID + (UP + HID) * HID + HID * HID)
    last = 2 * HID * (1 + v["tc"])
    if v.get("pbr"):
        # geometry side as above; texture side: tex_convs.0 at 3x3 with its 1x1 shortcut, tex_convs.1 (two 64 -> 64 3x3 convs), three heads
        geo = mlp * N + 2 * 25 * (32 * UP + UP * UP) * hw + 2 * 32 * UP * hw
        tex = 3 * mlp * N + 2 * 9 * (32 * UP + UP * UP) * hw + 2 * 32 * UP * hw + 2 * 9 * 2 * UP * UP * hw
        return geo + tex + last * N
    return nets * (mlp * N + 2 * 25 * (32 * UP + UP * UP) * hw + 2 * 32 * UP * hw) + last * N


def make(v):
    if v.get("pbr"):
        shapes = T.pbr_param_shapes(4, 8, UP, HID, 4, 8, with_encoder=True)
        net = AutoEncoderGroupPBR(4, 8, UP, HID, 4, tex_channels=8)
    else:
        shapes = (T.ae_param_shapes(4, 8, UP, HID, 4, v["tc"], with_encoder=True) if v["use_tex"]
                  else T.geo_only_param_shapes(4, UP, HID, 4, with_encoder=True))
        net = AutoEncoderGroupSkip(4, 8, UP, HID, 4, use_tex=v["use_tex"], tex_channels=max(v["tc"], 1))
    net.load_state_dict(T.synthetic_state_dict(shapes, 5), strict=False)
    net.to(dev)
    net.build_training_tier(**({"material_heads": True} if v.get("pbr") else {}))
    g = torch.Generator(device=dev).manual_seed(0)
    vol = torch.rand((1, 1 + v["tc"], 2 * H, 2 * W, 2 * D), device=dev, generator=g)
    vol[:, :1] = vol[:, :1] * 0.2 - 0.1
    net.set_volume(vol)
    pts = torch.rand((N, 3), device=dev, generator=g) * 2 - 1
    sdf = torch.rand((N, 1), device=dev, generator=g) * 0.1 - 0.05
    tex = torch.rand((N, v["tc"]), device=dev, generator=g) if v["tc"] else None
    opt = FlatGroupAdamW(net, 5e-3, 0.2, lr_decay=0.1 ** (1 / 25000))
    grad = torch.empty_like(net.flat_parameters)
    cfg = ae_loss_cfg("weightedl1", "l1", 0.05)

    def step():
        losses, _, gr = net.loss_and_grads(vol, pts, sdf, tex, cfg, grad_out=grad)
        opt.step(gr)
        return losses
    return net, step


runs = {}
if args.only:
    VARIANTS = {args.only: VARIANTS[args.only]}
for name, v in VARIANTS.items():
    net, step = make(v)
    for _ in range(args.warmup):
        step()
    runs[name] = (net, step, [])
    del net
torch.cuda.synchronize()
for _ in range(args.rounds):
    for name, (net, step, times) in runs.items():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            losses = step()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) / args.steps * 1e3)
        assert torch.isfinite(losses).all()
base = statistics.median(runs["sdftex"][2]) if "sdftex" in runs else float("nan")
line = {"what": "auto-encoder training iteration per network variant", "config": f"feature maps ({H},{W},{D}), {N} points/step",
        "rounds": args.rounds, "steps_per_round": args.steps}
for name, (net, step, times) in runs.items():
    assert torch.isfinite(net.flat_parameters).all()
    ms = statistics.median(times)
    line[name] = {"ms_per_step": round(ms, 3), "min": round(min(times), 3), "max": round(max(times), 3),
                  "ratio_to_sdftex": round(ms / base, 3), "flop_ratio_predicted": round(flops(VARIANTS[name]) / flops(dict(use_tex=True, tc=3)), 3)}
    if name == "pbr" and "skip8" in runs:
        line[name]["ratio_to_skip8"] = round(ms / statistics.median(runs["skip8"][2]), 3)
        line[name]["flop_ratio_to_skip8_predicted"] = round(flops(VARIANTS["pbr"]) / flops(VARIANTS["skip8"]), 3)
print(json.dumps(line), flush=True)
