#!/usr/bin/env python3
"""decode_grid of the three decoder variants on one MI355X in one run: variant 0 (skip net, sdf + rgb), variant 1 (geometry
only) and variant 2 (AutoEncoderGroupPBR: sdf + rgb + mr + normal), all on k_decode with their head tables.  Full-width nets (up 64,
hidden 256), a 128^3 triplane, reso 256 over a cubic aabb = 16.8 M points.  Synthetic weights and features (same arithmetic as
trained ones).  The plane stage is run once per net before timing (it is cached per triplane); each timed call is one fused
launch, timed with device events, the three variants interleaved round by round after a warm-up round; medians are reported.

FLOPs are counted from the shapes: per point and MLP chain 2 * (up*hid + 2*hid*hid + (up+hid)*hid + hid*hid + hid*out); the
gather's 3 planes x 4 taps x up multiply-adds per feature group are added.  By that count variant 2 is ~2.0x and variant 1
~0.5x variant 0; the measured ratios are printed next to it.

    python tools/bench_pbr_decode.py [--reso 256 --fm 128 --repeats 9] > profiles/pbr_decode.txt
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from sin3dm_amd import _lib, testing as T
from sin3dm_amd.encoding.networks import AutoEncoderGroupPBR, AutoEncoderGroupSkip

ap = argparse.ArgumentParser()
ap.add_argument("--reso", type=int, default=256)
ap.add_argument("--fm", type=int, default=128, help="feature-map side (H = W = D)")
ap.add_argument("--repeats", type=int, default=9)
args = ap.parse_args()

_lib.require_gpu()                                   # no GPU: fail, there is nothing to measure
dev = torch.device("cuda:0")
UP, HID = 64, 256
AABB = torch.tensor([-1.0, -1, -1, 1, 1, 1])
fm12 = [torch.from_numpy(np.tanh(T.synthetic_noise((1, 12, args.fm, args.fm), s))).to(dev) for s in (1, 2, 3)]
fm4 = [f[:, :4].contiguous() for f in fm12]


def chain_flops(out):
    return 2.0 * (UP * HID + 2 * HID * HID + (UP + HID) * HID + HID * HID + HID * out)


GATHER = 2.0 * 3 * 4 * UP
VARIANTS = {
    "variant 0  skip net, sdf + rgb, 2 heads": (AutoEncoderGroupSkip(4, 8, UP, HID, 4), T.ae_param_shapes(4, 8, UP, HID, 4), fm12,
                                                 chain_flops(1) + chain_flops(3) + 2 * GATHER),
    "variant 1  geometry only, 1 head": (AutoEncoderGroupSkip(4, 8, UP, HID, 4, use_tex=False), T.geo_only_param_shapes(4, UP, HID, 4), fm4,
                                          chain_flops(1) + GATHER),
    "variant 2  PBR net, 4 heads": (AutoEncoderGroupPBR(4, 8, UP, HID, 4, tex_channels=8), T.pbr_param_shapes(4, 8, UP, HID, 4, 8), fm12,
                                     chain_flops(1) + chain_flops(3) + chain_flops(2) + chain_flops(3) + 2 * GATHER),
}
nets = {}
for label, (net, shapes, fm, flops) in VARIANTS.items():
    net.load_state_dict(T.synthetic_state_dict(shapes, 5), strict=False)
    nets[label] = (net.to(dev).eval(), fm, flops)

times = {k: [] for k in nets}
npts = None
for rep in range(args.repeats + 1):                  # round 0 is the warm-up (plane stage, code objects, allocations)
    for label, (net, fm, _) in nets.items():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = net.decode_grid(fm, args.reso, aabb=AABB)
        e1.record()
        e1.synchronize()
        if rep:
            times[label].append(e0.elapsed_time(e1))
        npts = out.shape[0] * out.shape[1] * out.shape[2]
        assert bool(torch.isfinite(out[::16, ::16, ::16]).all())
        del out

print(f"decode_grid, reso {args.reso} ({npts} points), {args.fm}^3 triplane, up {UP}, hidden {HID}; {args.repeats} interleaved rounds after one "
      f"warm-up round, device events (the output allocation is inside the window)")
print(f"device: {torch.cuda.get_device_name(0)}")
base = None
rows = {}
for label, (_, _, flops) in nets.items():
    t = times[label]
    med = statistics.median(t)
    rows[label] = (med, flops)
    print(f"{label:48s} median {med:8.3f} ms   min {min(t):8.3f}   max {max(t):8.3f}   {flops / 1e6:5.3f} MFLOP/point   "
          f"{flops * npts / (med * 1e-3) / 1e12:6.1f} TF/s")
k0, k1, k2 = list(rows)
for label, k in (("variant 1 / variant 0", k1), ("variant 2 / variant 0", k2)):
    print(f"{label}: measured {rows[k][0] / rows[k0][0]:.3f}x   by FLOP count {rows[k][1] / rows[k0][1]:.3f}x")
