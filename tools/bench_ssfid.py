#!/usr/bin/env python3
"""Per-stage times of SSFID (sin3dm_amd.evaluation.ssfid, s3d_ssfid.hip) on one MI355X: procedural gyroid shapes
(sin3dm_amd.testing.gyroid_sdf) at 128^3 and at 128 x 104 x 88, 16 generated shapes plus the training shape, procedural classifier
weights.  The stages are timed by device events inside the library (s3d_ssfid_profile); the Frechet distances are host work and
are timed on the host.  Next to it PyTorch-ROCm eager runs the same two Conv3d / InstanceNorm3d / leaky_relu layers and torch.cov
(float64, as np.cov) on the same GPU, alternately in the same process; both paths are compared before they are timed.  Medians of
the repeats after a warm-up, [min .. max].

    python tools/bench_ssfid.py [--shapes 16 --repeats 7 --layer 2] > profiles/ssfid.txt
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import torch.nn.functional as F

from sin3dm_amd import _lib
from sin3dm_amd import evaluation as ev
from sin3dm_amd.testing import gyroid_sdf, synthetic_state_dict

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", type=int, default=16)
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--layer", type=int, default=2, choices=(1, 2))
ap.add_argument("--no_torch", action="store_true", help="skip the eager baseline")
args = ap.parse_args()

_lib.require_gpu()                                   # no GPU: fail, there is nothing to measure
W = synthetic_state_dict(ev.ssfid.PARAM_SHAPES, 7)
WD = {k: v.cuda() for k, v in W.items()}
STAGES = ("layer 1", "statistics 1", "layer 2", "statistics 2", "covariance")


def med(xs):
    return f"{statistics.median(xs):9.3f}  [{min(xs):.3f} .. {max(xs):.3f}]"


def eager(vox, layer):
    """The reference's forward and statistics with torch on the device."""
    x = vox.float()[None, None]
    a = F.leaky_relu(F.instance_norm(F.conv3d(x, WD["conv_1.weight"], WD["conv_1.bias"], stride=2, padding=1), eps=1e-5), 0.01)
    if layer == 2:
        a = F.leaky_relu(F.instance_norm(F.conv3d(a, WD["conv_2.weight"], WD["conv_2.bias"], stride=2, padding=1), eps=1e-5), 0.01)
    act = a.permute(0, 2, 3, 4, 1).reshape(-1, a.shape[1])
    act64 = act.double()
    return act64.mean(dim=0), torch.cov(act64.t()), act


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def run(shape):
    n = args.shapes
    vols = [torch.from_numpy(gyroid_sdf(shape, 2.5, (0.0, 0.0, 0.0)) <= 0).cuda()]
    vols += [torch.from_numpy(gyroid_sdf(shape, 2.5, (0.37 * i + 0.1, -0.21 * i, 0.13 * i + 0.2)) < 0).cuda() for i in range(n)]
    net = ev.VoxelClassifier(W)
    r1, r2 = int(np.prod([s // 2 for s in shape])), int(np.prod([s // 4 for s in shape]))
    print(f"SSFID per stage, one MI355X: {n} generated shapes + the training shape of {' x '.join(map(str, shape))}, out_layer {args.layer}: "
          f"{r1} rows x 32 at layer 1, {r2} rows x 64 at layer 2; median of {args.repeats} runs after one warm-up [min .. max], "
          f"ms for all {n + 1} shapes")
    # agreement before timing
    mu, sigma, act = net.features_device(vols[1], args.layer, return_activations=True)
    torch_ok = not args.no_torch
    if torch_ok:
        try:
            tmu, tsigma, tact = eager(vols[1], args.layer)
            torch.cuda.synchronize()
            print(f"  kernels vs eager torch on one shape: max |act| diff {float((act - tact).abs().max()):.2e}, "
                  f"mu {float((mu - tmu).abs().max()):.2e}, sigma {float((sigma - tsigma).abs().max()):.2e}")
        except Exception as e:                                            # (a missing convolution solver, for instance)
            torch_ok = False
            print(f"  eager torch baseline: not measured ({type(e).__name__}: {str(e)[:200]})")
    net.profile(True)
    stage = {s: [] for s in STAGES}
    ours, theirs, host = [], [], []
    for rep in range(args.repeats + 1):
        tot = [0.0] * 5
        stats = []
        whole = 0.0
        for v in vols:
            ms, out = event_ms(lambda: net.features_device(v, args.layer))
            whole += ms
            tot = [a + b for a, b in zip(tot, net.stage_ms())]
            stats.append((out[0].cpu().numpy(), out[1].cpu().numpy()))
        t0 = time.perf_counter()
        d = [ev.frechet_distance(*stats[0], *s) for s in stats[1:]]
        h = (time.perf_counter() - t0) * 1e3
        tw = 0.0
        if torch_ok:
            for v in vols:
                tw += event_ms(lambda: eager(v, args.layer)[:2])[0]
        if rep:                                                           # the first pass is the warm-up
            for s, t in zip(STAGES, tot):
                stage[s].append(t)
            ours.append(whole)
            host.append(h)
            theirs.append(tw)
    for s in STAGES:
        print(f"  {s:<40s} {med(stage[s])}")
    print(f"  {'all five, one call per shape (events)':<40s} {med(ours)}")
    print(f"  {'Frechet distances on the host (' + str(n) + ')':<40s} {med(host)}")
    if torch_ok:
        print(f"  {'eager torch: forward + torch.cov':<40s} {med(theirs)}     torch / kernels {statistics.median(theirs) / statistics.median(ours):.2f}x")
    per = statistics.median(stage["layer 2"]) / (n + 1)
    if args.layer == 2 and per > 0:
        flop = 2.0 * r2 * 64 * 2048
        print(f"  layer 2 per shape: {per * 1e3:.1f} us, {flop / 1e9:.2f} GFLOP -> {flop / per / 1e9:.1f} TFLOP/s of float32 MFMA")
    per1 = statistics.median(stage["layer 1"]) / (n + 1)
    print(f"  layer 1 per shape: {per1 * 1e3:.1f} us, {r1 * 32 * 4 / 1e6:.1f} MB stored -> {r1 * 32 * 4 / per1 / 1e9:.2f} TB/s of stores")
    print(f"  SSFID_avg {np.mean(d):.6f} SSFID_std {np.std(d):.6f}")


for shape in ((128, 128, 128), (128, 104, 88)):
    run(shape)
