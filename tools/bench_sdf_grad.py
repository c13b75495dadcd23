#!/usr/bin/env python3
"""The sdf gradient against what it replaces, on one MI355X in one process: the geometry-only net at full width (up 64,
hidden 256), a 128^3 triplane, N = 270 000 points (a 256^3 mesh's vertices) and N = 2^22, uniform in the box.

  decode              one decode of the geometry-only handle (k_decode, one head)
  7 x decode          what central differences cost today
  sdf_and_grad        s3d_decoder_sdf_grad, iters = 0: k_decode for the sdf's bits + k_decode_grad (forward for the ReLU
                      patterns, the chain transposed, the planes' derivative)
  project_to_surface  iters = 2: three such evaluations
  decode_mesh         ShapeAutoEncoder.decode_mesh at 256^3 (skip net with texture, save_voxel=False, files written) with the
                      defaults and with refine=2, normals="field"

Synthetic weights and features (same arithmetic as trained ones).  The plane stage and the transposed packs are built before
timing; the four are interleaved round by round after a warm-up round and timed with device events; medians and the spread
(min .. max) are reported.  Expectation from the FLOP count, not a gate: k_decode_grad's transposed products mirror the forward
ones, so it costs about two decodes and sdf_and_grad, with the k_decode launch in front, about three; the seven calls cost seven.

    python tools/bench_sdf_grad.py [--repeats 9] > profiles/sdf_grad.txt
"""
import argparse
import os
import statistics
import sys
import tempfile
from types import SimpleNamespace

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from sin3dm_amd import _lib, testing as T
from sin3dm_amd.encoding.model import ShapeAutoEncoder
from sin3dm_amd.encoding.networks import AutoEncoderGroupSkip

ap = argparse.ArgumentParser()
ap.add_argument("--fm", type=int, default=128, help="feature-map side (H = W = D)")
ap.add_argument("--repeats", type=int, default=9)
args = ap.parse_args()

_lib.require_gpu()                                   # no GPU: fail, there is nothing to measure
dev = torch.device("cuda:0")
UP, HID = 64, 256
AABB = torch.tensor([-1.0, -1, -1, 1, 1, 1])
fm = [torch.from_numpy(np.tanh(T.synthetic_noise((1, 4, args.fm, args.fm), s))).to(dev) for s in (1, 2, 3)]
net = AutoEncoderGroupSkip(4, 8, UP, HID, 4, use_tex=False)
net.load_state_dict(T.synthetic_state_dict(T.geo_only_param_shapes(4, UP, HID, 4), 5), strict=False)
net = net.to(dev).eval()
CELL = 2.0 / 256


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


print(f"geometry-only net, up {UP} / hidden {HID}, {args.fm}^3 triplane, {args.repeats} rounds after one warm-up, medians (min .. max) in ms")
for n in (270000, 2 ** 22):
    pts = torch.from_numpy(np.random.Generator(np.random.PCG64(n)).uniform(-1, 1, size=(n, 3)).astype(np.float32)).to(dev)
    runs = {
        "decode": lambda: net.decode(pts, fm, aabb=AABB),
        "7 x decode": lambda: [net.decode(pts, fm, aabb=AABB) for _ in range(7)][-1],
        "sdf_and_grad": lambda: net.sdf_and_grad(pts, fm, aabb=AABB)[1],
        "project_to_surface(iters=2)": lambda: net.project_to_surface(pts, fm, aabb=AABB, iters=2, max_step=CELL, max_move=CELL / 2)[2],
    }
    times = {k: [] for k in runs}
    for rep in range(args.repeats + 1):
        for label, fn in runs.items():
            ms, out = timed(fn)
            assert bool(torch.isfinite(out[::997]).all())
            if rep:
                times[label].append(ms)
    med = {k: statistics.median(v) for k, v in times.items()}
    print(f"\nN = {n}")
    for k, v in times.items():
        print(f"  {k:30s} {med[k]:9.3f}  ({min(v):.3f} .. {max(v):.3f})   {med[k] / med['decode']:5.2f} x decode")
    print(f"  sdf_and_grad / decode = {med['sdf_and_grad'] / med['decode']:.2f} (expected about 3: k_decode + about two decodes of k_decode_grad); "
          f"7 x decode / sdf_and_grad = {med['7 x decode'] / med['sdf_and_grad']:.2f}")
    print(f"  project_to_surface(iters=2) / sdf_and_grad = {med['project_to_surface(iters=2)'] / med['sdf_and_grad']:.2f} (expected 3)")

# ---------------------------------------------------------------- decode_mesh with and without refinement and field normals
cfg = SimpleNamespace(enc_net_type="skip", fdim_geo=4, fdim_tex=8, fdim_up=UP, hidden_dim=HID, n_hidden_layers=4, data_type="sdftex", gpu_id=0)
work = tempfile.mkdtemp(prefix="sdf_grad_")
ae = ShapeAutoEncoder(work, cfg, device=dev)
ae.net.load_state_dict(T.synthetic_state_dict(T.ae_param_shapes(), 5), strict=False)
ae.net.to(dev).eval()
ae.aabb = AABB.to(dev)
ae.net.reset_aabb(ae.aabb)
ae.featmap_size = (args.fm,) * 3
fm12 = [torch.from_numpy(np.tanh(T.synthetic_noise((1, 12, args.fm, args.fm), s))).to(dev) for s in (1, 2, 3)]
runs = {"decode_mesh": lambda: ae.decode_mesh(work, fm12, 256, save_voxel=False),
        'decode_mesh(refine=2, normals="field")': lambda: ae.decode_mesh(work, fm12, 256, save_voxel=False, refine=2, normals="field")}
times = {k: [] for k in runs}
reps = min(args.repeats, 3)
for rep in range(reps + 1):
    for label, fn in runs.items():
        ms, out = timed(fn)
        if rep:
            times[label].append(ms)
med = {k: statistics.median(v) for k, v in times.items()}
print(f"\ndecode_mesh at 256^3, {out[0].shape[0]} vertices, {out[1].shape[0]} faces, OBJ written, {reps} rounds after one warm-up (host time included)")
for k, v in times.items():
    print(f"  {k:42s} {med[k]:10.1f}  ({min(v):.1f} .. {max(v):.1f})")
a, b = med["decode_mesh"], med['decode_mesh(refine=2, normals="field")']
print(f"  refinement and normals add {b - a:.1f} ms ({100 * (b - a) / a:.1f} %): the projection of the vertices and the `vn` lines of the file")
