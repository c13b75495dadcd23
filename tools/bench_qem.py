#!/usr/bin/env python3
"""Quadric-error decimation (isosurface.simplify_mesh_quadric) next to the vertex clustering (simplify_mesh) on one MI355X: round
counts, time per stage and the RMS distance of the input vertices from the decimated surface (the exact closest-point kernel of
data/mesh_sampler.MeshSampler), on analytic iso-surfaces: a box with a box-shaped hole through it (sharp edges) and a bumpy torus.

    python tools/bench_qem.py [--reso 44 48 256 --divisor 50 --repeats 5] > profiles/qem.txt
"""
import argparse
import collections
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from sin3dm_amd import _lib
from sin3dm_amd.data.mesh_sampler import MeshSampler
from sin3dm_amd.encoding import isosurface as iso

ap = argparse.ArgumentParser()
ap.add_argument("--reso", type=int, nargs="+", default=[44, 256], help="grid sides of the box; the torus takes side + 4 up to 48")
ap.add_argument("--divisor", type=int, default=50, help="face budget = faces / divisor")
ap.add_argument("--n_faces", type=int, default=10000, help="face budget at grid sides above 64 (the export's default)")
ap.add_argument("--repeats", type=int, default=5)
args = ap.parse_args()
_lib.require_gpu()                                   # no GPU: fail, there is nothing to measure


def field(kind, n):
    """the fields of tests/test_qem_gpu.py at grid side n"""
    ax = np.linspace(-1, 1, n)
    x, y, z = np.meshgrid(ax + 0.0131, ax * 0.95 - 0.0072, ax * 1.05 + 0.0057, indexing="ij")
    if kind == "box":
        box = np.maximum(np.maximum(np.abs(x) - 0.71, np.abs(y) - 0.62), np.abs(z) - 0.53)
        hole = np.maximum(np.abs(x) - 0.31, np.abs(y) - 0.27)
        return np.maximum(box, -hole).astype(np.float32)
    f = np.sqrt((np.sqrt(x * x + y * y) - 0.6) ** 2 + z * z) - 0.24 + 0.03 * np.sin(7 * x) * np.sin(5 * y + 1) * np.sin(6 * z + 2)
    return f.astype(np.float32)


cur = collections.defaultdict(float)


def timed(label, fn):
    def wrapper(*a, **k):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn(*a, **k)
        e1.record()
        e1.synchronize()
        cur[label] += e0.elapsed_time(e1)
        return out
    return wrapper


def rms(points, v2, t2, band):
    dist, face, _ = MeshSampler(verts=v2.cpu().numpy(), faces=t2.cpu().numpy()).closest(points, band=band)
    miss = int((face < 0).sum())
    return float(torch.sqrt((dist.double() ** 2).mean())), miss


iso._qem_round = timed("  of which edges, cost, validity, selection (all rounds)", iso._qem_round)
quadric = timed("simplify_mesh_quadric", iso.simplify_mesh_quadric)
cluster = timed("simplify_mesh (vertex clustering)", iso.simplify_mesh)
print(f"quadric-error decimation next to vertex clustering, one MI355X; times: median of {args.repeats} runs after one warm-up, ms; "
      f"RMS: input vertices to the decimated surface, in grid cells")
for n in args.reso:
    for kind, side in (("box", n), ("torus", min(n + 4, 48) if n <= 64 else n)):
        v, t, _ = iso.marching_cubes(torch.from_numpy(field(kind, side)).cuda(), 0.0, 1.0)
        v, t, _ = iso.largest_component(v, t)
        budget = t.shape[0] // args.divisor if side <= 64 else args.n_faces
        runs = []
        for r in range(args.repeats + 1):
            cur.clear()
            torch.cuda.synchronize()
            vq, tq, iq = quadric(v, t, budget)
            vc, tc, ic = cluster(v, t, budget)
            runs.append(dict(cur))
        runs = runs[1:]
        print(f"\n{kind} {side}^3: {v.shape[0]} vertices / {t.shape[0]} faces, budget {budget}")
        for label in runs[0]:
            vals = [r[label] for r in runs]
            print(f"  {label:<58s} {statistics.median(vals):9.2f}  [{min(vals):8.2f} .. {max(vals):8.2f}]")
        per = [c for c, _ in iq["per_round"]]
        print(f"  quadric: {iq['rounds']} rounds, stuck {iq['stuck']}, {tq.shape[0]} faces / {vq.shape[0]} vertices; collapses per round: "
              f"first {per[:3]}, largest {max(per)}, last {per[-3:]}")
        print(f"  clustering: R = {ic['R']}, {tc.shape[0]} faces / {vc.shape[0]} vertices")
        band = 8.0 * side / 44.0
        (rq, mq), (rc, mc) = rms(v, vq, tq, band), rms(v, vc, tc, band)
        print(f"  RMS distance: quadric {rq:.5f}, clustering {rc:.5f}, ratio {rq / rc:.4f}   (vertices beyond the band of {band:.1f}: {mq}, {mc})")
