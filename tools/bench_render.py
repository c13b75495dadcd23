#!/usr/bin/env python3
"""Per-stage times of the mesh rasteriser (sin3dm_amd.rendering, s3d_render.hip) on one MI355X: the reference's eight views at
512 x 512, supersample 2 (a 1024 x 1024 sample grid), of a procedural textured mesh — a bumpy torus of about 10 000 faces (the
size of an exported sample) and one of about 270 000 (the size of an undecimated iso-surface at 256^3) with a 1024 x 1024 image.
Stages are timed by device events recorded between them (rasterizer.render_views(timer=)); `scan` and `sort and segments` are
the torch calls between the kernels and include the host read of the pair count.  Medians of the repeats after a warm-up,
[min .. max], summed over the eight views; beside them the number of (tile, triangle) pairs and the longest tile list per view.
The depth band of tests/render_cases.py is measured here as well (on the CPU).

    python tools/bench_render.py [--repeats 7] > profiles/render.txt
"""
import argparse
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import numpy as np
import torch

import render_cases as R
from sin3dm_amd import _lib
from sin3dm_amd.rendering import rasterizer

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--resolution", type=int, nargs=2, default=(512, 512))
ap.add_argument("--supersample", type=int, default=2)
args = ap.parse_args()

_lib.require_gpu()                                   # no GPU: fail, there is nothing to measure
STAGES = ("project", "bin count", "scan", "bin fill", "sort and segments", "raster", "shade")


def torus(n):
    """A bumpy torus on an n x n parameter grid: 2 n^2 faces, per-corner uv = the parameters."""
    a = np.arange(n) / n * 2 * np.pi
    u, v = np.meshgrid(a, a, indexing="ij")
    r = 0.35 + 0.05 * np.sin(5 * u) * np.cos(3 * v)
    p = np.stack([(1.0 + r * np.cos(v)) * np.cos(u), r * np.sin(v) + 0.1 * np.sin(2 * u), (1.0 + r * np.cos(v)) * np.sin(u)], 2).reshape(-1, 3)
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    i1, j1 = (i + 1) % n, (j + 1) % n
    q = lambda x, y: (x * n + y).reshape(-1)                                          # noqa: E731
    faces = np.concatenate([np.stack([q(i, j), q(i1, j), q(i1, j1)], 1), np.stack([q(i, j), q(i1, j1), q(i, j1)], 1)])
    fu = lambda x, y: np.stack([x.reshape(-1) / n, y.reshape(-1) / n], 1)             # noqa: E731 (the seam runs to 1, not back to 0)
    uvs = np.concatenate([np.stack([fu(i, j), fu(i + 1, j), fu(i + 1, j + 1)], 1), np.stack([fu(i, j), fu(i + 1, j + 1), fu(i, j + 1)], 1)])
    return p.astype(np.float32), faces.astype(np.int32), uvs.astype(np.float32)


def texture(T=1024):
    y, x = np.meshgrid(np.arange(T), np.arange(T), indexing="ij")
    return np.stack([(x * 255 // T), (y * 255 // T), 255 * (((x // 32) + (y // 32)) % 2)], 2).astype(np.uint8)


def med(xs):
    return f"{statistics.median(xs):9.3f}  [{min(xs):.3f} .. {max(xs):.3f}]"


def run(n):
    v, f, uv = torus(n)
    verts, faces, uvs = torch.from_numpy(v).cuda(), torch.from_numpy(f).cuda(), torch.from_numpy(uv).cuda()
    mats = [{"Kd": (1.0, 1.0, 1.0), "image": torch.from_numpy(texture()).cuda()}]
    W, H = args.resolution
    kw = dict(uvs=uvs, materials=mats, resolution=(W, H), supersample=args.supersample)
    _, bufs = rasterizer.render_views(verts, faces, return_buffers=True, **kw)        # warm-up, and the counts
    pairs = [b["info"]["n_pairs"] for b in bufs]
    longest = [b["info"]["longest_tile_list"] for b in bufs]
    dropped = sum(b["info"]["dropped"] for b in bufs)
    covered = [float((b["face_id"] >= 0).float().mean()) for b in bufs]
    per_stage = {s: [] for s in STAGES}
    total = []
    for _ in range(args.repeats):
        marks = []

        def timer(stage):
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            marks.append((stage, e))
        rasterizer.render_views(verts, faces, timer=timer, **kw)
        torch.cuda.synchronize()
        acc = {s: 0.0 for s in STAGES}
        for (_, e0), (s, e1) in zip(marks[:-1], marks[1:]):
            if s != "start":
                acc[s] += e0.elapsed_time(e1)
        for s in STAGES:
            per_stage[s].append(acc[s])
        total.append(sum(acc.values()))
    print(f"eight views of {W} x {H}, supersample {args.supersample}, of a textured torus of {len(f)} faces / {len(v)} vertices; "
          f"median of {args.repeats} runs after one warm-up [min .. max], ms for all eight views")
    for s in STAGES:
        print(f"  {s:<28}{med(per_stage[s])}")
    print(f"  {'all stages (events)':<28}{med(total)}")
    print(f"  (tile, triangle) pairs per view: {min(pairs)} .. {max(pairs)}; longest tile list per view: {min(longest)} .. {max(longest)}; "
          f"dropped triangles: {dropped}; covered share of the samples: {min(covered):.3f} .. {max(covered):.3f}")


print(f"depth band of tests/render_cases.py: largest relative float32 / float64 gap of the depth formula over every covering (sample, "
      f"triangle) of every case, measured on the CPU: {R.measure_depth_gap():.3e}; recorded gap {R.DEPTH_GAP:.1e}, band = 10 x gap = "
      f"{R.DEPTH_BAND:.1e}")
run(71)
run(368)
