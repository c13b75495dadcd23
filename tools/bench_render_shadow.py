#!/usr/bin/env python3
"""Times of the shadows of the PBR renders (sin3dm_amd.rendering, s3d_ray.hip) on one MI355X: the reference's eight
views at 512 x 512, supersample 2, of the two bumpy tori of tools/bench_render_pbr.py (10 082 and 270 848 faces) under the
three-light rig, smooth shading.  Interleaved in one process, per mesh: the ray grid's build (once per call: binning, scan, sort,
segments), the shadow mask (summed over the eight views), and the shade stage with and without the mask — at the default grid and
at half and double its resolution.  Stages are timed by device events recorded between them; medians of the repeats after a
warm-up, [min .. max].  In front: the float32 gap of tests/render_shadow_cases.py and the band derived from it, measured on the CPU.

    python tools/bench_render_shadow.py [--repeats 7] > profiles/render_shadow.txt
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

import render_shadow_cases as S
from sin3dm_amd import _lib
from sin3dm_amd.rendering import rasterizer

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--resolution", type=int, nargs=2, default=(512, 512))
ap.add_argument("--supersample", type=int, default=2)
ap.add_argument("--gaps-only", action="store_true", help="the CPU part alone (no GPU needed)")
args = ap.parse_args()


def torus(n):
    """The bumpy torus of tools/bench_render_pbr.py on an n x n parameter grid: 2 n^2 faces."""
    a = np.arange(n) / n * 2 * np.pi
    u, v = np.meshgrid(a, a, indexing="ij")
    r = 0.35 + 0.05 * np.sin(5 * u) * np.cos(3 * v)
    p = np.stack([(1.0 + r * np.cos(v)) * np.cos(u), r * np.sin(v) + 0.1 * np.sin(2 * u), (1.0 + r * np.cos(v)) * np.sin(u)], 2).reshape(-1, 3)
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    i1, j1 = (i + 1) % n, (j + 1) % n
    q = lambda x, y: (x * n + y).reshape(-1)                                          # noqa: E731
    faces = np.concatenate([np.stack([q(i, j), q(i1, j), q(i1, j1)], 1), np.stack([q(i, j), q(i1, j1), q(i, j1)], 1)])
    return p.astype(np.float32), faces.astype(np.int32)


def med(xs):
    return f"{statistics.median(xs):9.3f}  [{min(xs):.3f} .. {max(xs):.3f}]"


def staged(verts, faces, cols, **kw):
    """{stage: ms} of one render_views call, summed over the views"""
    marks = []

    def timer(stage):
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        marks.append((stage, e))
    rasterizer.render_views(verts, faces, vertex_colors=cols, resolution=tuple(args.resolution), supersample=args.supersample, shading="smooth",
                            timer=timer, **kw)
    torch.cuda.synchronize()
    acc = {}
    for (_, e0), (s, e1) in zip(marks[:-1], marks[1:]):
        if s != "start":
            acc[s] = acc.get(s, 0.0) + e0.elapsed_time(e1)
    return acc


def run(n):
    v, f = torus(n)
    verts, faces = torch.from_numpy(v).cuda(), torch.from_numpy(f).cuda()
    cols = torch.from_numpy((0.5 + 0.5 * v / np.abs(v).max()).astype(np.float32)).cuda()
    lo, hi = v.min(0).astype(np.float64), v.max(0).astype(np.float64)
    default = rasterizer.ray_grid_box(lo, hi, len(f))[2]
    grids = {"half": tuple(max(1, d // 2) for d in default), "default": tuple(default), "double": tuple(min(256, 2 * d) for d in default)}
    W, H = args.resolution
    print(f"eight views of {W} x {H}, supersample {args.supersample}, of a torus of {len(f)} faces / {len(v)} vertices, three lights; median of "
          f"{args.repeats} interleaved runs after one warm-up [min .. max], ms; mask and shade for all eight views")
    configs = [("no shadows", {})] + [(name, dict(shadows=True, shadow_grid=g)) for name, g in grids.items()]
    for _, kw in configs:
        staged(verts, faces, cols, **kw)                                              # warm-up
    times = {name: [] for name, _ in configs}
    for _ in range(args.repeats):
        for name, kw in configs:                                                      # interleaved
            times[name].append(staged(verts, faces, cols, **kw))
    base = [t["shade"] for t in times["no shadows"]]
    print(f"  {'no shadows':<28}{'shade':<10}{med(base)}")
    for name, g in grids.items():
        info = rasterizer.build_ray_grid(verts, faces, g)
        label = f"{name} {g[0]}x{g[1]}x{g[2]}"
        print(f"  {label:<28}{'grid':<10}{med([t['grid'] for t in times[name]])}   ({info['n_pairs']} (cell, triangle) pairs, "
              f"{info['n_pairs'] / max(1, len(f)):.2f} per face)")
        print(f"  {label:<28}{'shadow':<10}{med([t['shadow'] for t in times[name]])}")
        print(f"  {label:<28}{'shade':<10}{med([t['shade'] for t in times[name]])}")
    # the first stage behind the raster stage's host synchronisation carries the launch gap: "shade" without shadows, "shadow" with them.
    # So the cost of the shadows is the difference of the sums, not a ratio of the shade stages.
    extra = [t["shadow"] + t["shade"] - b for t, b in zip(times["default"], base)]
    print(f"  default grid: shadow + shade with the mask, minus shade without (the stage behind the raster stage's host synchronisation "
          f"carries the launch gap in both): {med(extra)}")


gap, shares = S.measure()
print(f"float32 against float64 over every ray and triangle of every case of tests/render_shadow_cases.py, measured on the CPU: gap of the "
      f"pair terms {gap:.3e} (recorded RAY_GAP {S.RAY_GAP:.2e}), band RAY_BAND = 10 x = {S.RAY_BAND:.2e}; largest share of a case's samples "
      f"left out {max(shares.values()):.4f} ({max(shares, key=shares.get)})")
if not args.gaps_only:
    _lib.require_gpu()                               # no GPU: fail, there is nothing to measure
    run(71)
    run(368)
