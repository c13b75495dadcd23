#!/usr/bin/env python3
"""Per-stage times of the PBR renders (sin3dm_amd.rendering, s3d_render_pbr.hip) on one MI355X beside the flat
shader: the reference's eight views at 512 x 512, supersample 2, of the two bumpy tori of tools/bench_render.py (10 082 and
270 848 faces), drawn flat (k_render_shade, the path a call without the new arguments takes), smooth (vertex normals, the
three-light GGX model, the same 1024 x 1024 base colour image) and pbr (four 2048 x 2048 maps: albedo, metallic, roughness,
normal).  Stages are timed by device events recorded between them, summed over the eight views; vertex normals and face tangents
run once per call and are timed on their own.  Medians of the repeats after a warm-up, [min .. max].  In front: the float32 gaps
of tests/render_pbr_cases.py, measured on the CPU.

    python tools/bench_render_pbr.py [--repeats 7] > profiles/render_pbr.txt
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

import render_pbr_cases as P
from sin3dm_amd import _lib
from sin3dm_amd.rendering import rasterizer

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--resolution", type=int, nargs=2, default=(512, 512))
ap.add_argument("--supersample", type=int, default=2)
ap.add_argument("--gaps-only", action="store_true", help="the CPU part alone (no GPU needed)")
args = ap.parse_args()

STAGES = ("project", "bin count", "scan", "bin fill", "sort and segments", "raster", "shade")


def torus(n):
    """The bumpy torus of tools/bench_render.py on an n x n parameter grid: 2 n^2 faces, per-corner uv = the parameters."""
    a = np.arange(n) / n * 2 * np.pi
    u, v = np.meshgrid(a, a, indexing="ij")
    r = 0.35 + 0.05 * np.sin(5 * u) * np.cos(3 * v)
    p = np.stack([(1.0 + r * np.cos(v)) * np.cos(u), r * np.sin(v) + 0.1 * np.sin(2 * u), (1.0 + r * np.cos(v)) * np.sin(u)], 2).reshape(-1, 3)
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    i1, j1 = (i + 1) % n, (j + 1) % n
    q = lambda x, y: (x * n + y).reshape(-1)                                          # noqa: E731
    faces = np.concatenate([np.stack([q(i, j), q(i1, j), q(i1, j1)], 1), np.stack([q(i, j), q(i1, j1), q(i, j1)], 1)])
    fu = lambda x, y: np.stack([x.reshape(-1) / n, y.reshape(-1) / n], 1)             # noqa: E731
    uvs = np.concatenate([np.stack([fu(i, j), fu(i + 1, j), fu(i + 1, j + 1)], 1), np.stack([fu(i, j), fu(i + 1, j + 1), fu(i, j + 1)], 1)])
    return p.astype(np.float32), faces.astype(np.int32), uvs.astype(np.float32)


def maps(T):
    y, x = np.meshgrid(np.arange(T), np.arange(T), indexing="ij")
    albedo = np.stack([(x * 255 // T), (y * 255 // T), 255 * (((x // 32) + (y // 32)) % 2)], 2).astype(np.uint8)
    metallic = (255 * (((x // 128) + (y // 128)) % 2)).astype(np.uint8)
    roughness = ((x + y) * 255 // (2 * T)).astype(np.uint8)
    t = np.stack([0.4 * np.sin(x / 9.0), 0.4 * np.cos(y / 7.0), np.ones(x.shape)], 2)
    normal = np.round((t / np.linalg.norm(t, axis=2, keepdims=True) * 0.5 + 0.5) * 255).astype(np.uint8)
    return albedo, metallic, roughness, normal


def med(xs):
    return f"{statistics.median(xs):9.3f}  [{min(xs):.3f} .. {max(xs):.3f}]"


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def run(n):
    v, f, uv = torus(n)
    verts, faces, uvs = torch.from_numpy(v).cuda(), torch.from_numpy(f).cuda(), torch.from_numpy(uv).cuda()
    albedo, metallic, roughness, normal = (torch.from_numpy(m).cuda() for m in maps(2048))
    base = torch.from_numpy(maps(1024)[0]).cuda()
    W, H = args.resolution
    common = dict(uvs=uvs, resolution=(W, H), supersample=args.supersample)
    modes = {"flat": dict(materials=[{"Kd": (1.0, 1.0, 1.0), "image": base}]),
             "smooth": dict(materials=[{"Kd": (1.0, 1.0, 1.0), "image": base}], shading="smooth"),
             "pbr": dict(materials=[{"Kd": (1.0, 1.0, 1.0), "image": albedo, "metallic_image": metallic, "roughness_image": roughness,
                                     "normal_image": normal}], shading="pbr")}
    print(f"eight views of {W} x {H}, supersample {args.supersample}, of a torus of {len(f)} faces / {len(v)} vertices; median of {args.repeats} "
          f"runs after one warm-up [min .. max], ms for all eight views")
    shade = {}
    for name, kw in modes.items():
        rasterizer.render_views(verts, faces, **common, **kw)                         # warm-up
        per_stage = {s: [] for s in STAGES}
        for _ in range(args.repeats):
            marks = []

            def timer(stage):
                e = torch.cuda.Event(enable_timing=True)
                e.record()
                marks.append((stage, e))
            rasterizer.render_views(verts, faces, timer=timer, **common, **kw)
            torch.cuda.synchronize()
            acc = {s: 0.0 for s in STAGES}
            for (_, e0), (s, e1) in zip(marks[:-1], marks[1:]):
                if s != "start":
                    acc[s] += e0.elapsed_time(e1)
            for s in STAGES:
                per_stage[s].append(acc[s])
        shade[name] = statistics.median(per_stage["shade"])
        rest = [sum(per_stage[s][k] for s in STAGES if s != "shade") for k in range(args.repeats)]
        print(f"  {name:<8}{'shade':<22}{med(per_stage['shade'])}")
        print(f"  {name:<8}{'all other stages':<22}{med(rest)}")
    rasterizer.vertex_normals(verts, faces)
    rasterizer.face_tangents(verts, faces, uvs)
    vn = [timed(lambda: rasterizer.vertex_normals(verts, faces)) for _ in range(args.repeats)]
    ft = [timed(lambda: rasterizer.face_tangents(verts, faces, uvs)) for _ in range(args.repeats)]
    print(f"  {'once':<8}{'vertex normals':<22}{med(vn)}   (the sort and the segment starts included)")
    print(f"  {'once':<8}{'face tangents':<22}{med(ft)}")
    print(f"  shade stage, smooth / flat: {shade['smooth'] / shade['flat']:.2f}; pbr / flat: {shade['pbr'] / shade['flat']:.2f}")


ng, tg, ig, share = P.measure()
print(f"float32 against float64 over every case of tests/render_pbr_cases.py, measured on the CPU: normal gap {ng:.3e} (recorded "
      f"{P.NORMAL_GAP:.2e}, device bound {P.NORMAL_BOUND:.2e}), tangent gap {tg:.3e} (recorded {P.TANGENT_GAP:.2e}, device bound "
      f"{P.TANGENT_BOUND:.2e}); image gaps in uint8 levels {ig}, device bounds {P.IMAGE_BOUND}; largest flagged share of a view's covered "
      f"samples {share:.4f}")
if not args.gaps_only:
    _lib.require_gpu()                               # no GPU: fail, there is nothing to measure
    run(71)
    run(368)
