#!/usr/bin/env python3
"""Per-stage times of the mesh preprocessing (sin3dm_amd.data.mesh_sampler.prepare) on one MI355X — reso 256 and 2 M surface
samples (the command line's defaults) on a procedural mesh of 24 000 faces: a bumpy torus with two materials, one of them with a
1024 x 1024 image.  Every stage ends in a device synchronise, so host work inside it is included; median of the repeats after one
warm-up run.  Writing the .npz (np.savez_compressed, host only) is timed once, separately.

    python tools/bench_prepare.py [--reso 256 --n_surf 2000000 --nu 120 --nv 100 --repeats 3] > profiles/prepare.txt
"""
import argparse
import collections
import os
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from sin3dm_amd import _lib
from sin3dm_amd.data.mesh_sampler import MeshSampler, prepare

ap = argparse.ArgumentParser()
ap.add_argument("--reso", type=int, default=256)
ap.add_argument("--n_surf", type=int, default=2_000_000)
ap.add_argument("--nu", type=int, default=120)
ap.add_argument("--nv", type=int, default=100)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--no_save", action="store_true", help="skip timing np.savez_compressed")
args = ap.parse_args()

_lib.require_gpu()                                   # no GPU: fail, there is nothing to measure


def bumpy_torus(nu, nv):
    u, v = np.meshgrid(np.arange(nu) * 2 * np.pi / nu, np.arange(nv) * 2 * np.pi / nv, indexing="ij")
    r = 0.3 * (1 + 0.15 * np.sin(5 * u) * np.cos(3 * v))
    V = np.stack([(0.7 + r * np.cos(v)) * np.cos(u), 1.4 * r * np.sin(v), (0.7 + r * np.cos(v)) * np.sin(u)], -1).reshape(-1, 3)
    idx = np.arange(nu * nv).reshape(nu, nv)
    a, b, c, d = idx, np.roll(idx, -1, 0), np.roll(np.roll(idx, -1, 0), -1, 1), np.roll(idx, -1, 1)
    F = np.concatenate([np.stack([a, c, b], -1).reshape(-1, 3), np.stack([a, d, c], -1).reshape(-1, 3)])
    uv = np.stack([u / (2 * np.pi), v / (2 * np.pi)], -1).reshape(-1, 2)
    return V, F, uv[F]


V, F, uvs = bumpy_torus(args.nu, args.nv)
yy, xx = np.mgrid[0:1024, 0:1024]
image = np.stack([xx // 4, yy // 4, (xx ^ yy) & 255], -1).astype(np.uint8)
face_mat = (V[F].mean(1)[:, 1] < 0).astype(np.int32)
materials = [{"Kd": (1.0, 1.0, 1.0), "image": image}, {"Kd": (0.3, 0.6, 0.2)}]

stages = collections.OrderedDict()


def run():
    mesh = MeshSampler(verts=V, faces=F, uvs=uvs, face_mat=face_mat, materials=materials)
    cur, state = collections.OrderedDict(), {"name": None, "t": 0.0}

    def tick(name):
        torch.cuda.synchronize()
        now = time.perf_counter()
        if state["name"] is not None:
            cur[state["name"]] = cur.get(state["name"], 0.0) + (now - state["t"]) * 1e3
        state["name"], state["t"] = name, now
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = prepare(mesh, reso=args.reso, n_surf=args.n_surf, timer=tick)
    cur["TOTAL (wall clock, without writing the file)"] = (time.perf_counter() - t0) * 1e3
    return cur, out, mesh


run()                                                # warm-up: allocations, code objects
runs = [run() for _ in range(args.repeats)]
out, mesh = runs[-1][1], runs[-1][2]
n_pairs = mesh._binned(mesh.band)[5]
grid = out["sdf_grid"].shape
print(f"mesh preprocessing per stage, one MI355X: {len(F)} faces, reso {args.reso} (grid {grid[0]} x {grid[1]} x {grid[2]} = {out['sdf_grid'].size} points), "
      f"{args.n_surf} surface samples, band {out['threshold']:.6f}; median of {args.repeats} runs after one warm-up [min .. max], ms")
for label in runs[0][0]:
    vals = [r[0][label] for r in runs]
    print(f"  {label:<52s} {statistics.median(vals):9.2f}  [{min(vals):8.2f} .. {max(vals):8.2f}]")
inside = int((out["sdf_grid"] < 0).sum())
banded = int((np.abs(out["sdf_grid"]) < np.float32(out["threshold"])).sum())
wind = [r[0]["grid winding"] for r in runs]
print(f"  cell grid: {n_pairs} (cell, triangle) pairs = {n_pairs * 12 / 2 ** 20:.1f} MiB; grid points inside {inside}, within the band {banded}")
print(f"  grid winding: {out['sdf_grid'].size * len(F) / (statistics.median(wind) * 1e-3) / 1e9:.1f} G solid angles / s")
if not args.no_save:
    path = os.path.join(tempfile.mkdtemp(prefix="prepare_"), "shape.npz")
    t0 = time.perf_counter()
    np.savez_compressed(path, **out)
    print(f"  np.savez_compressed (host, once)                     {(time.perf_counter() - t0) * 1e3:9.2f}   ({os.path.getsize(path) / 2 ** 20:.1f} MiB)")
    os.remove(path)
