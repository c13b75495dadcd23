#!/usr/bin/env python3
"""Per-stage times of the mesh preprocessing (sin3dm_amd.data.mesh_sampler.prepare) on one MI355X — reso 256 and 2 M surface
samples (the command line's defaults) on a procedural mesh of 24 000 faces: a bumpy torus with two materials, one of them with a
1024 x 1024 image.  Every stage ends in a device synchronise, so host work inside it is included; median of the repeats after one
warm-up run.  Writing the .npz (np.savez_compressed, host only) is timed once, separately.

    python tools/bench_prepare.py [--reso 256 --n_surf 2000000 --nu 120 --nv 100 --repeats 3] > profiles/prepare.txt
    python tools/bench_prepare.py --pbr > profiles/prepare_pbr.txt         # prepare against mesh_sampler_pbr.prepare_pbr, interleaved
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
ap.add_argument("--pbr", action="store_true", help="the eight-channel prepare_pbr (four maps of different sizes) against the three-channel prepare, "
                                                   "interleaved in one process, per stage and per texture launch by device events")
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
TEXTURE_CALLS = ("grid", "on-surface", "near-surface")          # the three texture calls of prepare, in order


def pbr_materials():
    """The two materials with four procedural maps of different sizes on the first: albedo 1024 x 1024 (the image above), metallic
    512 x 512, roughness 256 x 512, normal 2048 x 1024."""
    def plane(w, h, k):
        y, x = np.mgrid[0:h, 0:w]
        return ((x * k + y * (k + 2)) & 255).astype(np.uint8)
    normal = np.stack([plane(2048, 1024, 1), plane(2048, 1024, 3), np.full((1024, 2048), 255, np.uint8)], -1)
    return [dict(materials[0], metallic_image=plane(512, 512, 5), roughness_image=plane(256, 512, 7), normal_image=normal, Pm=0.0, Pr=1.0),
            dict(materials[1], Pm=0.2, Pr=0.6)]


def run_timed(pbr):
    """One prepare (three channels) or prepare_pbr (eight): ({stage: ms} by device events recorded at every stage start, {texture
    call: ms} by events around the three texture launches, the saved dictionary)."""
    from sin3dm_amd.data.mesh_sampler_pbr import MeshSamplerPBR, prepare_pbr
    if pbr:
        mesh = MeshSamplerPBR(verts=V, faces=F, uvs=uvs, face_mat=face_mat, materials=pbr_materials())
    else:
        mesh = MeshSampler(verts=V, faces=F, uvs=uvs, face_mat=face_mat, materials=materials)
    marks, calls = [], []
    inner = mesh.materials8 if pbr else mesh.colors

    def texture(face, bary):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = inner(face, bary)
        b.record()
        calls.append((a, b, int(face.shape[0]), face))
        return out
    setattr(mesh, "materials8" if pbr else "colors", texture)    # (prepare looks the method up on the instance)

    def tick(name):
        ev = torch.cuda.Event(enable_timing=True)
        ev.record()
        marks.append((name, ev))
    out = (prepare_pbr if pbr else prepare)(mesh, reso=args.reso, n_surf=args.n_surf, timer=tick)
    torch.cuda.synchronize()
    cur = collections.OrderedDict()
    for (name, ev), (_, nxt) in zip(marks[:-1], marks[1:]):
        cur[name] = cur.get(name, 0.0) + ev.elapsed_time(nxt)
    cur["TOTAL (without writing the file)"] = marks[0][1].elapsed_time(marks[-1][1])
    tex =collections.OrderedDict((label, a.elapsed_time(b)) for label, (a, b, _, _) in zip(TEXTURE_CALLS, calls))
    hits = collections.OrderedDict((label, (n, int((face >= 0).sum()))) for label, (_, _, n, face) in zip(TEXTURE_CALLS, calls))
    return cur, tex, hits, out


def run_pbr():
    """The three-channel and the eight-channel prepare interleaved in one process."""
    run_timed(False), run_timed(True)                    # warm-up: allocations, code objects
    runs = {False: [], True: []}
    for _ in range(args.repeats):
        for pbr in (False, True):
            runs[pbr].append(run_timed(pbr))
    out = runs[True][-1][3]
    grid = out["sdf_grid"].shape
    assert out["tex_grid"].shape[-1] == 8 and runs[False][-1][3]["tex_grid"].shape[-1] == 3
    assert all(np.array_equal(out[k], runs[False][-1][3][k]) for k in ("sdf_grid", "pts_on_surf", "sdf_near_surf"))
    print(f"mesh preprocessing, three channels (prepare) against eight (prepare_pbr), one MI355X: {len(F)} faces, reso {args.reso} (grid "
          f"{grid[0]} x {grid[1]} x {grid[2]} = {out['sdf_grid'].size} points), {args.n_surf} surface samples; the two interleaved in one process, "
          f"median of {args.repeats} runs each after one warm-up [min .. max], ms by device events")

    def row(label, a, b):
        print(f"  {label:<34s} {statistics.median(a):9.3f} [{min(a):9.3f} .. {max(a):9.3f}]   {statistics.median(b):9.3f} [{min(b):9.3f} .. {max(b):9.3f}]"
              f"   x {statistics.median(b) / max(statistics.median(a), 1e-9):.2f}")
    print(f"  {'stage (with its host work and copies)':<34s} {'3 channels':^33s}   {'8 channels':^33s}")
    for label in runs[False][0][0]:
        row(label, [r[0][label] for r in runs[False]], [r[0][label] for r in runs[True]])
    # nominal traffic of a query: face 4 B; on a hit bary 12, the face's uv 24, its material 4, the texels (3 | 3 + 1 + 1 + 3) and, per
    # material, the table row; the row written (12 | 32)
    miss, hit = (4 + 12, 4 + 32), (4 + 12 + 24 + 4 + 3 + 12, 4 + 12 + 24 + 4 + 8 + 32)
    print(f"  {'texture launch alone':<34s} {'3 channels':^33s}   {'8 channels':^33s}        bytes moved, 8 : 3")
    for label in TEXTURE_CALLS:
        n, h = runs[True][-1][2][label]
        b3, b8 = (n - h) * miss[0] + h * hit[0], (n - h) * miss[1] + h * hit[1]
        row(f"{label} ({n} queries)", [r[1][label] for r in runs[False]], [r[1][label] for r in runs[True]])
        print(f"      {h} hits at {hit[0]} | {hit[1]} B, {n - h} misses at {miss[0]} | {miss[1]} B: {b3 / 2 ** 20:.1f} | {b8 / 2 ** 20:.1f} MiB, ratio {b8 / b3:.2f}; "
              f"{b3 / statistics.median([r[1][label] for r in runs[False]]) / 1e6:.0f} | {b8 / statistics.median([r[1][label] for r in runs[True]]) / 1e6:.0f} GB/s")


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


if args.pbr:
    run_pbr()
    sys.exit(0)
run()                                                # warm-up: allocations, code objects
runs =[run() for _ in range(args.repeats)]
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
