#!/usr/bin/env python3
"""The baked normal map of the textured export on one MI355X in one process: the skip net with texture at full
width (up 64, hidden 256), a 128^3 triplane, the iso-surface at 256^3 cut to 10 000 faces, a 2048^2 atlas.

  stages      isosurface.bake_normal_map taken apart, device-event times: the texel positions (s3d_tex_face_corner0 +
              s3d_tex_texel_positions), the compaction of the covered texels, the gradient (net.sdf_and_grad for K = 0,
              net.project_to_surface(iters=2) for K = 2), the face tangents, s3d_tex_normal_texels, s3d_tex_dilate_nearest
  whole       bake_normal_map for K = 0 and K = 2 next to bake_texture (the colour bake it runs beside), host time included
  status      the counts of the map's status values
  sphere      the numbers of tests/test_normal_bake_gpu.py::test_analytic_sphere

Synthetic weights and features (same arithmetic as trained ones).  The stages are interleaved round by round after a warm-up
round; medians and the spread (min .. max) are reported.  Expectation from profiles/sdf_grad.txt, not a gate: the covered texels
are about 0.7 of its N = 2^22 row, so about 45 ms per gradient evaluation, three of them for K = 2.

    python tools/bench_normal_bake.py [--repeats 7] > profiles/normal_bake.txt
"""
import argparse
import os
import statistics
import sys
import tempfile
import time
from types import SimpleNamespace

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]
import numpy as np
import torch

from sin3dm_amd import _lib, testing as T
from sin3dm_amd.encoding import isosurface as iso
from sin3dm_amd.encoding.model import ShapeAutoEncoder
from sin3dm_amd.rendering.rasterizer import face_tangents, vertex_normals

ap = argparse.ArgumentParser()
ap.add_argument("--fm", type=int, default=128, help="feature-map side (H = W = D)")
ap.add_argument("--reso", type=int, default=256)
ap.add_argument("--n_faces", type=int, default=10000)
ap.add_argument("--texreso", type=int, default=2048)
ap.add_argument("--repeats", type=int, default=7)
args = ap.parse_args()

_lib.require_gpu()                                   # no GPU: fail, there is nothing to measure
dev = torch.device("cuda:0")
lib = _lib.load()
AABB = torch.tensor([-1.0, -1, -1, 1, 1, 1])
cfg = SimpleNamespace(enc_net_type="skip", fdim_geo=4, fdim_tex=8, fdim_up=64, hidden_dim=256, n_hidden_layers=4, data_type="sdftex", gpu_id=0)
work = tempfile.mkdtemp(prefix="normal_bake_")
ae = ShapeAutoEncoder(work, cfg, device=dev)
ae.net.load_state_dict(T.synthetic_state_dict(T.ae_param_shapes(), 5), strict=False)
ae.net.to(dev).eval()
ae.aabb = AABB.to(dev)
ae.net.reset_aabb(ae.aabb)
ae.featmap_size = (args.fm,) * 3
fm = [torch.from_numpy(np.tanh(T.synthetic_noise((1, 12, args.fm, args.fm), s))).to(dev) for s in (1, 2, 3)]
mesh = ae.decode_texmesh(work, fm, args.reso, n_faces=args.n_faces, texture_reso=args.texreso, save_voxel=False)
verts, tris = mesh["verts"], mesh["tris"].contiguous().to(torch.int32)
aabb = ae._resize_aabb((args.fm,) * 3)
TR, F = args.texreso, tris.shape[0]
CELL = float(aabb[3:].max() - aabb[:3].min()) / args.reso
base = vertex_normals(verts, tris)


def grad_k0(p):
    return ae.net.sdf_and_grad(p, fm, aabb=aabb)[1]


def grad_k2(p):
    return ae.net.project_to_surface(p, fm, aabb=aabb, iters=2, max_step=CELL, max_move=CELL)[2]


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def report(times, width=34):
    for k, v in times.items():
        print(f"  {k:{width}s} {statistics.median(v):9.3f}  ({min(v):.3f} .. {max(v):.3f})")


print(f"skip net with texture, up 64 / hidden 256, {args.fm}^3 triplane, iso-surface at {args.reso}^3 cut to {F} faces ({verts.shape[0]} vertices), "
      f"{TR}^2 atlas; {args.repeats} rounds after one warm-up, medians (min .. max) in ms")

# ---------------------------------------------------------------- the stages of bake_normal_map, device events
state = {}


def st_texels():
    state["face_id"], state["pos"], state["corner0"], state["atlas"] = iso.atlas_texels(verts, tris, TR)


def st_compact():
    state["idx"] = torch.nonzero(state["face_id"] >= 0).squeeze(1)
    state["pts"] = state["pos"][state["idx"]]


def st_tangents():
    uvs = torch.from_numpy(state["atlas"].uvs(state["corner0"].cpu().numpy())).to(dev)
    state["tangents"] = face_tangents(verts, tris, uvs)


def st_texel_kernel(key):
    a, idx = state["atlas"], state["idx"]
    raw = torch.empty((TR, TR, 3), device=dev, dtype=torch.uint8)
    status = torch.empty((TR, TR), device=dev, dtype=torch.uint8)
    _lib.check(lib.s3d_tex_normal_texels(_lib.ptr(state[key]), _lib.ptr(idx), idx.shape[0], _lib.ptr(verts), verts.shape[0], _lib.ptr(tris),
                                         _lib.ptr(state["corner0"]), F, TR, a.n, a.c, _lib.ptr(base), _lib.ptr(state["tangents"]), _lib.ptr(raw),
                                         _lib.ptr(status), _lib.stream_ptr()))
    state["raw"], state["status_" + key] = raw, status


def st_dilate():
    out = torch.empty_like(state["raw"])
    _lib.check(lib.s3d_tex_dilate_nearest(_lib.ptr(state["raw"]), _lib.ptr(state["face_id"]), TR, 3, _lib.ptr(out), _lib.stream_ptr()))
    state["image"] = out


stages = {
    "texel positions (atlas_texels)": st_texels,
    "compaction of covered texels": st_compact,
    "gradient, K = 0 (sdf_and_grad)": lambda: state.__setitem__("g0", grad_k0(state["pts"])),
    "gradient, K = 2 (project, 3 evals)": lambda: state.__setitem__("g2", grad_k2(state["pts"])),
    "face tangents (uvs via the host)": st_tangents,
    "s3d_tex_normal_texels": lambda: st_texel_kernel("g0"),
    "s3d_tex_dilate_nearest": st_dilate,
}
times = {k: [] for k in stages}
for rep in range(args.repeats + 1):
    for label, fn in stages.items():
        ms, _ = timed(fn)
        if rep:
            times[label].append(ms)
n_cov = int(state["idx"].shape[0])
print(f"\nstages of bake_normal_map, {n_cov} covered texels ({n_cov / 2 ** 22:.2f} of 2^22; atlas cells of {state['atlas'].c} texels)")
report(times)
med = {k: statistics.median(v) for k, v in times.items()}
print(f"  the two kernels together {med['s3d_tex_normal_texels'] + med['s3d_tex_dilate_nearest']:.3f} ms against {med['gradient, K = 0 (sdf_and_grad)']:.3f} ms "
      f"for one gradient evaluation; K = 2 / K = 0 = {med['gradient, K = 2 (project, 3 evals)'] / med['gradient, K = 0 (sdf_and_grad)']:.2f} (expected 3)")

# ---------------------------------------------------------------- whole calls next to the colour bake, host time included
runs = {
    "bake_texture": lambda: iso.bake_texture(verts, tris, TR, lambda p: ae.decode_batch(fm, p, aabb=aabb)[..., 1:]),
    "bake_normal_map, K = 0": lambda: iso.bake_normal_map(verts, tris, TR, grad_k0, base_normals=base),
    "bake_normal_map, K = 2": lambda: iso.bake_normal_map(verts, tris, TR, grad_k2, base_normals=base),
}
times = {k: [] for k in runs}
reps = min(args.repeats, 5)
for rep in range(reps + 1):
    for label, fn in runs.items():
        ms, out = wall(fn)
        if rep:
            times[label].append(ms)
        if label.endswith("K = 0"):
            st0 = out[1]
        elif label.endswith("K = 2"):
            st2 = out[1]
print(f"\nwhole calls, wall clock with the device drained, {reps} rounds after one warm-up")
report(times)

print("\nstatus counts (0 uncovered, 1 encoded, 2 no gradient direction, 3 no frame, 4 encoded around the face normal)")
for label, st in (("K = 0", st0), ("K = 2", st2)):
    print(f"  {label}: " + "  ".join(f"{k}: {int((st == k).sum())}" for k in range(5)))

# ---------------------------------------------------------------- the analytic sphere of the GPU test
from test_normal_bake_gpu import sphere_errors  # noqa: E402
with_map, without, n = sphere_errors()
print(f"\nanalytic sphere (32 faces against 8 192, `normal` pass at 96^2, 8 views, {n} pixels covered in all three renders)")
print(f"  mean angular error with the baked map {with_map:.3f} degrees, with the flat normals alone {without:.3f} degrees, ratio {without / with_map:.2f}")
