#!/usr/bin/env python3
"""Per-stage times of ShapeAutoEncoder.decode_texmesh on one MI355X — reso 256, n_faces 10000, texreso 2048 (the reference's
defaults, src/utils/parser_util.py) — next to decode_mesh (the vertex-coloured export, unchanged) on the same triplane.
Synthetic weights and features as tools/bench_end_to_end.py builds them (same arithmetic as trained ones; the surface they
decode to is whatever it is: its size is printed).  Every stage is timed with device events around the call (a stage ends in a
synchronise, so host work inside it is included), after a warm-up run, and reported as the median of the repeats.

    python tools/bench_texmesh.py [--reso 256 --n_faces 10000 --texreso 2048 --repeats 7 --fm 128] > profiles/texmesh.txt
"""
import argparse
import collections
import os
import statistics
import sys
import tempfile
import time
from types import SimpleNamespace

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from sin3dm_amd import _lib, testing as T
from sin3dm_amd.encoding import isosurface as iso
from sin3dm_amd.encoding.model import ShapeAutoEncoder

ap = argparse.ArgumentParser()
ap.add_argument("--reso", type=int, default=256)
ap.add_argument("--n_faces", type=int, default=10000)
ap.add_argument("--texreso", type=int, default=2048)
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--fm", type=int, default=128, help="feature-map side (H = W = D)")
args = ap.parse_args()

_lib.require_gpu()                                   # no GPU: fail, there is nothing to measure
dev = torch.device("cuda:0")
cfg = SimpleNamespace(enc_net_type="skip", fdim_geo=4, fdim_tex=8, fdim_up=64, hidden_dim=256, n_hidden_layers=4, data_type="sdftex", gpu_id=0)
work = tempfile.mkdtemp(prefix="texmesh_")
ae = ShapeAutoEncoder(work, cfg, device=dev)
ae.net.load_state_dict(T.synthetic_state_dict(T.ae_param_shapes(), 5), strict=False)
ae.net.to(dev).eval()
ae.aabb = torch.tensor([-1.0, -1, -1, 1, 1, 1], device=dev)
ae.net.reset_aabb(ae.aabb)
ae.featmap_size = (args.fm,) * 3
fm = [torch.from_numpy(np.tanh(T.synthetic_noise((1, 12, args.fm, args.fm), s))).to(dev) for s in (1, 2, 3)]

cur = collections.defaultdict(float)
sizes = {}


def timed(label, fn):
    def wrapper(*a, **k):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        out = fn(*a, **k)
        e1.record()
        e1.synchronize()
        cur[label] += e0.elapsed_time(e1)
        return out
    return wrapper


def sized(label, fn):
    def wrapper(*a, **k):
        out = fn(*a, **k)
        sizes[label] = (int(out[0].shape[0]), int(out[1].shape[0]))
        return out
    return wrapper


# decode_texmesh looks its stages up in these objects when it runs, so wrapping the attributes times the real pipeline
ae.decode_grid = timed("decode_grid", ae.decode_grid)
ae.decode_batch = timed("  of which decode_batch over the covered texels", ae.decode_batch)
iso.marching_cubes = timed("marching_cubes", sized("iso-surface", iso.marching_cubes))
iso.largest_component = timed("largest_component", sized("largest component", iso.largest_component))
iso.simplify_mesh = timed("simplify_mesh", sized("decimated", iso.simplify_mesh))
iso.simplify_mesh_quadric = timed("simplify_mesh_quadric (decimation=\"quadric\")", sized("decimated (quadric)", iso.simplify_mesh_quadric))
iso.atlas_texels = timed("  of which corner0 + texel positions", iso.atlas_texels)
iso.bake_texture = timed("bake_texture", iso.bake_texture)
iso.export_textured_obj = timed("export_textured_obj (host: OBJ + MTL + PNG)", iso.export_textured_obj)
iso.export_obj = timed("export_obj (host: vertex-coloured OBJ)", iso.export_obj)


ORDER = ["decode_grid", "marching_cubes", "largest_component", "simplify_mesh", "simplify_mesh_quadric (decimation=\"quadric\")", "bake_texture", "  of which corner0 + texel positions",
         "  of which decode_batch over the covered texels", "export_textured_obj (host: OBJ + MTL + PNG)",
         "export_obj (host: vertex-coloured OBJ)", "TOTAL (wall clock)"]


def run(which):
    cur.clear()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if which in ("texmesh", "texmesh_quadric"):
        kw = {"decimation": "quadric"} if which == "texmesh_quadric" else {}
        out = ae.decode_texmesh(work, fm, args.reso, n_faces=args.n_faces, texture_reso=args.texreso, save_voxel=False, **kw)
        if out is None:
            raise SystemExit("the synthetic decoder gave an empty iso-surface: nothing to measure")
        sizes["covered texels"] = int(out["mask"].sum())
        if which == "texmesh":
            sizes["R"] = out["info"]["R"]
        else:
            sizes["rounds"], sizes["stuck"] = out["info"]["rounds"], out["info"]["stuck"]
    else:
        ae.decode_mesh(work, fm, args.reso, save_voxel=False)
    torch.cuda.synchronize()
    res = dict(cur)
    res["TOTAL (wall clock)"] = (time.perf_counter() - t0) * 1e3
    return res


print(f"decode_texmesh per stage, one MI355X: reso {args.reso}, n_faces {args.n_faces}, texreso {args.texreso}, feature maps {args.fm}^3, "
      f"synthetic weights; median of {args.repeats} runs after one warm-up [min .. max], ms")
TITLES = {"texmesh": "decode_texmesh (textured OBJ, save_voxel=False)",
          "texmesh_quadric": "decode_texmesh(decimation=\"quadric\") (textured OBJ, save_voxel=False)",
          "mesh": "decode_mesh (vertex-coloured OBJ, save_voxel=False; unchanged by this export)"}
for which in ("texmesh", "texmesh_quadric", "mesh"):
    run(which)                                      # warm-up: allocations, code objects, first-call packing
    runs = [run(which) for _ in range(args.repeats)]
    print(f"\n{TITLES[which]}")
    for label in sorted(runs[0], key=lambda l: ORDER.index(l) if l in ORDER else len(ORDER)):
        vals = [r[label] for r in runs]
        print(f"  {label:<52s} {statistics.median(vals):9.2f}  [{min(vals):8.2f} .. {max(vals):8.2f}]")
    if which == "texmesh_quadric":
        print(f"  mesh: decimated ({sizes['rounds']} rounds, stuck {sizes['stuck']}) {sizes['decimated (quadric)'][0]} / {sizes['decimated (quadric)'][1]}, "
              f"{sizes['covered texels']} covered texels")
    if which == "texmesh":
        at = iso.triangle_atlas(sizes["decimated"][1], args.texreso)
        print(f"  mesh: iso-surface {sizes['iso-surface'][0]} vertices / {sizes['iso-surface'][1]} faces, largest component "
              f"{sizes['largest component'][0]} / {sizes['largest component'][1]}, decimated (R = {sizes['R']}) {sizes['decimated'][0]} / {sizes['decimated'][1]}")
        print(f"  atlas: {at.n} x {at.n} cells of {at.c} texels, L = {at.L}, utilisation L^2/c^2 = {at.utilisation:.3f}, "
              f"{sizes['covered texels']} covered texels of {args.texreso ** 2}")
