"""Mesh -> the .npz `sin3dm_amd.train --data_path` reads, on one MI355X (the reference's data/mesh_sampler.py, which needs
trimesh and point_cloud_utils; an own design, DESIGN.md §16 — parity with those libraries is not claimed).

    python -m sin3dm_amd.data.mesh_sampler -s SRC.obj -d DST.npz [--reso 256 --n_surf 2000000 --mult 8 --threshold T
                                                                   --enlarge_scale 1.03 --only_vol --seed 0]

The distance is exact inside the band |sdf| < threshold and +-threshold outside, which is all the clipped target needs; the sign
comes from the generalized winding number of the mesh as it is (inside iff |wn| >= 0.5), so no watertight copy is built and an
inward-oriented mesh gives the same result.  There is no CPU fallback.
"""
import argparse
import ctypes as C
import math
import os
import sys

import numpy as np

from .. import _lib
from . import obj_io
from .utils import normalize_aabb, sample_grid_points_aabb

MAX_CELLS_PER_AXIS = 256        # the host's choice of cell grid: cell edge = max(band, longest extent / 256)
NEAR_SURF_SIGMA = 0.005         # reference :197
KEYS_VOL = ("pts_grid", "sdf_grid", "tex_grid", "aabb", "threshold", "Ka", "Kd", "Ks", "Ns")
KEYS_ALL = KEYS_VOL + ("pts_on_surf", "tex_on_surf", "pts_near_surf", "sdf_near_surf", "tex_near_surf")


def cell_grid(vmin, vmax, band):
    """(origin float32 [3], cell, dims) of the uniform grid that covers the mesh's box dilated by the band (and a margin)."""
    vmin, vmax = np.asarray(vmin, dtype=np.float64), np.asarray(vmax, dtype=np.float64)
    pad = band * 1.01 + 1e-5
    lo, hi = vmin - pad, vmax + pad
    cell = max(float(band), float((hi - lo).max()) / MAX_CELLS_PER_AXIS)
    dims = [int(max(1, math.ceil((hi[k] - lo[k]) / cell))) for k in range(3)]
    return lo.astype(np.float32), float(np.float32(cell)), dims


class MeshSampler:
    """A triangle mesh with per-corner uv and per-face materials, queried on the device.

    MeshSampler(path) reads an OBJ (+ MTL, images); MeshSampler(verts=, faces=, uvs=, face_mat=, materials=) takes arrays:
    verts [V, 3], faces [F, 3], uvs [F, 3, 2] or None, face_mat [F] or None, materials: list of dicts with Kd (and Ka, Ks, Ns,
    image uint8 [H, W, 3] or None).  band: the default band of query_sdf / query_tex / closest."""

    def __init__(self, path=None, *, verts=None, faces=None, uvs=None, face_mat=None, materials=None, band=None):
        if path is not None:
            mesh = obj_io.load_obj(path)
            verts, faces, uvs, face_mat = mesh["verts"], mesh["faces"], mesh["uvs"], mesh["face_mat"]
            materials = [m for _, m in mesh["materials"]]
            self.n_degenerate = mesh["n_degenerate"]
        self.path = path
        self.vs = np.asarray(verts, dtype=np.float64).reshape(-1, 3)
        self.fs = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
        if self.fs.shape[0] == 0:
            raise ValueError("MeshSampler: the mesh has no faces")
        if self.fs.min() < 0 or self.fs.max() >= self.vs.shape[0]:
            raise ValueError(f"MeshSampler: face indices outside [0, {self.vs.shape[0]})")
        F = self.fs.shape[0]
        self.uvs = np.zeros((F, 3, 2)) if uvs is None else np.asarray(uvs, dtype=np.float64).reshape(F, 3, 2)
        self.face_mat = np.zeros(F, dtype=np.int32) if face_mat is None else np.asarray(face_mat, dtype=np.int32).reshape(F)
        self.materials = [dict(obj_io.DEFAULT_MATERIAL, **m) for m in (materials or [{}])]
        if self.face_mat.min() < 0 or self.face_mat.max() >= len(self.materials):
            raise ValueError(f"MeshSampler: material ids outside [0, {len(self.materials)})")
        self.Kas = np.array([m["Ka"] for m in self.materials], dtype=np.float64)
        self.Kds = np.array([m["Kd"] for m in self.materials], dtype=np.float64)
        self.Kss = np.array([m["Ks"] for m in self.materials], dtype=np.float64)
        self.Nss = np.array([m["Ns"] for m in self.materials], dtype=np.float64)
        self.aabb = None
        self.band = band                                   # default band of the queries (the CLI: --threshold)
        self._dev = None                                   # device images of the mesh: built at the first query
        self._bins = {}                                    # band -> cell grid and segments

    # ------------------------------------------------------------------ host
    def normalize(self, reso=256, enlarge_scale=1.03, mult=8):
        self.aabb, translation, scale = normalize_aabb(self.vs, reso=reso, enlarge_scale=enlarge_scale, mult=mult)
        self.vs = (self.vs + translation) * scale
        self._dev, self._bins = None, {}

    # ------------------------------------------------------------------ device images
    def _device(self):
        import torch
        _lib.require_gpu()
        if self._dev is None:
            dev = torch.device("cuda")
            d = {"tri9": torch.from_numpy(self.vs[self.fs].reshape(-1, 9).astype(np.float32)).to(dev).contiguous(),
                 "uv": torch.from_numpy(self.uvs.reshape(-1, 6).astype(np.float32)).to(dev).contiguous(),
                 "face_mat": torch.from_numpy(self.face_mat).to(dev).contiguous()}
            table, blobs, off = [], [], 0
            for m in self.materials:
                img = m.get("image")
                if img is None:
                    table.append([0, 0, 0])
                    continue
                img = np.ascontiguousarray(np.asarray(img, dtype=np.uint8)[..., :3])
                table.append([off, img.shape[1], img.shape[0]])
                blobs.append(img.reshape(-1))
                off += img.size
            packed = np.concatenate(blobs) if blobs else np.zeros(1, dtype=np.uint8)
            d["mat"] = torch.tensor(table, dtype=torch.int64, device=dev).contiguous()
            d["kd"] = torch.from_numpy(self.Kds.astype(np.float32)).to(dev).contiguous()
            d["img"] = torch.from_numpy(packed).to(dev)
            d["img_bytes"] = off
            self._dev = d
        return self._dev

    def _points(self, points):
        import torch
        d = self._device()
        if not torch.is_tensor(points):
            points = torch.from_numpy(np.ascontiguousarray(np.asarray(points, dtype=np.float32)))
        return points.to(d["tri9"].device, torch.float32).reshape(-1, 3).contiguous()

    def _binned(self, band):
        """(origin, cell, dims, seg, seg_tri, n_pairs) for a band: count, scan, fill, stable sort by cell, segment starts."""
        import torch
        if band is None:
            band = self.band
        if band is None or not band > 0:
            raise ValueError(f"MeshSampler: band {band!r}: pass band= or set .band to the clipping threshold (> 0)")
        band = float(np.float32(band))
        if band in self._bins:
            return self._bins[band]
        d, lib = self._device(), _lib.load()
        tri9 = d["tri9"]
        F = tri9.shape[0]
        origin, cell, dims = cell_grid(self.vs.min(0), self.vs.max(0), band)
        o3, d3 = (C.c_float * 3)(*[float(x) for x in origin]), (C.c_int * 3)(*dims)
        counts = torch.empty(F, device=tri9.device, dtype=torch.int64)
        _lib.check(lib.s3d_meshsdf_bin_count(_lib.ptr(tri9), F, band, o3, cell, d3, _lib.ptr(counts), _lib.stream_ptr()))
        ends = torch.cumsum(counts, 0)
        n_pairs = int(ends[-1])
        if n_pairs > _lib.MESHSDF_MAX_PAIRS:
            raise NotImplementedError(f"MeshSampler: band {band:g} puts {n_pairs} (cell, triangle) pairs on a {dims[0]} x {dims[1]} x {dims[2]} grid: "
                                      f"{n_pairs * 12 / 2 ** 30:.2f} GiB of workspace, over the cap of {_lib.MESHSDF_MAX_PAIRS} pairs = 1.5 GiB")
        offsets = (ends - counts).contiguous()
        pair_cell = torch.empty(max(n_pairs, 1), device=tri9.device, dtype=torch.int64)
        pair_tri = torch.empty(max(n_pairs, 1), device=tri9.device, dtype=torch.int32)
        _lib.check(lib.s3d_meshsdf_bin_fill(_lib.ptr(tri9), F, band, o3, cell, d3, _lib.ptr(offsets), n_pairs, _lib.ptr(pair_cell),
                                            _lib.ptr(pair_tri), _lib.stream_ptr()))
        pair_cell, order = torch.sort(pair_cell[:n_pairs], stable=True)
        seg_tri = pair_tri[:n_pairs][order].contiguous()
        n_cells = dims[0] * dims[1] * dims[2]
        seg = torch.searchsorted(pair_cell, torch.arange(n_cells + 1, device=tri9.device, dtype=torch.int64)).contiguous()
        self._bins[band] = (o3, cell, d3, seg, seg_tri, n_pairs, band)
        return self._bins[band]

    # ------------------------------------------------------------------ queries
    def closest(self, points, band=None):
        """(dist [N], face [N] int32, bary [N, 3]) on the device: the closest surface point within `band`, else (band, -1, 0)."""
        import torch
        pts = self._points(points)
        o3, cell, d3, seg, seg_tri, n_pairs, band = self._binned(band)
        d, N = self._device(), pts.shape[0]
        dist = torch.empty(N, device=pts.device, dtype=torch.float32)
        face = torch.empty(N, device=pts.device, dtype=torch.int32)
        bary = torch.empty((N, 3), device=pts.device, dtype=torch.float32)
        _lib.check(_lib.load().s3d_meshsdf_closest(_lib.ptr(pts), N, _lib.ptr(d["tri9"]), d["tri9"].shape[0], band, o3, cell, d3, _lib.ptr(seg),
                                                   _lib.ptr(seg_tri), n_pairs, _lib.ptr(dist), _lib.ptr(face), _lib.ptr(bary), _lib.stream_ptr()))
        return dist, face, bary

    def winding_number(self, points):
        import torch
        pts = self._points(points)
        d = self._device()
        wn = torch.empty(pts.shape[0], device=pts.device, dtype=torch.float32)
        _lib.check(_lib.load().s3d_meshsdf_winding(_lib.ptr(pts), pts.shape[0], _lib.ptr(d["tri9"]), d["tri9"].shape[0], _lib.ptr(wn),
                                                   _lib.stream_ptr()))
        return wn

    def query_sdf(self, points, band=None, with_closest=False):
        """Signed distance clipped to +-band (negative inside: |winding number| >= 0.5), float32 [N] on the device."""
        import torch
        pts = self._points(points)
        dist, face, bary = self.closest(pts, band)
        sdf = torch.where(self.winding_number(pts).abs() >= 0.5, -dist, dist)
        return (sdf, face, bary) if with_closest else sdf

    def colors(self, face, bary):
        """Colour float32 [N, 3] of (face, barycentrics) pairs; face -1 gives 0."""
        import torch
        d = self._device()
        face, bary = face.contiguous(), bary.contiguous()
        out = torch.empty((face.shape[0], 3), device=face.device, dtype=torch.float32)
        _lib.check(_lib.load().s3d_meshsdf_texture(_lib.ptr(face), _lib.ptr(bary), face.shape[0], _lib.ptr(d["uv"]), _lib.ptr(d["face_mat"]),
                                                   d["uv"].shape[0], _lib.ptr(d["mat"]), _lib.ptr(d["kd"]), len(self.materials), _lib.ptr(d["img"]),
                                                   d["img_bytes"], _lib.ptr(out), _lib.stream_ptr()))
        return out

    def query_tex(self, points, band=None):
        """Colour of the closest surface point where it lies within `band`, 0 elsewhere: float32 [N, 3] on the device."""
        _, face, bary = self.closest(points, band)
        return self.colors(face, bary)

    def sample_surf(self, n, generator=None):
        """n area-weighted surface points: (points [n, 3], face [n] int32, bary [n, 3]) on the device.  generator: a torch.Generator
        (of either device) that the three uniforms per sample are drawn from; the same state gives the same samples."""
        import torch
        d, lib = self._device(), _lib.load()
        tri9 = d["tri9"]
        F, dev = tri9.shape[0], tri9.device
        areas = torch.empty(F, device=dev, dtype=torch.float32)
        _lib.check(lib.s3d_meshsdf_face_areas(_lib.ptr(tri9), F, _lib.ptr(areas), _lib.stream_ptr()))
        cdf = torch.cumsum(areas.double(), 0).contiguous()
        gdev = generator.device if generator is not None else dev
        u = torch.rand((int(n), 3), generator=generator, device=gdev, dtype=torch.float32).to(dev).contiguous()
        pts = torch.empty((int(n), 3), device=dev, dtype=torch.float32)
        face = torch.empty(int(n), device=dev, dtype=torch.int32)
        bary = torch.empty((int(n), 3), device=dev, dtype=torch.float32)
        _lib.check(lib.s3d_meshsdf_sample_surface(_lib.ptr(tri9), F, _lib.ptr(cdf), _lib.ptr(u), int(n), _lib.ptr(pts), _lib.ptr(face),
                                                  _lib.ptr(bary), _lib.stream_ptr()))
        return pts, face, bary


def build_parser(prog="python -m sin3dm_amd.data.mesh_sampler",
                 description="OBJ/MTL -> the .npz that sin3dm_amd.train --data_path reads, on one MI355X"):
    p = argparse.ArgumentParser(prog=prog, description=description)
    p.add_argument("-s", "--src", type=str, required=True)
    p.add_argument("-d", "--dst", type=str, required=True)
    p.add_argument("--reso", type=int, default=256)
    p.add_argument("--watertight_reso", type=int, default=100_000,
                   help="accepted for compatibility with the reference's command line; does nothing (no watertight copy is built: the "
                        "sign comes from the generalized winding number)")
    p.add_argument("--n_surf", type=int, default=2_000_000)
    p.add_argument("--mult", type=int, default=8)
    p.add_argument("--threshold", type=float, default=None, help="band of the clipped distance; default 2 / reso * 3")
    p.add_argument("--enlarge_scale", type=float, default=1.03)
    p.add_argument("-wt", "--watertight", action="store_true", help="accepted for compatibility with the reference's command line; does nothing")
    p.add_argument("--only_vol", action="store_true", help="write the grid keys only")
    p.add_argument("--seed", type=int, default=0, help="seed of the surface and near-surface samples")
    return p


def parse_args(argv=None, parser=None):
    args = (parser or build_parser()).parse_args(argv)
    if args.threshold is None:
        args.threshold = 2. / args.reso * 3
    return args


def prepare_stages(mesh, texture, extra, reso=256, n_surf=2_000_000, mult=8, threshold=None, enlarge_scale=1.03, only_vol=False, seed=0,
                   timer=None):
    """The stages of prepare and of mesh_sampler_pbr.prepare_pbr.  texture(face, bary) -> float32 [n, C] on the device, 0 where
    face is -1 (|sdf| = threshold); extra(mesh) -> the keys saved beside the grid keys."""
    import torch
    _lib.require_gpu()
    tick = timer or (lambda name: None)
    thr = 2. / reso * 3 if threshold is None else float(threshold)
    mesh.band = thr
    tick("normalize")
    mesh.normalize(reso=reso, enlarge_scale=enlarge_scale, mult=mult)
    vol_pts = sample_grid_points_aabb(mesh.aabb, reso)
    shape = vol_pts.shape[:3]
    tick("upload")
    pts = mesh._points(vol_pts.reshape(-1, 3))
    tick("bin")
    mesh._binned(thr)
    tick("grid closest")
    dist, face, bary = mesh.closest(pts, thr)
    tick("grid winding")
    wn = mesh.winding_number(pts)
    tick("grid texture")
    vol_sdf = torch.where(wn.abs() >= 0.5, -dist, dist)
    vol_tex = texture(face, bary)                           # face -1 (|sdf| = threshold) gives 0
    out = {"pts_grid": vol_pts, "sdf_grid": vol_sdf.cpu().numpy().reshape(shape), "tex_grid": vol_tex.cpu().numpy().reshape(shape + (-1,)),
           "aabb": mesh.aabb, "threshold": thr, **extra(mesh)}
    if only_vol:
        tick(None)
        return out
    tick("surface samples")
    gen = torch.Generator(device="cuda")
    gen.manual_seed(int(seed))
    on_pts, on_face, on_bary = mesh.sample_surf(n_surf, gen)
    on_tex = texture(on_face, on_bary)
    tick("near-surface samples")
    lo = torch.from_numpy(mesh.aabb[:3].astype(np.float32)).to(on_pts.device)
    hi = torch.from_numpy(mesh.aabb[3:].astype(np.float32)).to(on_pts.device)
    noise = torch.randn(on_pts.shape, generator=gen, device=on_pts.device, dtype=torch.float32)
    near_pts = torch.minimum(torch.maximum(on_pts + noise * NEAR_SURF_SIGMA, lo), hi).contiguous()
    near_sdf, near_face, near_bary = mesh.query_sdf(near_pts, thr, with_closest=True)
    near_tex = texture(near_face, near_bary)
    tick("download")
    out.update(pts_on_surf=on_pts.cpu().numpy(), tex_on_surf=on_tex.cpu().numpy(), pts_near_surf=near_pts.cpu().numpy(),
               sdf_near_surf=near_sdf.cpu().numpy(), tex_near_surf=near_tex.cpu().numpy())
    tick(None)
    return out


def prepare(mesh, reso=256, n_surf=2_000_000, mult=8, threshold=None, enlarge_scale=1.03, only_vol=False, seed=0, timer=None):
    """The dictionary the CLI saves (reference :152-222).  timer(name) is called at the start of every stage (tools/bench_prepare.py)."""
    return prepare_stages(mesh, mesh.colors, lambda m: {"Ka": m.Kas[0], "Kd": m.Kds[0], "Ks": m.Kss[0], "Ns": m.Nss[0]}, reso=reso,
                          n_surf=n_surf, mult=mult, threshold=threshold, enlarge_scale=enlarge_scale, only_vol=only_vol, seed=seed, timer=timer)


def run_cli(args, sampler, prepare_fn):
    """What main does after parsing: refuse without a GPU, read args.src with `sampler`, save prepare_fn's dictionary to args.dst."""
    _lib.require_gpu()                                     # before any work: no CPU fallback
    print("threshold:", args.threshold)
    mesh = sampler(args.src)
    out = prepare_fn(mesh, reso=args.reso, n_surf=args.n_surf, mult=args.mult, threshold=args.threshold, enlarge_scale=args.enlarge_scale,
                     only_vol=args.only_vol, seed=args.seed)
    os.makedirs(os.path.dirname(os.path.abspath(args.dst)), exist_ok=True)
    np.savez_compressed(args.dst, **out)
    for k in out:
        print(f"{k}: {np.asarray(out[k]).shape}")
    return 0


def main(argv=None):
    return run_cli(parse_args(argv), MeshSampler, prepare)


if __name__ == "__main__":
    sys.exit(main())
