"""PBR mesh -> the .npz of a `sdfpbr` experiment, on one MI355X (the reference's data/mesh_sampler_pbr.py, which needs trimesh and
point_cloud_utils; an own design, DESIGN.md §16 "PBR variant" — parity with those libraries is not claimed).

    python -m sin3dm_amd.data.mesh_sampler_pbr -s SRC.obj -d DST.npz [--reso 256 --n_surf 2000000 --mult 8 --threshold T
                                                                       --enlarge_scale 1.03 --only_vol --seed 0]

Geometry (distance, sign, surface samples) is mesh_sampler's, unchanged.  tex_* have eight channels, float32: albedo rgb |
metallic | roughness | normal xyz (reference :121-125), each the nearest texel of its own map by the rule of s3d_meshsdf_texture.

Where the maps of MeshSamplerPBR(path) come from, per channel (albedo, metallic, roughness, normal):
 1. textures/ beside the OBJ, the reference's convention (:29-76), so that a folder prepared for the reference gives the same
    texels: albedo.*; metallicRoughness.*, else metallic.* and / or roughness.*; normal.*.  Of several matches the first in
    sorted order is taken.  A file found there applies to every material.  From metallicRoughness.* channel 0 is metallic and
    channel 1 is roughness — the reference's `[..., :2]` of the image as RGBA, NOT glTF's G = roughness, B = metallic.  When
    metallicRoughness.* is there, metallic.* and roughness.* are not looked at.
 2. a channel without a file there: the material's own MTL entry (map_Kd; map_Pm; map_Pr; map_Bump, map_bump, bump, norm),
    read by rendering.pbr.load_pbr_maps.
 3. otherwise the scalar: Kd; Pm or 0; Pr or 0 (the reference composes zero images for a missing metallic or roughness map);
    the flat normal (128, 128, 255) / 255 for a missing normal map, where the reference raises.
Images are read through PIL as RGB (albedo, normal, metallicRoughness) or L (metallic, roughness).  A file that cannot be read
warns and counts as not there: the next rule applies.  The files isosurface.export_pbr_obj writes satisfy rules 1 and 2 with the
same images.  There is no CPU fallback.
"""
import glob
import os
import sys

import numpy as np

from .. import _lib
from . import obj_io
from .mesh_sampler import MeshSampler, build_parser as _build_parser, parse_args as _parse_args, prepare_stages, run_cli

KEYS_VOL = ("pts_grid", "sdf_grid", "tex_grid", "aabb", "threshold")                                         # reference :177, without Ka..Ns
KEYS_ALL = KEYS_VOL + ("pts_on_surf", "tex_on_surf", "pts_near_surf", "sdf_near_surf", "tex_near_surf")       # reference :210-213


def _first(folder, stem):
    """The first file textures/<stem>.* in sorted order, or None."""
    found = sorted(glob.glob(os.path.join(glob.escape(folder), stem + ".*")))
    return found[0] if found else None


def discover_maps(obj_path):
    """{field: uint8 image} of the maps found in textures/ beside `obj_path` (rule 1 of the module docstring): "image" and
    "normal_image" [H, W, 3], "metallic_image" and "roughness_image" [H, W].  A channel without a readable file has no entry."""
    from ..rendering.pbr import _read_map
    folder = os.path.join(os.path.dirname(os.path.abspath(obj_path)), "textures")
    out = {}
    if not os.path.isdir(folder):
        return out

    def read(stem, channels):
        path = _first(folder, stem)
        return None if path is None else _read_map(path, channels)

    albedo = read("albedo", 3)
    if albedo is not None:
        out["image"] = albedo
    packed = read("metallicRoughness", 3)
    if packed is not None:
        out["metallic_image"] = np.ascontiguousarray(packed[..., 0])
        out["roughness_image"] = np.ascontiguousarray(packed[..., 1])
    else:
        for stem, field in (("metallic", "metallic_image"), ("roughness", "roughness_image")):
            img = read(stem, 1)
            if img is not None:
                out[field] = img
    normal = read("normal", 3)
    if normal is not None:
        out["normal_image"] = normal
    return out


class MeshSamplerPBR(MeshSampler):
    """MeshSampler with the eight material channels of a PBR asset.

    MeshSamplerPBR(path) reads an OBJ, its MTL and the maps in the order of the module docstring; MeshSamplerPBR(verts=, faces=,
    uvs=, face_mat=, materials=) takes arrays, the material dicts as in rendering/pbr.py: Kd, image, and when present
    metallic_image / roughness_image (uint8 [H, W], or [H, W, C] whose first channel is read), normal_image (uint8 [H, W, 3]),
    Pm, Pr.  A material without Pm / Pr gets 0 here (not the renderer's roughness 0.5).  colors and the geometry queries are the
    base class's."""

    def __init__(self, path=None, *, verts=None, faces=None, uvs=None, face_mat=None, materials=None, band=None):
        n_degenerate = None
        if path is not None:
            from ..rendering.pbr import load_pbr_maps
            mesh = obj_io.load_obj(path)
            load_pbr_maps(path, mesh["materials"])
            found = discover_maps(path)
            verts, faces, uvs, face_mat = mesh["verts"], mesh["faces"], mesh["uvs"], mesh["face_mat"]
            materials = [dict(m, **found) for _, m in mesh["materials"]]
            n_degenerate = mesh["n_degenerate"]
        super().__init__(verts=verts, faces=faces, uvs=uvs, face_mat=face_mat, materials=materials, band=band)
        self.path = path
        if n_degenerate is not None:
            self.n_degenerate = n_degenerate
        for m in self.materials:
            m.setdefault("Pm", 0.0)
            m.setdefault("Pr", 0.0)

    def _device(self):
        import torch
        d = super()._device()                               # (normalize drops it, and the PBR entries with it)
        if "pbr_table" not in d:
            from ..rendering.pbr import pack_pbr_materials
            dev = d["tri9"].device
            table, factors, images, image_bytes = pack_pbr_materials(self.materials, dev)
            d["pbr_table"] = torch.from_numpy(table).to(dev).contiguous()
            d["pbr_factors"] = torch.from_numpy(factors).to(dev).contiguous()
            d["pbr_img"], d["pbr_img_bytes"] = images, image_bytes
        return d

    def materials8(self, face, bary, out=None):
        """albedo rgb | metallic | roughness | normal xyz, float32 [n, 8] on the device, of (face, barycentrics) pairs; face -1 gives
        eight zeros.  out: a contiguous float32 device tensor of n * 8 elements to write into (16-byte aligned)."""
        import torch
        d = self._device()
        face, bary = face.contiguous(), bary.contiguous()
        n = face.shape[0]
        if out is None:
            out = torch.empty((n, 8), device=face.device, dtype=torch.float32)
        elif out.dtype != torch.float32 or not out.is_cuda or not out.is_contiguous() or out.numel() != n * 8:
            raise ValueError(f"materials8: out must be a contiguous float32 device tensor of {n * 8} elements, got {out.dtype} {tuple(out.shape)}")
        _lib.check(_lib.load().s3d_meshsdf_texture_pbr(_lib.ptr(face), _lib.ptr(bary), n, _lib.ptr(d["uv"]), _lib.ptr(d["face_mat"]),
                                                       d["uv"].shape[0], _lib.ptr(d["pbr_table"]), _lib.ptr(d["pbr_factors"]),
                                                       len(self.materials), _lib.ptr(d["pbr_img"]), d["pbr_img_bytes"], _lib.ptr(out),
                                                       _lib.stream_ptr()))
        return out.view(n, 8)

    def query_tex(self, points, band=None):
        """The eight channels of the closest surface point where it lies within `band`, 0 elsewhere: float32 [n, 8] on the device."""
        _, face, bary = self.closest(points, band)
        return self.materials8(face, bary)


def build_parser():
    return _build_parser(prog="python -m sin3dm_amd.data.mesh_sampler_pbr",
                         description="PBR OBJ/MTL + textures -> the .npz of a sdfpbr experiment (eight texture channels), on one MI355X")


def parse_args(argv=None):
    return _parse_args(argv, build_parser())


def prepare_pbr(mesh, reso=256, n_surf=2_000_000, mult=8, threshold=None, enlarge_scale=1.03, only_vol=False, seed=0, timer=None):
    """The dictionary the CLI saves (reference :152-213): mesh_sampler.prepare's stages and timer hooks with tex_* [..., 8]; no
    Ka .. Ns keys (the reference's --only_vol line reads attributes it never sets)."""
    return prepare_stages(mesh, mesh.materials8, lambda m: {}, reso=reso, n_surf=n_surf, mult=mult, threshold=threshold,
                          enlarge_scale=enlarge_scale, only_vol=only_vol, seed=seed, timer=timer)


def main(argv=None):
    return run_cli(parse_args(argv), MeshSamplerPBR, prepare_pbr)


if __name__ == "__main__":
    sys.exit(main())
