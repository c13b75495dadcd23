"""Multi-view renders of a mesh file with the flags of the reference's rendering/blender_render_multiview.py:

    python -m sin3dm_amd.rendering.render_multiview -s mesh.obj -o DIR [--image_resolution W H] [--supersample N]
           [--shading flat|smooth|pbr] [--shadows]

writes DIR/000.png ... 007.png (RGBA, transparent background): the eight views of the reference's rig, drawn by the device
rasteriser (rasterizer.py; DESIGN.md §22 — not Blender: flat shading, one overhead light, shadows opt-in).  Reads textured OBJs
(+ MTL, images) through data/obj_io.load_obj and the vertex-coloured OBJ of isosurface.export_obj (`v x y z r g b`).
--shading smooth: the same colours under smooth normals and the three-light GGX model of DESIGN.md §24; pbr: also the MTL's
metallic, roughness and normal maps (rendering/pbr.py).  The default, flat, is the shader of §22, bit for bit.
--shadows: hard shadows of the mesh on itself under the three lights of §24 (with --shading flat: that light model
on flat normals)."""
from __future__ import annotations

import argparse
import os

import numpy as np


def build_parser():
    p = argparse.ArgumentParser(prog="sin3dm_amd.rendering.render_multiview", description=__doc__.split("\n\n")[0])
    p.add_argument("-s", "--mesh_path", type=str, required=True, help="the OBJ to render (textured, or vertex-coloured `v x y z r g b`)")
    p.add_argument("-o", "--output_dir", type=str, required=True, help="where 000.png ... 007.png are written (created if missing)")
    p.add_argument("--image_resolution", nargs=2, type=int, default=(512, 512), metavar=("W", "H"), help="size of every view in pixels")
    p.add_argument("--supersample", type=int, default=2, help="samples per pixel and axis (1 to 8)")
    p.add_argument("--shading", type=str, default="flat", choices=["flat", "smooth", "pbr"], help="flat: one light, flat normals (the default)")
    p.add_argument("--shadows", action="store_true", help="shadow rays against the mesh itself (the light model of --shading smooth, on flat normals under flat)")
    return p


def parse_args(argv=None):
    args = build_parser().parse_args(argv)
    args.image_resolution = tuple(args.image_resolution)
    if min(args.image_resolution) < 1:
        raise SystemExit(f"--image_resolution {args.image_resolution}: both must be positive")
    if not 1 <= args.supersample <= 8:
        raise SystemExit(f"--supersample {args.supersample}: 1 to 8")
    return args


def read_vertex_colors(text):
    """float64 [V, 3] from the `v x y z r g b` lines of an OBJ text, or None unless EVERY vertex line carries a colour."""
    cols, n = [], 0
    for line in text.splitlines():
        tok = line.split("#", 1)[0].split()
        if not tok or tok[0] != "v":
            continue
        n += 1
        if len(tok) >= 7:
            cols.append([float(x) for x in tok[4:7]])
    if n == 0 or len(cols) != n:
        return None
    return np.clip(np.asarray(cols, dtype=np.float64), 0.0, 1.0)


def load_mesh(path):
    """load_obj plus "vertex_colors" ([V, 3] or None); "textured": some material has an image."""
    from ..data import obj_io
    mesh = obj_io.load_obj(path)
    with open(path, errors="replace") as fh:
        mesh["vertex_colors"] = read_vertex_colors(fh.read())
    mesh["textured"] = any(m.get("image") is not None for _, m in mesh["materials"])
    return mesh


def write_views(images, out_dir):
    """images uint8 [n, H, W, 4] -> out_dir/000.png ...; returns the paths."""
    from ..encoding.isosurface import png_bytes
    os.makedirs(out_dir, exist_ok=True)
    paths = []
    for i, im in enumerate(images):
        paths.append(os.path.join(out_dir, f"{i:03d}.png"))
        with open(paths[-1], "wb") as fh:
            fh.write(png_bytes(im))
    return paths


def render_mesh_file(path, out_dir, resolution=(512, 512), supersample=2, shading="flat", shadows=False):
    import torch
    from .rasterizer import render_views
    mesh = load_mesh(path)
    if shading == "pbr":
        from . import pbr
        pbr.load_pbr_maps(path, mesh["materials"])
    dev = torch.device("cuda")
    verts = torch.from_numpy(mesh["verts"].astype(np.float32)).to(dev)
    faces = torch.from_numpy(mesh["faces"].astype(np.int32)).to(dev)
    kw = {}
    if mesh["vertex_colors"] is not None and not mesh["textured"]:
        kw["vertex_colors"] = torch.from_numpy(mesh["vertex_colors"].astype(np.float32)).to(dev)
    else:
        kw.update(uvs=torch.from_numpy(mesh["uvs"].astype(np.float32)).to(dev), face_mat=torch.from_numpy(mesh["face_mat"]).to(dev),
                  materials=[m for _, m in mesh["materials"]])
    if shading != "flat":                                   # (the default call stays the one it always was)
        kw["shading"] = shading
    if shadows:
        kw["shadows"] = True
    images = render_views(verts, faces, resolution=resolution, supersample=supersample, **kw)
    return write_views(images.cpu().numpy(), out_dir)


def main(argv=None):
    args = parse_args(argv)
    paths = render_mesh_file(args.mesh_path, args.output_dir, args.image_resolution, args.supersample, args.shading, args.shadows)
    print(f"wrote {len(paths)} views under {args.output_dir}")
    return paths


if __name__ == "__main__":
    main()
