"""One PBR render of a mesh file with the flags of the reference's rendering/blender_render_pbr.py:

    python -m sin3dm_amd.rendering.render_pbr -s object.obj [-o out.png] [-az 45] [-el 45] [--rot 0] [--scale 1]
           [--image_resolution W H] [--shading smooth|flat] [--supersample 2] [--shadows]

writes out.png (default: the mesh path with .png) and beside it out_albedo.png, out_metallic.png, out_roughness.png,
out_normal.png — each only when a material of the mesh carries that map or factor, as the reference writes them — and
out_geo.png (grey 134, no maps): one camera of the reference's rig at azimuth / elevation, its key / fill / rim lights as
directional lights, drawn by the device rasteriser (rasterizer.py, pbr.py; DESIGN.md §24 — not Blender: shadows opt-in, no ambient
occlusion, no tone curve).  --shadows: hard shadows of the mesh on itself under the three lights in out.png and
out_geo.png; the material passes do not change.  A vertex-coloured OBJ (`v x y z r g b`, isosurface.export_obj) without texture or PBR entries is
drawn with its colours as the albedo (metallic 0, roughness 0.5): out.png, out_albedo.png, out_geo.png.

-el defaults to 45: the reference's default 0 puts the eye on the rig's vertical axis, where its look-at with z up has no
right vector; -el 0 and -el 180 (any multiple of 180) are refused for that reason."""
from __future__ import annotations

import argparse
import math
import os

import numpy as np

PASS_FILES = (("albedo", "_albedo"), ("metallic", "_metallic"), ("roughness", "_roughness"), ("normal", "_normal"))


def build_parser():
    p = argparse.ArgumentParser(prog="sin3dm_amd.rendering.render_pbr", description=__doc__.split("\n\n")[0])
    p.add_argument("-s", "--mesh_path", type=str, required=True, help="the OBJ to render (+ MTL with map_Kd / map_Pm / map_Pr / map_Bump)")
    p.add_argument("-o", "--output_path", type=str, default=None, help="the shaded image (default: the mesh path with .png)")
    p.add_argument("-az", "--azimuth", type=float, default=45.0, help="azimuth of the camera in degrees")
    p.add_argument("-el", "--elevation", type=float, default=45.0, help="polar angle of the camera in degrees (not a multiple of 180)")
    p.add_argument("--scale", type=float, default=1.0, help="scale of the normalised mesh")
    p.add_argument("--rot", type=float, default=0.0, help="rotation of the mesh about the vertical axis in degrees")
    p.add_argument("--light_radius", type=float, default=2.0)
    p.add_argument("--light_height", type=float, default=10.0)
    p.add_argument("--image_resolution", nargs=2, type=int, default=(512, 512), metavar=("W", "H"), help="size of the images in pixels")
    p.add_argument("--shading", type=str, default="smooth", choices=["smooth", "flat"])
    p.add_argument("--supersample", type=int, default=2, help="samples per pixel and axis (1 to 8)")
    p.add_argument("--shadows", action="store_true", help="shadow rays against the mesh itself for the three lights")
    return p


def parse_args(argv=None):
    args = build_parser().parse_args(argv)
    args.image_resolution = tuple(args.image_resolution)
    if min(args.image_resolution) < 1:
        raise SystemExit(f"--image_resolution {args.image_resolution}: both must be positive")
    if not 1 <= args.supersample <= 8:
        raise SystemExit(f"--supersample {args.supersample}: 1 to 8")
    if not args.scale > 0 or not math.isfinite(args.scale):
        raise SystemExit(f"--scale {args.scale}: must be positive")
    if abs(math.sin(args.elevation / 180 * math.pi)) < 1e-9:
        raise ValueError(f"-el {args.elevation}: the eye would sit on the rig's vertical axis, where the look-at with z up has no right "
                         f"vector (the reference's default 0 is such a value; the default here is 45)")
    if args.output_path is None:
        args.output_path = os.path.splitext(args.mesh_path)[0] + ".png"
    if not args.output_path.endswith(".png"):
        args.output_path += ".png"
    return args


def rot_z(degrees):
    c, s = math.cos(degrees / 180 * math.pi), math.sin(degrees / 180 * math.pi)
    m = np.eye(4)
    m[:2, :2] = [[c, -s], [s, c]]
    return m


def pbr_view(vmin, vmax, azimuth, elevation, resolution, rot=0.0, scale=1.0):
    """(camera.View, world: float64 [3, 3] the rotation from the stored mesh's axes to the rig's): the mesh normalised as in
    camera.normalization_matrix, turned by `rot` about z and scaled (blender_render_pbr.py:57, 84-88), seen from
    camera.camera_position(azimuth, elevation) (:170-177)."""
    from . import camera
    model = np.diag([scale, scale, scale, 1.0]) @ rot_z(rot) @ camera.normalization_matrix(vmin, vmax)
    matrix = camera.view_projection(camera.camera_position(azimuth, elevation), resolution) @ model
    return camera.View(matrix, near=camera.NEAR), rot_z(rot)[:3, :3] @ camera.ROT_X90


def render_pbr_file(args):
    import torch
    from ..encoding.isosurface import png_bytes
    from . import pbr
    from .rasterizer import render_views
    from .render_multiview import load_mesh
    mesh = load_mesh(args.mesh_path)
    materials = [m for _, m in pbr.load_pbr_maps(args.mesh_path, mesh["materials"])]
    dev = torch.device("cuda")
    verts = torch.from_numpy(mesh["verts"].astype(np.float32)).to(dev)
    faces = torch.from_numpy(mesh["faces"].astype(np.int32)).to(dev)
    v = mesh["verts"].reshape(-1, 3)
    lo, hi = (v.min(0), v.max(0)) if len(v) else (np.zeros(3), np.ones(3))
    view, world = pbr_view(lo, hi, args.azimuth, args.elevation, args.image_resolution, args.rot, args.scale)
    rig = pbr.three_light_rig(args.light_radius, args.light_height)
    rig[:, :3] = (rig[:, :3] @ pbr.camera.ROT_X90.T) @ world          # back to the rig's axes, then into the stored mesh's, `rot` included
    info = pbr.has_pbr_info(materials)
    names = ["shaded"] + [n for n, _ in PASS_FILES if info[n]] + ["geo"]
    if mesh["vertex_colors"] is not None and not any(info.values()):
        # the vertex-coloured OBJ of isosurface.export_obj: its colours are the albedo (render_multiview.render_mesh_file does the same)
        kw = dict(vertex_colors=torch.from_numpy(mesh["vertex_colors"].astype(np.float32)).to(dev))
        names = ["shaded", "albedo", "geo"]
    else:
        kw = dict(uvs=torch.from_numpy(mesh["uvs"].astype(np.float32)).to(dev), face_mat=torch.from_numpy(mesh["face_mat"]).to(dev),
                  materials=materials)
    images = render_views(verts, faces, **kw, views=[view], resolution=args.image_resolution, supersample=args.supersample,
                          shading="pbr" if args.shading == "smooth" else "pbr_flat", passes=tuple(names), lights=rig,
                          **({"shadows": True} if args.shadows else {}))
    stem = args.output_path[:-4]
    suffix = dict(PASS_FILES, shaded="", geo="_geo")
    os.makedirs(os.path.dirname(os.path.abspath(args.output_path)), exist_ok=True)
    paths = []
    for n in names:
        paths.append(stem + suffix[n] + ".png")
        with open(paths[-1], "wb") as fh:
            fh.write(png_bytes(images[n][0].cpu().numpy()))
    return paths


def main(argv=None):
    args = parse_args(argv)
    paths = render_pbr_file(args)
    print(f"wrote {len(paths)} images: {', '.join(os.path.basename(p) for p in paths)}")
    return paths


if __name__ == "__main__":
    main()
