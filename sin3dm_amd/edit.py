"""Outpainting and local editing CLI: known-region sampling from a trained experiment.

    python -m sin3dm_amd.edit --tag EXP --outpaint 0 0 0 0.5 0 0 [--resample 2] [sample.py's flags]
    python -m sin3dm_amd.edit --tag EXP --keep 0 1 0 0.5 0 1 [--resize 1 1.5 1] [--feather 2]
    python -m sin3dm_amd.edit --tag EXP --keep 0 1 0 0.4 0 1 --paste 0 1 0 0.4 0 1  0 0.6 0 ...

--keep x0 x1 y0 y1 z0 z1     (repeatable) the source cells of this box stay where they are; fractions of the SOURCE volume
--paste x0 x1 y0 y1 z0 z1 X Y Z   (repeatable) the source cells of the box appear with their low corner at (X, Y, Z), fractions of
                             the canvas; --keep and --paste apply in the order keep, then paste, later ones on top
--outpaint xl xh yl yh zl zh the canvas is the source grown by these fractions of its size below / above each axis and the whole
                             source is kept at that offset (on the planes that contain a grown axis unless --planes says otherwise)
--planes xy,xz,yz            restrict every operation to these planes
--feather N                  a linear mask ramp over N cells inside each box
--resample R                 every step but the last runs R times with a re-noising in between (RePaint's resampling)

--resize sets the canvas for --keep / --paste (as for sample.py); --outpaint sets its own.  Everything else — flags, lanes and
chains at batch 1 and 2, S3D_NOISE / S3D_MESH / S3D_DECIMATE / S3D_MESH_NORMAL_MAP / S3D_MESH_SPARSE, S3D_SAMPLER (the few-step samplers of DESIGN.md section 26; not with
--resample > 1), the per-sample feat.npz and mesh files, the aabb scaled with the canvas — is sin3dm_amd.sample's.  A box marks its projection on each plane, and a plane pixel stands for a whole column of the
volume (sin3dm_amd/utils/region_util.py).
"""
from __future__ import annotations

import argparse
import math

from . import parallel, sample
from .utils import dist_util, region_util
from .utils.parser_util import encoding_feat_path, sample_args


def edit_parser():
    p = argparse.ArgumentParser(add_help=False, allow_abbrev=False)
    p.add_argument("--keep", type=float, nargs=6, action="append", default=[], metavar="F")
    p.add_argument("--paste", type=float, nargs=9, action="append", default=[], metavar="F")
    p.add_argument("--outpaint", type=float, nargs=6, default=None, metavar="F")
    p.add_argument("--planes", type=str, default=None)
    p.add_argument("--feather", type=int, default=0)
    p.add_argument("--resample", type=int, default=1)
    return p


def edit_args(argv=None):
    """(the edit flags, sample_args of everything else): sample_args sees the remaining argv unchanged."""
    ed, rest = edit_parser().parse_known_args(argv)
    if ed.outpaint is None and not ed.keep and not ed.paste:
        raise ValueError("nothing to do: give --keep, --paste or --outpaint")
    if ed.outpaint is not None and (ed.keep or ed.paste):
        raise ValueError("--outpaint sets its own canvas and cannot be combined with --keep / --paste")
    if ed.resample < 1 or ed.feather < 0:
        raise ValueError("--resample must be >= 1 and --feather >= 0")
    if ed.resample > 1 and sample.sampler_choice():
        raise ValueError(f"--resample {ed.resample} with S3D_SAMPLER={sample.sampler_choice()}: a re-noised step would need the multistep history restarted")
    return ed, sample_args(rest)


def plan(ed, src_hwd, resize=(1, 1, 1)):
    """(canvas (H, W, D), operations of region_util) for the edit flags on a source of src_hwd cells."""
    planes = ed.planes
    if ed.outpaint is not None:
        if tuple(float(r) for r in resize) != (1.0, 1.0, 1.0):
            raise ValueError("--outpaint sets its own canvas: leave --resize out")
        grow = tuple((int(math.ceil(ed.outpaint[2 * a] * n)), int(math.ceil(ed.outpaint[2 * a + 1] * n))) for a, n in enumerate(src_hwd))
        return region_util.outpaint_canvas(src_hwd, grow), [region_util.outpaint(grow, planes=planes, feather=ed.feather)]
    canvas = tuple(int(s * r) for s, r in zip(src_hwd, resize))
    ops = [region_util.keep(region_util.cells_from_fractions(b, src_hwd), planes=planes, feather=ed.feather) for b in ed.keep]
    for b in ed.paste:
        dst = tuple(int(math.floor(f * n)) for f, n in zip(b[6:], canvas))
        ops.append(region_util.paste(region_util.cells_from_fractions(b[:6], src_hwd), dst, planes=planes, feather=ed.feather))
    return canvas, ops


def main(argv=None):
    from .diffusion.gaussian_diffusion import KnownRegion
    from .utils.triplane_util import load_triplane_data
    ed, args = edit_args(argv)
    rank, local, world = parallel.env_rank_world()
    dist_util.setup_dist(local if world > 1 else args.gpu_id)
    parallel.init(device=dist_util.dev())
    src = load_triplane_data(encoding_feat_path(args.tag), device=dist_util.dev(), compose=False)
    src_hwd = (src[0].shape[1], src[0].shape[2], src[1].shape[2])
    canvas, ops = plan(ed, src_hwd, args.resize)
    y0, mask = region_util.build_known(src, canvas, ops)
    paths = sample.sample_diffusion(args, rank, world, hwd=canvas, loop_kw=dict(known=KnownRegion(y0, mask), resample=ed.resample))
    sample.decode(args, paths)
    all_paths = sorted(p for ps in parallel.gather_objects(paths) for p in ps)
    if rank == 0:
        print(f"wrote {len(all_paths)} edited samples under {args.tag}/{args.output}")
    parallel.shutdown()
    return all_paths


if __name__ == "__main__":
    from .launcher import maybe_spawn_module
    rc = maybe_spawn_module("sin3dm_amd.edit")
    if rc is not None:
        raise SystemExit(rc)
    main()
