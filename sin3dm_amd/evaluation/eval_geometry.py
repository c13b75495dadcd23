"""python -m sin3dm_amd.evaluation.eval_geometry -s SRC -r REF: the geometry part of the reference's evaluation/eval_full.py.

SRC/*/*voxel.npz (sorted) are the generated shapes, the first of REF/*.npz (sorted) is the training shape's SDF grid.  Writes the
five numbers LP-IOU-avg, LP-IOU-percent, LP-F-score-avg, LP-F-score-percent and Div as JSON.

With --ssfid_weights PATH (the reference's classifier checkpoint, Clsshapenet_128.pth) SSFID_avg and SSFID_std come first, in the
order of eval_full.py: seven of its keys.  --ssfid_layer {1,2} selects the classifier layer (default 2, the reference's).  SIFID
and LPIPS are not computed.
"""
from __future__ import annotations

import argparse
import glob
import json
import os
import sys

NOT_COMPUTED = ("eval_geometry: SSFID, SIFID and LPIPS are not computed: they need a 3D classifier checkpoint, Inception and VGG weights "
                "and rendered views, none of which can be obtained offline")
NOT_COMPUTED_WITH_SSFID = ("eval_geometry: SIFID and LPIPS are not computed: they need Inception and VGG weights and rendered views")


def build_parser():
    parser = argparse.ArgumentParser(prog="python -m sin3dm_amd.evaluation.eval_geometry", description=__doc__.split("\n\n")[0])
    parser.add_argument("-s", "--src", type=str, required=True, help="generated data folder: SRC/<sample>/*voxel.npz")
    parser.add_argument("-r", "--ref", type=str, required=True, help="reference data folder: REF/*.npz holds the SDF grid")
    parser.add_argument("--patch_size", type=int, default=11, help="patch size")
    parser.add_argument("--stride", type=int, default=5, help="patch stride")
    parser.add_argument("--patch_num", type=int, default=1000, help="max number of patches sampled from each generated shape")
    parser.add_argument("--ssfid_weights", type=str, default=None,
                        help="classifier checkpoint (Clsshapenet_128.pth): also compute SSFID_avg and SSFID_std")
    parser.add_argument("--ssfid_layer", type=int, default=2, choices=(1, 2), help="classifier layer the SSFID statistics are taken of")
    parser.add_argument("-o", "--output", type=str, default=None, help="result save path (default: SRC + '_eval.json')")
    return parser


def parse_args(argv=None):
    return build_parser().parse_args(argv)


def find_inputs(src, ref):
    gen = sorted(glob.glob(os.path.join(src, "*/*voxel.npz")))
    refs = sorted(glob.glob(os.path.join(ref, "*.npz")))
    if not gen:
        raise FileNotFoundError(f"no */*voxel.npz under {src}")
    if not refs:
        raise FileNotFoundError(f"no *.npz under {ref}")
    return gen, refs[0]


def main(argv=None):
    args = parse_args(argv)
    from .. import _lib
    from .patch_utils import eval_div, eval_lp
    _lib.require_gpu()
    gen, ref = find_inputs(args.src, args.ref)
    print(NOT_COMPUTED if args.ssfid_weights is None else NOT_COMPUTED_WITH_SSFID, file=sys.stderr)
    result = {}
    if args.ssfid_weights is not None:
        from .ssfid import eval_ssfid
        result.update(eval_ssfid(gen, ref, args.ssfid_weights, args.ssfid_layer))
    result.update(eval_lp(gen, ref, args.patch_size, args.stride, args.patch_num))
    result.update(eval_div(gen))
    print(result)
    save_path = args.output if args.output is not None else args.src + "_eval.json"
    with open(save_path, "w") as fp:
        json.dump(result, fp, indent=4)
    return result


if __name__ == "__main__":
    main()
