"""python -m sin3dm_amd.evaluation.eval_full -s SRC -r REF --ssfid_weights W --inception_weights W --alexnet_weights W
--lpips_weights W: the ten numbers of the reference's evaluation/eval_full.py, in its order.

The first seven are eval_geometry's (SRC/*/*voxel.npz against the first of REF/*.npz), computed by its functions; the last three
are eval_renders' (SRC/*/renderings against REF/renderings).  Writes them as JSON.
"""
from __future__ import annotations

import argparse
import json

from . import eval_geometry, eval_renders

KEYS = ("SSFID_avg", "SSFID_std", "LP-IOU-avg", "LP-IOU-percent", "LP-F-score-avg", "LP-F-score-percent", "Div") + eval_renders.KEYS


def build_parser():
    parser = argparse.ArgumentParser(prog="python -m sin3dm_amd.evaluation.eval_full", description=__doc__.split("\n\n")[0])
    parser.add_argument("-s", "--src", type=str, required=True, help="generated data folder: SRC/<sample>/{*voxel.npz, renderings/NNN.png}")
    parser.add_argument("-r", "--ref", type=str, required=True, help="reference data folder: REF/*.npz (the SDF grid), REF/renderings/NNN.png")
    parser.add_argument("--patch_size", type=int, default=11, help="patch size")
    parser.add_argument("--stride", type=int, default=5, help="patch stride")
    parser.add_argument("--patch_num", type=int, default=1000, help="max number of patches sampled from each generated shape")
    parser.add_argument("--ssfid_weights", type=str, required=True, help="classifier checkpoint (Clsshapenet_128.pth)")
    parser.add_argument("--ssfid_layer", type=int, default=2, choices=(1, 2), help="classifier layer the SSFID statistics are taken of")
    eval_renders.add_weight_arguments(parser)
    parser.add_argument("-o", "--output", type=str, default=None, help="result save path (default: SRC + '_eval.json')")
    return parser


def parse_args(argv=None):
    return build_parser().parse_args(argv)


def main(argv=None):
    args = parse_args(argv)
    from .. import _lib
    from .patch_utils import eval_div, eval_lp
    from .ssfid import eval_ssfid
    _lib.require_gpu()
    gen, ref = eval_geometry.find_inputs(args.src, args.ref)
    gen_dirs, ref_dir = eval_renders.find_renders(args.src, args.ref)
    result = {}
    result.update(eval_ssfid(gen, ref, args.ssfid_weights, args.ssfid_layer))
    result.update(eval_lp(gen, ref, args.patch_size, args.stride, args.patch_num))
    result.update(eval_div(gen))
    result.update(eval_renders.eval_renders(gen_dirs, ref_dir, args.inception_weights, args.alexnet_weights, args.lpips_weights))
    print(result)
    save_path = args.output if args.output is not None else args.src + "_eval.json"
    with open(save_path, "w") as fp:
        json.dump(result, fp, indent=4)
    return result


if __name__ == "__main__":
    main()
