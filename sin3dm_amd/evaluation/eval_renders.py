"""python -m sin3dm_amd.evaluation.eval_renders -s SRC -r REF --inception_weights W --alexnet_weights W --lpips_weights W: the
renderings part of the reference's evaluation/eval_full.py.

SRC/*/renderings (sorted) hold the generated samples' views, REF/renderings the training shape's, as NNN.png
(python -m sin3dm_amd.rendering.render_multiview writes them).  Writes mv_sifid_dim64, mv_sifid_dim192 and mv_lpips as JSON.
The three checkpoints are torchvision's inception_v3 and alexnet state dicts and the reference's lpips_weights.ckpt.
"""
from __future__ import annotations

import argparse
import glob
import json
import os

KEYS = ("mv_sifid_dim64", "mv_sifid_dim192", "mv_lpips")


def add_weight_arguments(parser):
    parser.add_argument("--inception_weights", type=str, required=True, help="state dict of torchvision's inception_v3 (SIFID)")
    parser.add_argument("--alexnet_weights", type=str, required=True, help="state dict of torchvision's alexnet (LPIPS)")
    parser.add_argument("--lpips_weights", type=str, required=True, help="the reference's lpips_weights.ckpt (LPIPS)")


def build_parser():
    parser = argparse.ArgumentParser(prog="python -m sin3dm_amd.evaluation.eval_renders", description=__doc__.split("\n\n")[0])
    parser.add_argument("-s", "--src", type=str, required=True, help="generated data folder: SRC/<sample>/renderings/NNN.png")
    parser.add_argument("-r", "--ref", type=str, required=True, help="reference data folder: REF/renderings/NNN.png")
    add_weight_arguments(parser)
    parser.add_argument("-o", "--output", type=str, default=None, help="result save path (default: SRC + '_eval_renders.json')")
    return parser


def parse_args(argv=None):
    return build_parser().parse_args(argv)


def find_renders(src, ref):
    gen = sorted(glob.glob(os.path.join(src, "*/renderings")))
    ref_dir = os.path.join(ref, "renderings")
    if not gen:
        raise FileNotFoundError(f"no */renderings under {src}")
    if not os.path.isdir(ref_dir):
        raise FileNotFoundError(f"no renderings under {ref}")
    return gen, ref_dir


def eval_renders(gen_render_dirs, ref_render_dir, inception_weights, alexnet_weights, lpips_weights):
    """The three keys in eval_full.py's order; each network is loaded once."""
    from .lpips import AlexNetLpips, eval_lpips
    from .sifid import InceptionStem, eval_sifid
    stem = InceptionStem(inception_weights)
    result = {}
    result.update(eval_sifid(gen_render_dirs, ref_render_dir, stem, 64))
    result.update(eval_sifid(gen_render_dirs, ref_render_dir, stem, 192))
    result.update(eval_lpips(gen_render_dirs, AlexNetLpips(alexnet_weights, lpips_weights)))
    return result


def main(argv=None):
    args = parse_args(argv)
    from .. import _lib
    _lib.require_gpu()
    gen, ref_dir = find_renders(args.src, args.ref)
    result = eval_renders(gen, ref_dir, args.inception_weights, args.alexnet_weights, args.lpips_weights)
    print(result)
    save_path = args.output if args.output is not None else args.src + "_eval_renders.json"
    with open(save_path, "w") as fp:
        json.dump(result, fp, indent=4)
    return result


if __name__ == "__main__":
    main()
