#!/usr/bin/env python3
"""Generate tests/golden/pbr_decoder.npz by IMPORTING the reference (PyTorch-CPU): the decode of AutoEncoderGroupPBR, of
the geometry-only AutoEncoderGroupSkip(use_tex=False) and of the skip net with 8 texture channels.

Data only (make_golden.py's rules): inputs + the reference's outputs.  Weights are NOT stored: they are
sin3dm_amd.testing.synthetic_tensor(name, shape, 5), and this script asserts that the manifest it uses
(T.pbr_param_shapes / T.geo_only_param_shapes / T.ae_param_shapes) equals the reference modules' own state_dict.

    python tests/golden/make_golden_pbr.py

Inputs are those of make_golden.py:gen_decoder: planes 0.8*tanh(noise) (seeds 800..802), aabb [-0.7,-1,-0.45,0.7,1,0.45],
257 points uniform in +-1.15 x extent (two full 128-point blocks + one tail point; ~13 % of the coordinates outside the box
exercise the border clamp).  The geometry-only nets take the first 4 channels of the same planes.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import T, planes, quiet, save  # noqa: E402  (puts the reference on sys.path)

from encoding.networks import AutoEncoderGroupPBR, AutoEncoderGroupSkip  # noqa: E402

SIZES = {"small": (16, 32, 10, 14, 6), "wide": (64, 256, 9, 8, 11)}
AABB = [-0.7, -1.0, -0.45, 0.7, 1.0, 0.45]


def relerr(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b)) / max(float(np.max(np.abs(b))), 1e-30))


def load(net, shapes):
    """Synthetic weights (seed 5) into a reference module; the manifest must be its state_dict minus encoders and aabb."""
    sd = T.synthetic_state_dict(shapes, 5)
    ref = {k: tuple(v.shape) for k, v in net.state_dict().items() if not k.startswith(("geo_encoder", "tex_encoder", "aabb"))}
    assert list(ref) == list(shapes) and all(ref[k] == tuple(shapes[k]) for k in ref), sorted(set(ref) ^ set(shapes))
    missing, unexpected = net.load_state_dict(sd, strict=False)
    assert not unexpected and all(k.startswith(("geo_encoder", "tex_encoder", "aabb")) for k in missing), missing
    return net.eval()


def inputs(H, W, D):
    fm = [0.8 * torch.tanh(x) for x in planes(1, 12, H, W, D, 800)]
    aabb = torch.tensor(AABB)
    g = np.random.Generator(np.random.PCG64(900))
    pts = torch.from_numpy(g.uniform(-1.15, 1.15, size=(257, 3)).astype(np.float32)) * aabb[3:]
    return fm, aabb, pts


def main():
    out = {}
    for tag, (up, hid, H, W, D) in SIZES.items():
        fm, aabb, pts = inputs(H, W, D)
        # ---- AutoEncoderGroupPBR
        shapes = T.pbr_param_shapes(4, 8, up, hid, 4, 8)
        net = load(quiet(AutoEncoderGroupPBR, 4, 8, up, hid, 4, use_tex=True, tex_channels=8), shapes)
        y = net.decode(pts, fm, aabb=aabb)
        y64 = net.double().decode(pts.double(), [f.double() for f in fm], aabb=aabb.double())
        net.float()
        frac = float(((y[:, 1:] < 0) | (y[:, 1:] > 1)).float().mean())
        print(f"pbr.{tag}: max|out| {float(y.abs().max()):.3f}, material outside [0,1] {100 * frac:.1f} %, "
              f"fp32 vs fp64 relerr {relerr(y, y64):.2e}")
        # both sides of [0,1] are well populated, so a clamp test on these outputs is not vacuous
        assert torch.isfinite(y).all() and float(y.abs().max()) <= 2.6 and 0.3 <= frac <= 0.7
        k = f"pbr.{tag}"
        out[f"{k}.xy"], out[f"{k}.xz"], out[f"{k}.yz"] = fm
        out[f"{k}.aabb"], out[f"{k}.pts"], out[f"{k}.out"] = aabb, pts, y
        out[f"{k}.out_default_aabb"] = net.decode(pts[:33], fm)
        geo = net.geo_convs([f[:, :4] for f in fm])
        tex0 = net.tex_convs[0]([f[:, 4:] for f in fm])
        tex = net.tex_convs[1](tex0)
        for p, a, b, c in zip(T.PLANES, geo, tex0, tex):
            out[f"{k}.geo_{p}"], out[f"{k}.tex0_{p}"], out[f"{k}.tex_{p}"] = a, b, c
        out[f"{k}.cfg"] = np.asarray([up, hid, H, W, D])
        out[f"{k}.param_names"] = np.asarray(list(shapes))
        out[f"{k}.param_shapes"] = np.asarray([list(s) + [0] * (4 - len(s)) for s in shapes.values()])
        # ---- geometry only: the skip net and the PBR net without texture are the same module
        gshapes = T.geo_only_param_shapes(4, up, hid, 4)
        gnet = load(quiet(AutoEncoderGroupSkip, 4, 8, up, hid, 4, use_tex=False), gshapes)
        load(quiet(AutoEncoderGroupPBR, 4, 8, up, hid, 4, use_tex=False), gshapes)      # (same manifest)
        gfm = [f[:, :4].contiguous() for f in fm]
        k = f"geo.{tag}"
        out[f"{k}.out"] = gnet.decode(pts, gfm, aabb=aabb)
        out[f"{k}.out_default_aabb"] = gnet.decode(pts[:33], gfm)
        assert torch.equal(out[f"{k}.out"], y[:, :1])            # the geo side of the PBR net is this network
        out[f"{k}.param_names"] = np.asarray(list(gshapes))
        out[f"{k}.param_shapes"] = np.asarray([list(s) + [0] * (4 - len(s)) for s in gshapes.values()])
        # ---- skip net with the 8 channels of data_type sdfpbr
        if tag == "small":
            sshapes = T.ae_param_shapes(4, 8, up, hid, 4, 8)
            snet = load(quiet(AutoEncoderGroupSkip, 4, 8, up, hid, 4, use_tex=True, tex_channels=8), sshapes)
            k = f"skip8.{tag}"
            out[f"{k}.out"] = snet.decode(pts, fm, aabb=aabb)
            out[f"{k}.out_default_aabb"] = snet.decode(pts[:33], fm)
    save("pbr_decoder", **out)


if __name__ == "__main__":
    main()
