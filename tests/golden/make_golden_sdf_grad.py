#!/usr/bin/env python3
"""Generate tests/golden/sdf_grad.npz by IMPORTING the reference (PyTorch-CPU): the float32 autograd gradient, with respect
to the points, of the sdf of the reference's own AutoEncoderGroupSkip.decode (src/encoding/networks.py:192-220) on one small
geometry-only case, and the same in float64.

Data only (make_golden.py's rules): inputs + the reference's outputs.  Weights are NOT stored: they are
sin3dm_amd.testing.synthetic_tensor(name, shape, 5), and this script asserts the manifest against the module's state_dict.

    python tests/golden/make_golden_sdf_grad.py

The box is [-1,1]^3 and the planes are 4 x 8 x 2, so that a texel centre is an exact float32 point whose sample position is
an exact integer: the first rows pin F.grid_sample's conventions at the kinks of the gradient,
  rows 0..2   one axis each beyond the low / the high border (-1.5, +1.25; just outside the outermost centres): 0 there,
  rows 3..5   one axis each ON an interior texel centre: the derivative of the cell that floor selects,
and the other 58 rows are uniform in +-1.15.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import T, planes, quiet, save  # noqa: E402  (puts the reference on sys.path)
from make_golden_pbr import load  # noqa: E402

from encoding.networks import AutoEncoderGroupSkip  # noqa: E402

UP, HID, H, W, D = 16, 32, 4, 8, 2
N = 64


def points():
    g = np.random.Generator(np.random.PCG64(901))
    x = g.uniform(-1.15, 1.15, size=(N, 3))
    c = lambda s, i: -1.0 + (2 * i + 1) / s                     # noqa: E731  texel centre i of a plane side of s texels
    x[0] = [-1.5, 0.3, c(D, 0) - 0.125]                          # axis 0 far below, axis 2 just outside the first centre
    x[1] = [0.1, 1.25, -0.2]                                     # axis 1 far above
    x[2] = [c(H, H - 1) + 0.0625, c(W, 0) - 0.03125, 1.5]        # just outside the last / first centre, far above
    x[3] = [c(H, 1), 0.3, 0.1]                                   # ON an interior centre of axis 0
    x[4] = [0.2, c(W, 3), -0.3]                                  # ... of axis 1
    x[5] = [c(H, 2), c(W, 5), 0.2]                               # ... of axes 0 and 1
    return torch.from_numpy(x.astype(np.float32))


def grad_of(net, pts, fm, aabb):
    p = pts.clone().requires_grad_(True)
    with torch.enable_grad():
        y = net.decode(p, fm, aabb=aabb)[:, 0]
        (g,) = torch.autograd.grad(y.sum(), p)
    return y.detach(), g


def main():
    shapes = T.geo_only_param_shapes(4, UP, HID, 4)
    net = load(quiet(AutoEncoderGroupSkip, 4, 8, UP, HID, 4, use_tex=False), shapes)
    fm = [(0.8 * torch.tanh(x))[:, :4].contiguous() for x in planes(1, 12, H, W, D, 800)]
    aabb = torch.tensor([-1.0, -1.0, -1.0, 1.0, 1.0, 1.0])
    pts = points()
    sdf, g = grad_of(net, pts, fm, aabb)
    net.double()
    sdf64, g64 = grad_of(net, pts.double(), [f.double() for f in fm], aabb.double())
    gap = float((g.double() - g64).abs().max() / g64.abs().max())
    print(f"max|grad| {float(g64.abs().max()):.3f}, float32 vs float64 gap {gap:.2e}, clamped components exactly 0: "
          f"{bool(g[0, 0] == 0 and g[0, 2] == 0 and g[1, 1] == 0 and (g[2] == 0).all())}")
    assert g[0, 0] == 0 and g[0, 2] == 0 and g[1, 1] == 0 and (g[2] == 0).all()
    save("sdf_grad", xy=fm[0], xz=fm[1], yz=fm[2], aabb=aabb, pts=pts, sdf=sdf, grad=g, sdf64=sdf64, grad64=g64,
         gap=np.asarray(gap), cfg=np.asarray([UP, HID, H, W, D]))


if __name__ == "__main__":
    main()
