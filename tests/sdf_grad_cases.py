"""The cases, restatements and metrics of the sdf-gradient tests (s3d_decoder_sdf_grad, k_decode_grad), shared by
tests/test_sdf_grad_host.py and tests/test_sdf_grad_gpu.py.  A plain module: no GPU at import.

Reference: the restatement tests/pbr_cases.py evaluated in float64 on the promoted float32 inputs and differentiated by
torch.autograd with respect to the points.  Yardstick: the same in float32 throughout (one thread); never the reference.
tests/golden/sdf_grad.npz pins that restatement's gradient to the reference's own autograd gradient, kinks included.

Cases: the widths, kinds and plane sizes of decoder_f64_cases.CASES, one per compiled tile pair of k_decode_grad<UPT,HIDT>
plus a padded form of each family, in the non-cubic box pbr_cases.AABB.  The points are this module's own."""
import functools

import numpy as np
import torch

import decoder_f64_cases as D
import pbr_cases as P
from sin3dm_amd import testing as T

EPS32 = D.EPS32
AABB32 = D.AABB32
CASES = D.CASES
POINT_SEED = 92
EXTENT = 1.15
COORDS = ((0, 1), (0, 2), (1, 2))                 # plane p samples rows along axis COORDS[p][0], columns along COORDS[p][1]

# A point is left out of the accuracy metric where the gradient is discontinuous within rounding distance: a hidden
# pre-activation with |z| < DELTA * rms(z of that layer), or an unclamped sample position within DELTA_T texels of one of the
# integers 0 .. size - 1 (texel centres; the two ends are the clamp boundaries).  float32 moves z by a few 1e-7
# rms and a sample position by 2^-24 * 1.15 * 14 < 2^-20 texels.  With 5 * 256 hidden units, 2e-5 leaves out about 2 % of the points of the widest cases.
DELTA = 2e-5
DELTA_T = 2.0 ** -16
LEFT_OUT_CAP = 0.05                               # at most this share of a case's points, and no designed row

# What the float32 yardstick's E_a must stay under on every case: about 1.5 times its worst case as measured on the CPU
# (1.65e-6, case F, axis 1), rounded up.  A case that breaks it is ill-conditioned and gets other inputs, never a wider cap.
CAP32 = 2.5e-6
# Every axis of every case has max|g64| of at least this over the kept points (measured smallest: 0.578, case H, axis 1; the
# one-point launch is judged on the 33-point scale).
AXIS_FLOOR = 0.5
# The device's E_a may be K_DEVICE times max(the float32 yardstick's E_a, 2^-23) on the same case, point set and axis (the floor
# is decoder_f64_cases.ratios': on the one-point launch the yardstick is exact on two axes).  K_DEVICE is twice the worst such
# ratio measured on an MI355X over all cases and axes, rounded up to a power of two: worst measured
# 2.37 (case D <3,4>, axis 1; profiles/sdf_grad_f64.txt), twice that 4.74.
K_DEVICE = 8.0

# ---------------------------------------------------------------------------------------------------------------- points
# Normalised coordinates an axis of a designed row takes (s = the plane size along that axis); 1/8 texel = 0.25 / s.
VALUES = ("-1.5", "+1.5", "just outside the first centre", "just outside the last centre", "centre 1 - 1/8 texel", "centre 1 + 1/8 texel")
# Designed row i takes VALUES[TABLE[i][axis]].  Rows 0..5 give every axis every value; row 0 (the one-point launch) has an axis
# beyond a border and both sides of a centre; row 8 lies outside every plane.  A row never sits on a centre itself, where the
# derivative jumps and the float32 rounding of the point picks the side.
TABLE = ((0, 4, 5), (4, 1, 3), (5, 2, 0), (1, 5, 4), (2, 0, 1), (3, 3, 2), (4, 4, 4), (5, 5, 5), (0, 1, 0), (2, 3, 3))
DESIGNED_AT = D.DESIGNED_AT


def designed_rows(n):
    return D.designed_rows(n)


def _value(v, s):
    return {0: -1.5, 1: 1.5, 2: -1.0 + 0.75 / s, 3: 1.0 - 0.75 / s, 4: -1.0 + 2.75 / s, 5: -1.0 + 3.25 / s}[v]


@functools.lru_cache(maxsize=None)
def points(case, n):
    """[n,3] float32, read-only: seeded uniform points in +-1.15 of the half extent, the designed rows overwritten."""
    sizes = CASES[case]["hwd"]
    g = np.random.Generator(np.random.PCG64([POINT_SEED, ord(case), n]))
    lo, hi = AABB32[:3].astype(np.float64), AABB32[3:].astype(np.float64)
    x = g.uniform(-EXTENT, EXTENT, size=(n, 3))
    for i, row in enumerate(designed_rows(n)):
        x[row] = [_value(TABLE[i][a], sizes[a]) for a in range(3)]
    pts = ((x + 1) / 2 * (hi - lo) + lo).astype(np.float32)
    pts.setflags(write=False)
    return pts


def sample_positions(case, pts):
    """[n,3,2] float64: the unclamped (row, column) sample position of each point on each plane; sizes [3,2]"""
    H, W, Dd = CASES[case]["hwd"]
    lo, hi = AABB32[:3].astype(np.float64), AABB32[3:].astype(np.float64)
    x = 2 * (np.asarray(pts, np.float64) - lo) / (hi - lo) - 1
    sizes = np.asarray(((H, W), (H, Dd), (W, Dd)), np.float64)
    f = np.stack([np.stack([((x[:, i] + 1) * sizes[p, 0] - 1) / 2, ((x[:, j] + 1) * sizes[p, 1] - 1) / 2], axis=-1)
                  for p, (i, j) in enumerate(COORDS)], axis=1)
    return f, sizes


def beyond_border(case, pts):
    """[n,3] bool: the axis is clamped (by more than DELTA_T) on both planes that hold it: its gradient component is exactly 0"""
    f, sizes = sample_positions(case, pts)
    out = (f < -DELTA_T) | (f > sizes[None] - 1 + DELTA_T)
    res = np.ones((len(f), 3), bool)
    for p, (i, j) in enumerate(COORDS):
        res[:, i] &= out[:, p, 0]
        res[:, j] &= out[:, p, 1]
    return res


# ---------------------------------------------------------------------------------------------------- the two evaluations
# Case B's designed row 63 sat 5e-6 rms from a ReLU kink on decoder_f64_cases' planes (seed 40): other planes, not a smaller DELTA.
PLANE_SEED = {"B": 43}


def _geo_sd(case, dt):
    c = CASES[case]
    return P.weights(c["kind"], c["up"], c["hid"], dtype=dt)


@functools.lru_cache(maxsize=None)
def inputs(case):
    """Three float32 [1,C,h,w] planes (4 channels for the geometry-only net), as torch tensors."""
    c = CASES[case]
    fm = P.synthetic_planes(*c["hwd"], seed=PLANE_SEED.get(case, c["plane_seed"]))
    return tuple(torch.from_numpy(np.ascontiguousarray(f.astype(np.float32))) for f in D.geo_planes(c["kind"], fm))


@functools.lru_cache(maxsize=None)
def geo_feats(case, double):
    """The geometry group's three prepared planes [up,h,w] of the restatement, numpy, read-only"""
    dt = torch.float64 if double else torch.float32
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        fs = P.plane_stage("geo", _geo_sd(case, dt), [f[:, :4].to(dt) for f in inputs(case)])["geo"]
    finally:
        torch.set_num_threads(threads)
    out = tuple(f[0].numpy() for f in fs)
    for a in out:
        assert a.dtype == (np.float64 if double else np.float32)
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def autograd(case, n, double):
    """(sdf [n], grad [n,3]) of the pbr_cases restatement, differentiated by torch.autograd, in float64 or float32 throughout"""
    dt = torch.float64 if double else torch.float32
    feats = {"geo": [torch.from_numpy(f.copy())[None] for f in geo_feats(case, double)]}
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        p = torch.from_numpy(points(case, n).copy()).to(dt).requires_grad_(True)
        y = P.decode("geo", _geo_sd(case, dt), p, list(inputs(case)), AABB32, feats, dtype=dt)[:, 0]
        (g,) = torch.autograd.grad(y.sum(), p)
    finally:
        torch.set_num_threads(threads)
    assert y.dtype == dt and g.dtype == dt
    out = y.detach().numpy(), g.numpy()
    for a in out:
        a.setflags(write=False)
    return out


FAULTS = ("no_border_zero", "s_minus_1", "no_skip_dx", "one_extent")


def manual(case, pts, fault=None, want_z=False):
    """The kernel's algorithm written out in float64 numpy, without autograd: the forward with its ReLU patterns, the chain
    transposed, the planes' bilinear derivative.  (sdf [n], grad [n,3][, the five hidden pre-activations]).  fault: one of
    FAULTS, a deliberately wrong form (the host test shows that the metric sees each)."""
    c = CASES[case]
    up = c["up"]
    sd = {k: v.numpy() for k, v in _geo_sd(case, torch.float64).items() if k.startswith("geo_decoder")}
    W = [sd[f"geo_decoder.{l}.weight"] for l in ("first_layers.0", "first_layers.2", "first_layers.4", "second_layers.0", "second_layers.2", "second_layers.4")]
    B = [sd[f"geo_decoder.{l}.bias"] for l in ("first_layers.0", "first_layers.2", "first_layers.4", "second_layers.0", "second_layers.2", "second_layers.4")]
    feats = geo_feats(case, True)
    f, sizes = sample_positions(case, pts)
    n = len(f)
    gsize = (AABB32[3:] - AABB32[:3]).astype(np.float64)
    cells = []
    x = np.zeros((n, up))
    for p, fm in enumerate(feats):
        h, w = fm.shape[1:]
        fy, fx = f[:, p, 0], f[:, p, 1]
        on_y, on_x = (fy >= 0) & (fy <= h - 1), (fx >= 0) & (fx <= w - 1)
        fy, fx = np.clip(fy, 0, h - 1), np.clip(fx, 0, w - 1)
        y0, x0 = np.floor(fy).astype(int), np.floor(fx).astype(int)
        ty, tx = fy - y0, fx - x0
        y1, x1 = np.minimum(y0 + 1, h - 1), np.minimum(x0 + 1, w - 1)
        c00, c01, c10, c11 = fm[:, y0, x0].T, fm[:, y0, x1].T, fm[:, y1, x0].T, fm[:, y1, x1].T
        x += ((1 - ty) * (1 - tx))[:, None] * c00 + ((1 - ty) * tx)[:, None] * c01 + (ty * (1 - tx))[:, None] * c10 + (ty * tx)[:, None] * c11
        cells.append(((c10 - c00) * (1 - tx)[:, None] + (c11 - c01) * tx[:, None], (c01 - c00) * (1 - ty)[:, None] + (c11 - c10) * ty[:, None],
                      on_y, on_x, h, w))
    z0 = x @ W[0].T + B[0]
    z1 = np.maximum(z0, 0) @ W[1].T + B[1]
    z2 = np.maximum(z1, 0) @ W[2].T + B[2]
    z3 = np.concatenate([x, np.maximum(z2, 0)], axis=1) @ W[3].T + B[3]
    z4 = np.maximum(z3, 0) @ W[4].T + B[4]
    sdf = (np.maximum(z4, 0) @ W[5].T + B[5])[:, 0]
    g = np.broadcast_to(W[5][0], z4.shape) * (z4 > 0)
    g = (g @ W[4]) * (z3 > 0)
    dx = g @ W[3][:, :up]
    g = (g @ W[3][:, up:]) * (z2 > 0)
    g = (g @ W[2]) * (z1 > 0)
    g = (g @ W[1]) * (z0 > 0)
    dx = g @ W[0] + (0 if fault == "no_skip_dx" else dx)
    grad = np.zeros((n, 3))
    for (i, j), (dy_, dx_, on_y, on_x, h, w) in zip(COORDS, cells):
        if fault == "no_border_zero":
            on_y, on_x = np.ones_like(on_y), np.ones_like(on_x)
        sy, sx = ((h - 1) / 2, (w - 1) / 2) if fault == "s_minus_1" else (h / 2, w / 2)
        grad[:, i] += on_y * (dx * dy_).sum(1) * sy * (2 / gsize[0 if fault == "one_extent" else i])
        grad[:, j] += on_x * (dx * dx_).sum(1) * sx * (2 / gsize[0 if fault == "one_extent" else j])
    return (sdf, grad, (z0, z1, z2, z3, z4)) if want_z else (sdf, grad)


@functools.lru_cache(maxsize=None)
def kept(case, n):
    """[n] bool, read-only: the points that enter the accuracy metric (see DELTA, DELTA_T)"""
    pts = points(case, n)
    _, _, zs = manual(case, pts, want_z=True)
    near_relu = np.zeros(n, bool)
    # rms over the case's largest point set, so that the one-point launch is judged on the same scale
    _, _, zs_all = manual(case, points(case, max(CASES[case]["n"])), want_z=True)
    for z, za in zip(zs, zs_all):
        near_relu |= (np.abs(z) < DELTA * np.sqrt(np.mean(za ** 2))).any(axis=1)
    # the kinks of a plane are the integer positions 0 .. size - 1 (the two ends are the clamp boundaries); far beyond a border
    # there is none, whatever the position's fraction (-1.5 on a side of 6 texels samples at -2.0)
    f, sizes = sample_positions(case, pts)
    near_texel = ((np.abs(f - np.round(f)) < DELTA_T) & (f > -0.5) & (f < sizes[None] - 0.5)).any(axis=(1, 2))
    k = ~(near_relu | near_texel)
    k.setflags(write=False)
    return k


def axis_scale(case):
    """max_n |g64[n,a]| over the kept points of the case's largest point set"""
    n = max(CASES[case]["n"])
    return np.abs(autograd(case, n, True)[1][kept(case, n)]).max(axis=0)


def axis_errors(case, n, g, rows=None):
    """(E [3], at [3]): E_a = max_n |g - g64|[n,a] / max_n |g64[n,a]| over the kept points (or those of `rows`), and the point
    of each axis' worst"""
    g64 = autograd(case, n, True)[1]
    rows = np.flatnonzero(kept(case, n)) if rows is None else np.asarray([r for r in rows if kept(case, n)[r]])
    d = np.abs(np.asarray(g, np.float64)[rows] - g64[rows])
    return d.max(axis=0) / axis_scale(case), rows[d.argmax(axis=0)]


def place(case, n, row):
    """Where point `row` of an n-point launch sits, for a failure message (lanes j and j + 32 of its wave)"""
    return dict(point=int(row), block=int(row) // 128, wave=int(row) % 128 // 32, lane=int(row) % 32, designed=int(row) in designed_rows(n))


def yardstick(case, n):
    return axis_errors(case, n, autograd(case, n, False)[1])[0]


# ------------------------------------------------------------------------------------------------------------------ Newton
def newton_step32(p, p0, sdf, g, max_step, max_move):
    """One Newton update of k_decode_grad in numpy float32, every operation rounded once: p <- p0 + clamp((p - clamp(sdf
    g / |g|^2, +-max_step)) - p0, +-max_move) per component, no move where |g|^2 < 1e-20.  -> (p', hit max_step, hit max_move)"""
    p, p0, sdf, g = (np.asarray(a, np.float32) for a in (p, p0, sdf, g))
    ms, mm = np.float32(max_step), np.float32(max_move)
    g2 = (g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2]
    assert g2.dtype == np.float32
    move = g2 >= np.float32(1e-20)
    with np.errstate(divide="ignore", invalid="ignore"):
        s = (sdf[:, None] * g) / g2[:, None]
    sc = np.minimum(np.maximum(s, -ms), ms)
    dm = (p - sc) - p0
    dc = np.minimum(np.maximum(dm, -mm), mm)
    out = np.where(move[:, None], p0 + dc, p).astype(np.float32)
    return out, move[:, None] & (sc != s), move[:, None] & (dc != dm)


def newton64(case, pts, iters, max_step, max_move):
    """The iteration in float64 on the manual restatement -> (p', sdf(p'), grad(p'))"""
    p0 = np.asarray(pts, np.float64)
    p = p0.copy()
    for _ in range(iters):
        sdf, g = manual(case, p)
        g2 = (g * g).sum(1)
        with np.errstate(divide="ignore", invalid="ignore"):
            s = np.clip(sdf[:, None] * g / g2[:, None], -max_step, max_step)
        p = np.where((g2 >= 1e-20)[:, None], p0 + np.clip((p - s) - p0, -max_move, max_move), p)
    return (p, *manual(case, p))


# ------------------------------------------------------------------------------------------------------------- the device
def device_inputs(case):
    return [f.to("cuda:0") for f in inputs(case)], torch.from_numpy(AABB32)


def fixture():
    import os
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sdf_grad.npz"))


def fixture_restated(double):
    """(sdf, grad) of the pbr_cases restatement on the fixture's inputs, by autograd"""
    z = fixture()
    up, hid = int(z["cfg"][0]), int(z["cfg"][1])
    dt = torch.float64 if double else torch.float32
    sd = {k: v.to(dt) for k, v in T.synthetic_state_dict(T.geo_only_param_shapes(4, up, hid, 4), 5).items()}
    p = torch.from_numpy(z["pts"]).to(dt).requires_grad_(True)
    y = P.decode("geo", sd, p, [z["xy"], z["xz"], z["yz"]], z["aabb"], dtype=dt)[:, 0]
    (g,) = torch.autograd.grad(y.sum(), p)
    return y.detach().numpy(), g.numpy()
