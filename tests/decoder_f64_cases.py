"""The cases and metrics of the decoder float64-reference tests, shared by tests/test_decoder_f64_host.py,
tests/test_hip_decoder_f64.py and tools/decoder_f64_report.py.  A plain module: no fixtures, no GPU at import.

Reference: the restatement tests/pbr_cases.py (pinned to the reference's own outputs by test_pbr_host.py) evaluated in float64
on the float32 parameter, plane, point and bounding-box values, promoted.  The same restatement in float32 throughout is the
yardstick: a device error is judged as a multiple of the float32 restatement's error on the same case
(tests/test_hip_decoder_f64.py), and the float32 restatement itself is held under the caps below.  It is never the reference.

One case per compiled tile pair of k_decode<UPT,HIDT> (s3d_decoder.hip: run_decode) and the padded forms of each; planes are
tiny, so a case costs a fraction of a second."""
import functools

import numpy as np
import torch

import pbr_cases as P
from sin3dm_amd import testing as T

EPS32 = 2.0 ** -23
AABB32 = np.asarray(P.AABB, np.float32)          # both evaluations and the device take these float32 values
POINT_SEED = 91
EXTENT = 1.15                                     # uniform points in +-EXTENT of the half extent


def _case(kind, up, hid, kernel, hwd, n, grid=None, plane_seed=40):
    return dict(kind=kind, up=up, hid=hid, kernel=kernel, hwd=hwd, n=tuple(n), grid=grid, plane_seed=plane_seed)


# grid: the resolution of the grid-mode run; dims (6,9,4), (8,12,5), (7,11,4): non-cubic, 216 / 480 / 308 cells, no multiple of 128.
# Resolutions and case D's plane seed are chosen so that every CLAMPED grid column keeps a maximum of 0.2 too (with the default
# planes case D's column 7 stays below 0.1 on the grid at every resolution, and the relative metric grows tenfold with it).
CASES = {
    "A": _case("skip", 64, 256, "<2,8>", (9, 8, 11), (257,), grid=9),
    "B": _case("skip8", 32, 256, "<1,8>", (6, 5, 4), (130,)),
    "C": _case("pbr", 32, 64, "<1,2>", (7, 9, 13), (257,), grid=12),
    "D": _case("pbr", 96, 128, "<3,4>", (6, 5, 4), (129,), grid=11, plane_seed=41),
    "E": _case("geo", 48, 256, "<2,8>, up padded", (2, 3, 2), (127,)),
    "F": _case("skip8", 20, 40, "<1,2>, both padded", (10, 14, 6), (128,)),
    "G": _case("pbr", 80, 100, "<3,4>, both padded", (5, 2, 7), (257,)),
    "H": _case("skip", 16, 32, "<1,1>", (2, 2, 2), (1, 33)),      # (2,2,2): the smallest triplane the pipeline produces
}
GRID_CASES = tuple(k for k, c in CASES.items() if c["grid"])
GRID_DIMS = {"A": (6, 9, 4), "C": (8, 12, 5), "D": (7, 11, 4)}

# What the float32 restatement must stay under on every case (conditions on the inputs, about 1.5 times its worst error over the
# cases as measured on the CPU with the point recipe below, rounded up): a case that breaks one is ill-conditioned and gets other
# inputs, never a wider cap.  Measured worst: plane stage 7.2e-7 (case C, tex xy), point stage 1.75e-6 (case C, column 7, a
# normal column), grid mode 2.05e-6 (case C, column 2).
CAPS = dict(plane=1.1e-6, point=3e-6, grid=3.2e-6)
COLUMN_FLOOR = 0.2                                # every output column of every case has max|y64| of at least this, clamped grid columns too

# ---------------------------------------------------------------------------------------------------------------- points
# Designed rows.  Normalised coordinates an axis takes (s = the plane size along that axis: H, W, D for axes 0, 1, 2):
VALUES = ("-1", "+1", "first centre", "last centre", "interior centre", "-1.5", "+1.5")
# Row i of the designed rows takes VALUES[TABLE[i][axis]] on each axis.  Rows 0..2 give every axis a low clamp, a high clamp and
# a texel centre (all case H's 33 points have room for); rows 0..7 give every axis every value; row 3 sits on first / last texel
# centres on all three planes (where align_corners=True is furthest off), row 4 outside every plane (where zero padding is).
TABLE = ((0, 1, 2), (1, 2, 0), (2, 0, 1), (3, 2, 3), (5, 6, 5), (4, 4, 4), (6, 5, 6), (2, 3, 2), (1, 1, 1), (0, 0, 0))
# first and last lane of every wave of block 0, the first lane of the tail block, and the last point
DESIGNED_AT = (0, 31, 32, 63, 64, 95, 96, 127, 128)
TEXEL_TOL = 2.0 ** -18                            # "at a texel centre": see input_conditions


def designed_rows(n):
    return sorted({i for i in DESIGNED_AT if i < n} | {n - 1})


def _value(v, s):
    return {0: -1.0, 1: 1.0, 2: -1.0 + 1.0 / s, 3: 1.0 - 1.0 / s, 4: -1.0 + 3.0 / s, 5: -1.5, 6: 1.5}[v]


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


def normalised(case, n):
    """[n,3] float64: the points in the box's normalised coordinates, computed in float64 from the float32 values"""
    lo, hi = AABB32[:3].astype(np.float64), AABB32[3:].astype(np.float64)
    return 2 * (points(case, n).astype(np.float64) - lo) / (hi - lo) - 1


def input_conditions(case, n):
    """In float64 on the float32 points: per plane and per sampled coordinate (row, column) the number of points clamped low
    (sample position < 0), clamped high (> size - 1) and at a texel centre without a clamp (the bilinear fraction tx == 0), among
    all points and among the designed rows: {(plane, "row"|"col"): {"low": (all, designed), "high": .., "centre": ..}}.
    A designed coordinate is exact in float64; the float32 point that carries it is rounded, which moves the sample position
    by up to 2^-24 * 1.15 * size: "tx == 0" is |fraction| <= TEXEL_TOL = 2^-18 texels, four times that at size 14."""
    H, W, D = CASES[case]["hwd"]
    pts = points(case, n).astype(np.float64)
    lo, hi = AABB32[:3].astype(np.float64), AABB32[3:].astype(np.float64)
    x = 2 * (pts - lo) / (hi - lo) - 1
    des = np.zeros(n, bool)
    des[designed_rows(n)] = True
    out = {}
    for plane, (i, j), (h, w) in zip(T.PLANES, ((0, 1), (0, 2), (1, 2)), ((H, W), (H, D), (W, D))):
        for which, axis, s in (("row", i, h), ("col", j, w)):
            f = ((x[:, axis] + 1) * s - 1) / 2
            low, high = f < -TEXEL_TOL, f > s - 1 + TEXEL_TOL
            centre = ~low & ~high & (np.abs(f - np.round(f)) <= TEXEL_TOL)
            out[plane, which] = {k: (int(m.sum()), int((m & des).sum())) for k, m in (("low", low), ("high", high), ("centre", centre))}
    return out


# ------------------------------------------------------------------------------------------------------ the two evaluations
def geo_planes(kind, fm):
    return [f[:, :4] for f in fm] if kind == "geo" else list(fm)


@functools.lru_cache(maxsize=None)
def inputs(case):
    """Three float32 [1,C,h,w] planes (4 channels for the geometry-only net), as torch tensors."""
    c = CASES[case]
    return tuple(torch.from_numpy(np.ascontiguousarray(f.astype(np.float32))) for f in geo_planes(c["kind"], P.synthetic_planes(*c["hwd"], seed=c["plane_seed"])))


@functools.lru_cache(maxsize=None)
def restated(case, double, **gather):
    """The restatement of a case in float64 (double) or float32 throughout, as numpy arrays that callers leave unchanged:
    {"feats": {group: [three [up,h,w]]}, "out": {n: [n, cols]}, "grid": [cells, cols] with the material columns clamped}.
    gather: a wrong sampler for the point stage (padding_mode="zeros", align_corners=True)."""
    c = CASES[case]
    dt = torch.float64 if double else torch.float32
    threads = torch.get_num_threads()
    torch.set_num_threads(1)                      # one summation order for the float32 run, whatever the host
    try:
        return _restated(c, case, dt, gather)
    finally:
        torch.set_num_threads(threads)


def _restated(c, case, dt, gather):
    sd = P.weights(c["kind"], c["up"], c["hid"], dtype=dt)
    fm = [f.to(dt) for f in inputs(case)]
    feats = P.plane_stage(c["kind"], sd, fm)
    assert all(f.dtype == dt for fs in feats.values() for f in fs)
    res = {"feats": {g: [f[0].numpy() for f in fs] for g, fs in feats.items()}, "out": {}}
    for n in c["n"]:
        y = P.decode(c["kind"], sd, points(case, n).copy(), fm, AABB32, feats, dtype=dt, **gather)
        assert y.dtype == dt
        res["out"][n] = y.numpy()
    if c["grid"]:
        pts, dims = P.grid_points(AABB32, c["grid"])
        assert dims == GRID_DIMS[case] and pts.dtype == torch.float32, dims
        y = P.decode(c["kind"], sd, pts, fm, AABB32, feats, dtype=dt, **gather)
        y[:, 1:] = y[:, 1:].clamp(0, 1)
        res["grid"] = y.numpy()
    for a in [*res["out"].values(), *(f for fs in res["feats"].values() for f in fs), *([res["grid"]] if c["grid"] else [])]:
        a.setflags(write=False)
    return res


# ---------------------------------------------------------------------------------------------------------------- metrics
def plane_errors(feats, feats64):
    """{(group, plane): max|f - f64| / max|f64| over [up,h,w]} for each feature group the net has."""
    assert sorted(feats) == sorted(feats64)
    out = {}
    for g, fs in feats64.items():
        for name, f, r in zip(T.PLANES, feats[g], fs):
            f, r = np.asarray(f, np.float64), np.asarray(r, np.float64)
            assert f.shape == r.shape, (g, name, f.shape, r.shape)
            out[g, name] = float(np.max(np.abs(f - r)) / np.max(np.abs(r)))
    return out


def column_errors(y, y64, scale=None):
    """(E [cols], at [cols]): E_j = max_n |y[n,j] - y64[n,j]| / max_n |y64[n,j]|, no floor, and the row of each column's worst.
    scale [cols]: the column maxima to divide by, where the rows are part of a larger set (column_scale)."""
    y, y64 = np.asarray(y, np.float64), np.asarray(y64, np.float64)
    assert y.shape == y64.shape and y.ndim == 2, (y.shape, y64.shape)
    d = np.abs(y - y64)
    return d.max(axis=0) / (np.abs(y64).max(axis=0) if scale is None else scale), d.argmax(axis=0)


def column_scale(case):
    """max_n |y64[n,j]| over the case's largest point set.  Case H launches 1 point and 33: the one point is row 0 of the 33 (a
    designed row), and the one-point launch is judged on the columns' scale, not relative to its single value per column (its
    sdf there is 0.006)."""
    return np.abs(restated(case, True)["out"][max(CASES[case]["n"])]).max(axis=0)


def worst_of(d):
    """(value, key) of the largest entry of a map"""
    return max((v, k) for k, v in d.items())


def half_of_column(kind, j):
    """The lane half that stores output column j: rows 0..3 of a head's output tile are lane half 0's, rows 4..7 half 1's
    (k_decode).  Only the skip net's 8 texture channels reach half 1: its columns 5..8."""
    return 1 if kind == "skip8" and j >= 5 else 0


def place(case, n, row, col):
    """Where point `row` of an n-point launch sits, for a failure message: a point belongs to lanes j and j + 32 of its wave."""
    half = half_of_column(CASES[case]["kind"], col)
    return dict(point=int(row), block=int(row) // 128, wave=int(row) % 128 // 32, lane=int(row) % 32 + 32 * half, half=half,
                designed=int(row) in designed_rows(n))


def point_error(case, n, y, y64, rows=None):
    """(worst E_j, j, place of its worst point, E) of an [n, cols] result; rows: the points to take the maximum over (all)"""
    rows = np.arange(n) if rows is None else np.asarray(rows)
    E, at = column_errors(np.asarray(y)[rows], np.asarray(y64)[rows], column_scale(case))
    at = rows[at]
    j = int(np.argmax(E))
    return float(E[j]), j, place(case, n, at[j], j), E


def old_gate(a, b):
    """conftest.relerr: the measure of the gates these tests tighten (max|a-b| / max|b| over the whole array, < 1e-4)"""
    from conftest import relerr
    return relerr(a, b)


def yardstick(case):
    """The float32 restatement against float64: {"plane": worst, "plane_at", "point": worst over the case's point sets,
    "point_col", "point_place", "sdf": column 0 alone (the column that decides the mesh), "grid" (cases with a grid run)}."""
    r32, r64 = restated(case, False), restated(case, True)
    out = {}
    out["plane"], out["plane_at"] = worst_of(plane_errors(r32["feats"], r64["feats"]))
    out["point"] = out["sdf"] = -1.0
    for n in CASES[case]["n"]:
        e, j, where, E = point_error(case, n, r32["out"][n], r64["out"][n])
        out["sdf"] = max(out["sdf"], float(E[0]))
        if e > out["point"]:
            out["point"], out["point_col"], out["point_place"] = e, j, where
    if CASES[case]["grid"]:
        out["grid"] = float(column_errors(r32["grid"], r64["grid"])[0].max())
    return out


# ------------------------------------------------------------------------------------------------------------- the device
def make_net(case):
    """A fresh HIP net of the case on cuda:0 (as test_pbr_gpu.make_net builds it)."""
    from sin3dm_amd.encoding.networks import AutoEncoderGroupPBR, AutoEncoderGroupSkip
    c = CASES[case]
    kind, up, hid = c["kind"], c["up"], c["hid"]
    if kind == "pbr":
        net = AutoEncoderGroupPBR(4, 8, up, hid, 4, use_tex=True, tex_channels=8)
    elif kind == "geo":
        net = AutoEncoderGroupSkip(4, 8, up, hid, 4, use_tex=False)
    else:
        net = AutoEncoderGroupSkip(4, 8, up, hid, 4, use_tex=True, tex_channels=8 if kind == "skip8" else 3)
    missing, unexpected = net.load_state_dict(T.synthetic_state_dict(P.shapes_of(kind, up, hid), 5), strict=False)
    assert not unexpected and all(k.startswith(("geo_encoder", "tex_encoder", "aabb")) for k in missing)
    return net.to("cuda:0").eval()


def device_run(case):
    """A fresh net on the case: {"feats", "out", "grid"} in the shape of restated(), float32 numpy, plus "grid_as_points": the
    grid's float32 cell centres decoded in point mode with clamp_color."""
    c = CASES[case]
    net = make_net(case)
    fm = [f.to("cuda:0") for f in inputs(case)]
    aabb = torch.from_numpy(AABB32)
    res = {"feats": {g: [f[0].cpu().numpy() for f in net.plane_features(fm, g)] for g in restated(case, True)["feats"]}, "out": {}}
    for n in c["n"]:
        res["out"][n] = net.decode(torch.from_numpy(points(case, n).copy()).to("cuda:0"), fm, aabb=aabb).cpu().numpy()
    if c["grid"]:
        grid = net.decode_grid(fm, c["grid"], aabb=aabb)
        assert tuple(grid.shape[:3]) == GRID_DIMS[case], tuple(grid.shape)
        res["grid"] = grid.reshape(-1, grid.shape[-1]).cpu().numpy()
        pts, _ = P.grid_points(AABB32, c["grid"])
        res["grid_as_points"] = net.decode(pts.to("cuda:0"), fm, aabb=aabb, clamp_color=True).cpu().numpy()
    return res


def device_errors(case, res):
    """Errors of a device_run against float64, in the shape of yardstick(), with every plane and column error kept."""
    r64 = restated(case, True)
    out = {"planes": plane_errors(res["feats"], r64["feats"]), "columns": {}}
    out["plane"], out["plane_at"] = worst_of(out["planes"])
    out["point"] = out["sdf"] = -1.0
    for n in CASES[case]["n"]:
        e, j, where, E = point_error(case, n, res["out"][n], r64["out"][n])
        out["columns"][n] = E
        out["sdf"] = max(out["sdf"], float(E[0]))
        if e > out["point"]:
            out["point"], out["point_col"], out["point_place"] = e, j, where
    if CASES[case]["grid"]:
        E, at = column_errors(res["grid"], r64["grid"])
        out["grid"], out["grid_col"], out["grid_cell"] = float(E.max()), int(E.argmax()), int(at[E.argmax()])
        out["grid_vs_points"] = old_gate(res["grid_as_points"], res["grid"])
    return out


def ratios(dev, yard):
    """err_dev / max(err_32, 2^-23) for the stages present"""
    return {k: dev[k] / max(yard[k], EPS32) for k in ("plane", "point", "sdf", "grid") if k in dev}
