"""The sdf gradient without a GPU: the ABI entry and its refusals, the restatement against the reference's recorded autograd
gradient, the conditions on the cases (left-out share, axis floor, float32 caps), the Newton iteration in float64, and injected
faults that the metric must see.  The device tests are tests/test_sdf_grad_gpu.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import sdf_grad_cases as S
from sin3dm_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POINT_SETS = [(case, n) for case, c in S.CASES.items() for n in c["n"]]


def _handle(up=16, hid=32, variant=1):
    lib = _lib.load()
    h = C.c_void_p()
    _lib.check(lib.s3d_decoder_create_variant(C.byref(_lib.DecoderCfg(4, 8, up, hid, 4, 3)), variant, C.byref(h)))
    return lib, h


def test_abi_symbol_and_version():
    """The entry point is exported and bound, and header, binding and library agree on the ABI number.  The number itself stays
    where tests/test_render_host.py, test_render_pbr_host.py and test_ssfid_host.py pin it: a pure addition."""
    lib = _lib.load()
    assert "s3d_decoder_sdf_grad" in _lib.SIGNATURES and hasattr(lib, "s3d_decoder_sdf_grad")
    header = open(os.path.join(REPO, "include", "sin3dm_hip.h")).read()
    assert "s3d_decoder_sdf_grad(" in header
    assert int(re.search(r"#define S3D_ABI_VERSION (\d+)", header).group(1)) == _lib.ABI_VERSION == lib.s3d_abi_version()


def test_refusals_come_before_any_device_call():
    """On a machine without a GPU every refusal below must be the argument check's, not a device error."""
    lib, h = _handle()
    aabb = (C.c_float * 6)(-1, -1, -1, 1, 1, 1)
    buf = (C.c_float * 12)()
    p = C.cast(buf, C.c_void_p)

    def call(hh, n, iters, ms, mm, out=p, pts=p):
        return lib.s3d_decoder_sdf_grad(hh, pts, n, aabb, iters, ms, mm, out, p, p, None)
    try:
        assert call(h, 1, -1, 0.1, 0.1) == _lib.ERR_INVALID
        assert call(h, 1, 2, 0.1, 0.1, out=None) == _lib.ERR_INVALID
        assert call(h, 1, 2, 0.0, 0.1) == _lib.ERR_INVALID
        assert call(h, 1, 2, 0.1, -1.0) == _lib.ERR_INVALID
        assert call(h, 1, 0, 0.0, 0.0, pts=None) == _lib.ERR_INVALID
        assert call(None, 1, 0, 0.0, 0.0) == _lib.ERR_INVALID
        assert call(h, 0, 0, 0.0, 0.0, out=None, pts=None) == 0               # no points: a successful no-op
        assert call(h, 0, 3, 0.1, 0.1, out=None, pts=None) == 0
        assert call(h, 1, 0, 0.0, 0.0, out=None) == _lib.ERR_INVALID       # no prepared triplane
        assert "prepare_triplane" in _lib.last_error()
    finally:
        lib.s3d_decoder_destroy(h)
    for up, hid in ((128, 256), (64, 128), (96, 256)):                         # the widths k_decode refuses
        lib, h = _handle(up, hid)
        try:
            assert call(h, 1, 0, 0.0, 0.0) == _lib.ERR_UNSUPPORTED
            assert call(h, 1, -1, 0.0, 0.0) == _lib.ERR_INVALID
        finally:
            lib.s3d_decoder_destroy(h)


def test_restatement_reproduces_the_reference_gradient():
    """tests/golden/sdf_grad.npz: the float32 autograd gradient of the reference's own decode.  The restatement in float64 lies
    within twice the recorded float32-vs-float64 gap of it; in float32 it repeats it far below that; and the fixture's kink
    rows hold the conventions: exactly 0 beyond a border, the floor cell on a texel centre."""
    z = S.fixture()
    gap, scale = float(z["gap"]), np.abs(z["grad64"]).max()
    assert 0 < gap < 1e-6
    for double in (True, False):
        sdf, g = S.fixture_restated(double)
        e = np.abs(g - z["grad"]).max() / scale
        print(f"restatement ({'float64' if double else 'float32'}) against the fixture: {e:.2e}, recorded gap {gap:.2e}")
        assert e <= 2 * gap
    g = z["grad"]
    assert g[0, 0] == 0 and g[0, 2] == 0 and g[1, 1] == 0 and (g[2] == 0).all() and (g[3:6] != 0).all()
    # rows 3..5 sit ON centres: one-sided differences of the reference's own float64 field pick the floor cell (the + side)
    up, hid, H, W, D = (int(v) for v in z["cfg"])
    import torch
    import pbr_cases as P
    from sin3dm_amd import testing as T
    sd = {k: v.double() for k, v in T.synthetic_state_dict(T.geo_only_param_shapes(4, up, hid, 4), 5).items()}
    fm = [z["xy"], z["xz"], z["yz"]]
    h = 2.0 ** -20
    for row, axis in ((3, 0), (4, 1), (5, 0), (5, 1)):
        p = np.repeat(z["pts"][row:row + 1].astype(np.float64), 2, axis=0)
        p[1, axis] += h
        y = P.decode("geo", sd, torch.from_numpy(p), fm, z["aabb"])[:, 0].numpy()
        assert abs((y[1] - y[0]) / h - z["grad64"][row, axis]) < 1e-6 * scale, (row, axis)


@pytest.mark.parametrize("case,n", POINT_SETS)
def test_case_conditions(case, n):
    """Conditions on the inputs, not measurements: at most 5 % of the points and no designed row left out; the designed rows cover
    both borders on every axis; every axis maximum above the floor; the manual restatement equals autograd; the float32
    yardstick under its cap."""
    keep, des = S.kept(case, n), S.designed_rows(n)
    print(f"case {case}, {n} points: {100 * (1 - keep.mean()):.1f} % left out, designed rows {des}")
    assert 1 - keep.mean() <= S.LEFT_OUT_CAP and keep[des].all()
    assert S.DELTA <= 1e-4 and S.DELTA_T <= 2.0 ** -16
    assert (S.axis_scale(case) >= S.AXIS_FLOOR).all(), S.axis_scale(case)
    pts = S.points(case, n)
    sdf64, g64 = S.autograd(case, n, True)
    sdf_m, g_m = S.manual(case, pts)
    assert np.abs(sdf_m - sdf64).max() < 1e-12 and np.abs(g_m - g64)[keep].max() < 1e-11
    bb = S.beyond_border(case, pts)
    assert (g64[bb] == 0).all() and (g_m[bb] == 0).all()
    if n >= 129:                                     # every designed value on every axis
        f, sizes = S.sample_positions(case, pts[des])
        assert bb[des].any(axis=0).all() and (f < 0).any(axis=0).all() and (f > sizes[None] - 1).any(axis=0).all()
    E = S.yardstick(case, n)
    print(f"  float32 yardstick E = {E}")
    assert (E <= S.CAP32).all()


@pytest.mark.parametrize("case", list(S.CASES))
def test_injected_faults_lift_the_metric(case):
    n = max(S.CASES[case]["n"])
    des = S.designed_rows(n)
    assert S.axis_errors(case, n, S.manual(case, S.points(case, n))[1], rows=des)[0].max() < 1e-11
    for fault in S.FAULTS:
        e = S.axis_errors(case, n, S.manual(case, S.points(case, n), fault)[1], rows=des)[0].max()
        print(f"case {case}, {fault}: {e:.3g} on the designed rows")
        assert e > 100 * S.CAP32, (case, fault, e)


def test_newton_reduces_the_distance_in_float64():
    """The iteration itself (float64, iters=2, the clamp rules) on case C: mean|sdf| over the kept points that start within one
    cell of the surface falls.  The synthetic field is no distance field (|g| reaches 12), so "within one cell" is the first-order
    distance |sdf| / |g| < one cell of a 64-cell grid over the box's longest side; max_step = max_move = that cell.  Measured:
    124 points, factor 0.28 (median of the per-point factors 0.014; case A's 256-wide synthetic field is rougher: 0.39 on 2 points)."""
    case, n = "C", 257
    pts = S.points(case, n)
    cell = float((S.AABB32[3:] - S.AABB32[:3]).max()) / 64
    sdf0, g0 = S.manual(case, pts)
    with np.errstate(divide="ignore", invalid="ignore"):
        near = S.kept(case, n) & (np.abs(sdf0) / np.linalg.norm(g0, axis=1) < cell)
    assert near.sum() >= 8, near.sum()
    p, sdf, g = S.newton64(case, pts, 2, cell, cell)
    assert np.abs(p - pts).max() <= cell * (1 + 1e-12)
    factor = np.abs(sdf[near]).mean() / np.abs(sdf0[near]).mean()
    print(f"{near.sum()} points, mean|sdf| {np.abs(sdf0[near]).mean():.3e} -> {np.abs(sdf[near]).mean():.3e}: factor {factor:.3g}")
    assert factor < 0.5


def test_newton_step32_clamps():
    p0 = np.zeros((4, 3), np.float32)
    g = np.asarray([[1, 0, 0], [0, 2, 0], [0, 0, 0], [1e-11, 0, 0]], np.float32)
    sdf = np.asarray([0.5, 0.02, 1.0, 1.0], np.float32)
    p, hit_s, hit_m = S.newton_step32(p0, p0, sdf, g, 0.25, 0.125)
    assert np.array_equal(p, np.asarray([[-0.125, 0, 0], [0, -0.01, 0], [0, 0, 0], [0, 0, 0]], np.float32))
    assert hit_s[0, 0] and hit_m[0, 0] and not hit_s[1].any() and not hit_m[1].any()


def test_obj_reader_round_trips_normals(tmp_path):
    """A file with vn lines and v//vn or v/vt/vn faces reads back to the same vertices and faces; the normals are ignored."""
    from sin3dm_amd.data.obj_io import load_obj
    v = np.asarray([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32)
    f = np.asarray([[0, 1, 2], [0, 2, 3], [0, 3, 1], [1, 3, 2]])
    vn = v / np.maximum(np.linalg.norm(v, axis=1, keepdims=True), 1)
    for form in ("{0}//{0}", "{0}/{0}/{0}"):
        path = tmp_path / "n.obj"
        with open(path, "w") as fh:
            fh.writelines(f"v {a} {b} {c}\n" for a, b, c in v)
            fh.writelines(f"vt {a} {b}\n" for a, b, _ in v)
            fh.writelines(f"vn {a} {b} {c}\n" for a, b, c in vn)
            fh.writelines("f " + " ".join(form.format(i + 1) for i in tri) + "\n" for tri in f)
        m = load_obj(str(path))
        assert np.array_equal(np.asarray(m["verts"], np.float32), v) and np.array_equal(np.asarray(m["faces"]), f)
