"""CPU-only: the host half of the ray query and the shadow mask (s3d_ray.hip, sin3dm_amd/rendering/rasterizer.py).
The restatement of tests/render_shadow_cases.py against what is known analytically (the slab's footprint, a convex body), the
measured band and the cap on the rays it leaves out, the faults the GPU comparisons must see — each injected into the Python copy
of the walk —, the arguments the entry points refuse before anything is launched, the grid's host arithmetic and the ABI."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import render_cases as R
import render_shadow_cases as S
from conftest import REPO
from sin3dm_amd import _lib
from sin3dm_amd.rendering import rasterizer

NEW_SYMBOLS = ("s3d_mesh_ray_occluded", "s3d_pbr_shadow_mask", "s3d_pbr_shade_lit")


def test_band_is_the_measured_one_and_the_cap_holds_for_every_case():
    gap, shares = S.measure()
    print("float32 / float64 gap of the pair terms", gap, "recorded", S.RAY_GAP, "band", S.RAY_BAND, "left out", shares)
    assert gap <= S.RAY_GAP <= 1.1 * gap                      # the constant is the measurement, rounded up
    assert S.RAY_BAND == 10 * S.RAY_GAP
    for name, share in shares.items():
        assert share <= R.MAX_LEFT_OUT, (name, share)
    assert S.T_MIN_REL == rasterizer.SHADOW_T_MIN_REL


def test_restatement_gives_the_slab_its_analytic_footprint():
    c = S.case("a_slab")
    xy, iw, face_id, lit, left = S.restated("a_slab")
    rays = S.mask_rays(c, xy, iw, face_id)
    on_floor = rays["f"] < 2
    p = rays["P"][on_floor]
    (x0, _, z0), (x1, _, z1) = S.SLAB
    inside = (p[:, 0] > x0) & (p[:, 0] < x1) & (p[:, 2] > z0) & (p[:, 2] < z1)
    edge = np.minimum(np.abs(np.abs(p[:, 0]) - x1), np.abs(np.abs(p[:, 2]) - z1)) < 1e-3
    keep = ~edge & ~left.reshape(-1)[rays["s"][on_floor]]
    got = lit.reshape(-1)[rays["s"][on_floor]] & 1
    assert keep.sum() > 800 and inside[keep].sum() > 40
    assert np.array_equal(got[keep] == 0, inside[keep])
    top = (rays["f"] >= 2) & (rays["N"][:, 1] > 0)               # the slab's own top sees the light
    assert top.sum() > 20 and (lit.reshape(-1)[rays["s"][top]] & 1).all()


def test_restatement_shadows_no_sample_of_a_convex_body_that_faces_the_light():
    c = S.case("b_convex")
    xy, iw, face_id, lit, left = S.restated("b_convex")
    rays = S.mask_rays(c, xy, iw, face_id)
    for k, light in enumerate(c["lights"]):
        facing = (rays["N"] @ light[:3] > 0) & ~left.reshape(-1)[rays["s"]]
        bit = (lit.reshape(-1)[rays["s"]] >> k) & 1
        assert facing.sum() > 100 and bit[facing].all() and not bit[~(rays["N"] @ light[:3] > 0)].any()


def _generic_mismatches(dims, fault=None):
    g = S.generic()
    tri9 = S.tri9_of(g)
    grid = S.walk_grid(tri9, dims)
    bad = []
    for o, d, skip, t_min, t_max, hit, status, why in g["rays"]:
        got = S.walk(o, d, skip, t_min, t_max, tri9, grid, fault)
        if got != (hit, status):
            bad.append(why)
    return bad


def _subsampled_mask_rays(name, light, step=7):
    c = S.case(name)
    xy, iw, face_id, lit, left = S.restated(name)
    rays = S.mask_rays(c, xy, iw, face_id)
    L = np.asarray(np.asarray(c["lights"][light][:3], dtype=np.float32), dtype=np.float64)
    idx = np.nonzero(rays["N"] @ L > 0)[0][::step]
    return c, rays, L, idx, lit, left


@pytest.mark.parametrize("dims", S.WALK_GRIDS)
def test_walk_copy_agrees_with_the_restatement_on_every_grid(dims):
    assert _generic_mismatches(dims) == []
    for name, light in (("d_overhang_zero", 0), ("e_thin", 0)):
        c, rays, L, idx, lit, left = _subsampled_mask_rays(name, light)
        tri9 = S.tri9_of(c)
        grid = S.walk_grid(tri9, dims)
        for i in idx:
            s = rays["s"][i]
            if left.reshape(-1)[s]:
                continue
            hit, _ = S.walk(rays["P"][i], L, rays["f"][i], S.t_min_of(c), math.inf, tri9, grid)
            assert hit == 1 - ((lit.reshape(-1)[s] >> light) & 1), (name, dims, int(s))


@pytest.mark.parametrize("fault", S.FAULTS)
def test_injected_faults_are_seen_by_the_comparisons_of_the_gpu_test(fault):
    """The GPU test compares the generic rays in full (they are exact) and the masks outside the tie band, on every grid of
    WALK_GRIDS: each fault changes one of those."""
    seen = [dims for dims in S.WALK_GRIDS if _generic_mismatches(dims, fault)]
    print(fault, "seen by the generic rays on grids", seen)
    assert seen, fault
    if fault == "t_min_zero":                                   # the mask sees it too: the duplicated face shadows its twin
        c, rays, L, idx, lit, left = _subsampled_mask_rays("d_overhang_zero", 0, step=3)
        tri9 = S.tri9_of(c)
        grid = S.walk_grid(tri9, None)
        wrong = sum(S.walk(rays["P"][i], L, rays["f"][i], S.t_min_of(c), math.inf, tri9, grid, fault)[0] != 1 - (lit.reshape(-1)[rays["s"][i]] & 1)
                    for i in idx if not left.reshape(-1)[rays["s"][i]])
        assert wrong > 0


def test_grid_box_covers_the_mesh_with_the_slack_the_walk_needs():
    for name in S.CASES:
        tri9 = S.tri9_of(S.case(name)).astype(np.float64)
        c = tri9.reshape(-1, 3)
        lo, hi = (c.min(0), c.max(0)) if len(c) else (np.zeros(3), np.ones(3))
        for grid in S.WALK_GRIDS:
            origin, cell, dims, slack = rasterizer.ray_grid_box(lo, hi, len(tri9), grid)
            assert all(1 <= n <= rasterizer.RAY_MAX_CELLS_PER_AXIS for n in dims) and (grid is None or tuple(dims) == tuple(grid))
            mag = max(np.abs(lo).max(), np.abs(hi).max())
            assert slack >= 4 * 8 * 2.0 ** -24 * mag               # four times the bound of DESIGN.md §29 on the walked position
            assert (origin.astype(np.float64) <= lo - 2 * slack).all()
            assert (origin.astype(np.float64) + np.asarray(dims) * cell >= hi + 2 * slack).all()
    tri9 = S.tri9_of(S.case("e_thin")).astype(np.float64).reshape(-1, 3)
    assert rasterizer.ray_grid_box(tri9.min(0), tri9.max(0), 128)[2][1] == 1     # the thin sheet: one cell across
    assert rasterizer.ray_grid_dims((1.0, 1.0, 1.0), 10 ** 9) == (256, 256, 256) and rasterizer.ray_grid_dims((1.0, 2.0, 4.0), 0) == (1, 1, 1)
    with pytest.raises(ValueError):
        rasterizer.ray_grid_box(np.zeros(3), np.ones(3), 10, (4, 0, 4))


def _buf(n, ctype=C.c_float):
    return (ctype * n)()


def _ray_args(**kw):
    a = dict(origins=_buf(3), dirs=_buf(3), skip=None, n=1, t_min=0.0, t_max=math.inf, tri9=_buf(9), F=1, origin=(C.c_float * 3)(0, 0, 0), cell=1.0,
             dims=(C.c_int * 3)(1, 1, 1), seg=_buf(2, C.c_int64), seg_tri=_buf(1, C.c_int32), n_pairs=1, hit=_buf(1, C.c_uint8), status=_buf(1, C.c_uint8))
    a.update(kw)
    p = lambda x: C.cast(x, C.c_void_p) if x is not None else C.c_void_p(0)       # noqa: E731
    return (p(a["origins"]), p(a["dirs"]), p(a["skip"]), a["n"], a["t_min"], a["t_max"], p(a["tri9"]), a["F"], a["origin"], a["cell"], a["dims"],
            p(a["seg"]), p(a["seg_tri"]), a["n_pairs"], p(a["hit"]), p(a["status"]), C.c_void_p(0))


def _mask_args(**kw):
    a = dict(n_lights=1, t_min=0.0, dims=(C.c_int * 3)(1, 1, 1), lit=_buf(4, C.c_uint8), lights=(C.c_float * 20)(*([0.0, 1.0, 0.0, 1.0] * 5)))
    a.update(kw)
    p = lambda x: C.cast(x, C.c_void_p) if x is not None else C.c_void_p(0)       # noqa: E731
    m = (C.c_float * 16)(*np.eye(4).reshape(-1))
    return (p(_buf(9)), p(_buf(6, C.c_int32)), p(_buf(3)), 3, p(_buf(3, C.c_int32)), 1, p(_buf(4, C.c_int32)), 2, 2, m, a["lights"], a["n_lights"],
            a["t_min"], p(_buf(9)), (C.c_float * 3)(0, 0, 0), 1.0, a["dims"], p(_buf(2, C.c_int64)), p(_buf(1, C.c_int32)), 1, p(a["lit"]), C.c_void_p(0))


def test_entry_points_refuse_bad_arguments_before_any_launch():
    lib = _lib.load()
    refused = [("dims below 1", lib.s3d_mesh_ray_occluded, _ray_args(dims=(C.c_int * 3)(1, 0, 1))),
               ("negative t_min", lib.s3d_mesh_ray_occluded, _ray_args(t_min=-1e-3)),
               ("NaN t_min", lib.s3d_mesh_ray_occluded, _ray_args(t_min=math.nan)),
               ("infinite t_min", lib.s3d_mesh_ray_occluded, _ray_args(t_min=math.inf)),
               ("null hit", lib.s3d_mesh_ray_occluded, _ray_args(hit=None)),
               ("null status", lib.s3d_mesh_ray_occluded, _ray_args(status=None)),
               ("five lights", lib.s3d_pbr_shadow_mask, _mask_args(n_lights=_lib.RENDER_MAX_LIGHTS + 1)),
               ("mask dims below 1", lib.s3d_pbr_shadow_mask, _mask_args(dims=(C.c_int * 3)(0, 1, 1))),
               ("mask negative t_min", lib.s3d_pbr_shadow_mask, _mask_args(t_min=-1.0)),
               ("mask NaN t_min", lib.s3d_pbr_shadow_mask, _mask_args(t_min=math.nan)),
               ("null lit", lib.s3d_pbr_shadow_mask, _mask_args(lit=None))]
    for what, fn, args in refused:
        assert fn(*args) == _lib.ERR_INVALID, what
        assert _lib.last_error(), what
    # the shade entry with a mask: the light count is checked as s3d_pbr_shade checks it
    p = lambda x: C.cast(x, C.c_void_p)                          # noqa: E731
    eye, m = (C.c_float * 3)(0, 0, 3), (C.c_float * 16)(*np.eye(4).reshape(-1))
    rc = lib.s3d_pbr_shade_lit(p(_buf(9)), p(_buf(6, C.c_int32)), p(_buf(3)), 3, p(_buf(3, C.c_int32)), 1, p(_buf(4, C.c_int32)), 2, 2, 1, m, None, None,
                               None, None, None, 0, None, 0, None, None, None, None, eye, (C.c_float * 20)(*([0.0, 1.0, 0.0, 1.0] * 5)),
                               _lib.RENDER_MAX_LIGHTS + 1, 0.1, 0, p(_buf(4, C.c_uint8)), p(_buf(16, C.c_uint8)), None)
    assert rc == _lib.ERR_INVALID and "lights" in _lib.last_error()


def test_new_symbols_are_declared_bound_and_exported_under_the_same_abi():
    header = open(os.path.join(REPO, "include", "sin3dm_hip.h")).read()
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert re.search(r"S3D_API int " + name + r"\(", header), name
        assert name in _lib.SIGNATURES and getattr(lib, name) is not None, name
    assert re.search(r"#define S3D_ABI_VERSION (\d+)", header).group(1) == "13" and _lib.ABI_VERSION == 13 == lib.s3d_abi_version()
    # the arithmetic is spelled out where the symbols are declared, and the file is in the build list
    assert "u + v <= det" in header and "t_min <= w / det <= t_max" in header
    assert "s3d_ray.hip" in open(os.path.join(REPO, "sin3dm_amd", "csrc", "Makefile")).read()
    src = open(os.path.join(REPO, "sin3dm_amd", "csrc", "s3d_ray.hip")).read()
    assert '#include "s3d_pbr_shade_body.h"' in src and '#include "s3d_cellgrid.h"' in src
    assert '#include "s3d_pbr_shade_body.h"' in open(os.path.join(REPO, "sin3dm_amd", "csrc", "s3d_render_pbr.hip")).read()


def test_command_lines_and_environment_know_the_option(monkeypatch):
    from sin3dm_amd import sample
    from sin3dm_amd.rendering import render_multiview, render_pbr
    assert render_pbr.build_parser().parse_args(["-s", "x.obj", "--shadows"]).shadows is True
    assert render_pbr.build_parser().parse_args(["-s", "x.obj"]).shadows is False
    assert render_multiview.build_parser().parse_args(["-s", "x.obj", "-o", "d", "--shadows"]).shadows is True
    monkeypatch.delenv("S3D_RENDER_SHADOWS", raising=False)
    assert sample.render_shadows() is False
    monkeypatch.setenv("S3D_RENDER_SHADOWS", "1")
    assert sample.render_shadows() is True
    monkeypatch.setenv("S3D_RENDER_SHADOWS", "yes")
    with pytest.raises(ValueError):
        sample.render_shadows()
