"""GPU: the ray query and the shadows of the PBR renders (s3d_ray.hip, sin3dm_amd/rendering/rasterizer.py) against
the float64 brute force of tests/render_shadow_cases.py.  `hit` and `lit` equal the restatement on every ray that is not near a
tie (at most render_cases.MAX_LEFT_OUT of a case's rays), and on the exact rays in full; the same bytes on every grid, the rays
near a tie included; every pixel of a shadowed image is the pixel of the unshadowed render with the subset of lights its mask byte
names; nothing else moves; the command lines and the sampler hook end to end."""
import ctypes as C
import functools
import math
import os

import numpy as np
import pytest
import torch

import render_cases as R
import render_shadow_cases as S
from sin3dm_amd import _lib
from sin3dm_amd.rendering import camera, rasterizer
from test_render_gpu import _read_png

pytestmark = pytest.mark.gpu
Ws, Hs = S.GRID


def _dev(x, dtype):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=dtype))).cuda()


def _render(c, ss=1, lights=None, **kw):
    return rasterizer.render_views(_dev(c["verts"], np.float32), _dev(c["faces"], np.int32), vertex_colors=_dev(c.get("vertex_colors"), np.float32),
                                   views=[camera.View(c["matrix"], near=c["near"])], resolution=(Ws // ss, Hs // ss), supersample=ss,
                                   lights=c["lights"] if lights is None else lights, **kw)


@functools.lru_cache(maxsize=None)
def device_mask(name, grid=None):
    """(lit uint8 [Hs, Ws], the view's raster buffers as NumPy arrays) of a case at supersample 1 on a grid."""
    _, bufs = _render(S.case(name), shadows=True, shadow_grid=grid, return_buffers=True)
    b = {k: v.cpu().numpy() for k, v in bufs[0].items() if torch.is_tensor(v)}
    return b["lit"], b


@pytest.mark.parametrize("name", list(S.CASES))
def test_mask_equals_the_restatement_outside_the_tie_band(name, record_property):
    c = S.case(name)
    got, b = device_mask(name)
    assert got.dtype == np.uint8 and got.shape == (Hs, Ws)
    want, left = S.restate_mask(c, b["xy_fixed"].astype(np.int64), b["inv_w"].astype(np.float64), b["face_id"])
    covered = b["face_id"] >= 0
    share = float(left[covered].mean()) if covered.any() else 0.0
    record_property("left_out_share", share)
    print(name, "covered", int(covered.sum()), "left out", int(left.sum()), "differing", int((got != want)[~left].sum()))
    assert share <= R.MAX_LEFT_OUT
    assert not got[~covered].any()
    assert np.array_equal(got[~left], want[~left])
    if name in ("f_empty", "f_off"):
        assert not covered.any() and not got.any()
    else:
        assert covered.sum() > 1000 and 0 < (got[covered] & 1).mean() < 1          # the case has light and shadow


def test_no_lights_give_an_empty_mask():
    c = S.case("c_concave")
    images, bufs = _render(c, lights=np.zeros((0, 4)), shadows=True, return_buffers=True)
    assert not bufs[0]["lit"].any() and (bufs[0]["face_id"] >= 0).sum() > 1000
    assert torch.equal(images, _render(c, lights=np.zeros((0, 4))))


def _occluded(mesh, o, d, skip, t_min, t_max, grid):
    hit, status = rasterizer.ray_occluded(_dev(mesh["verts"], np.float32), _dev(mesh["faces"], np.int32), _dev(o, np.float32), _dev(d, np.float32),
                                          _dev(skip, np.int32), t_min, t_max, grid)
    assert hit.dtype == torch.uint8 and status.dtype == torch.uint8
    return hit.cpu().numpy(), status.cpu().numpy()


@pytest.mark.parametrize("dims", S.WALK_GRIDS)
def test_exact_rays_in_full_on_every_grid(dims):
    """Every product of these rays' tests is exact in float32: no tie band, every ray counts — the inclusive edges, corners and
    bounds, the skipped face, the three status values; zero, NaN and infinite rays come back with status 2 and hit 0."""
    g = S.generic()
    bad = []
    for (t_min, t_max) in sorted({(r[3], r[4]) for r in g["rays"]}):
        rays = [r for r in g["rays"] if (r[3], r[4]) == (t_min, t_max)]
        hit, status = _occluded(g, [r[0] for r in rays], [r[1] for r in rays], [r[2] for r in rays], t_min, t_max, dims)
        bad += [(r[7], int(h), int(s)) for r, h, s in zip(rays, hit, status) if (int(h), int(s)) != (r[5], r[6])]
    assert bad == []


@pytest.mark.parametrize("name", [n for n in S.CASES if n != "f_empty"])
def test_random_rays_equal_the_restatement_and_do_not_depend_on_the_grid(name):
    c = S.case(name)
    o, d, skip = S.random_rays(name)
    t_min = S.t_min_of(c)
    want, tie, _ = S.restate(o, d, skip, S.tri9_of(c), t_min, math.inf)
    assert tie.mean() <= R.MAX_LEFT_OUT
    runs = [_occluded(c, o, d, skip, t_min, math.inf, dims) for dims in S.WALK_GRIDS]
    hit, status = runs[-1]
    print(name, "rays", len(o), "hits", int(hit.sum()), "ties", int(tie.sum()), "status 1", int((status == 1).sum()))
    assert np.array_equal(hit[~tie].astype(bool), want[~tie])
    assert not (status == 2).any() and not hit[status != 0].any()
    if name != "f_off":
        assert 0 < hit.mean() < 1
    for other, _ in runs[:-1]:
        assert np.array_equal(other, hit)                                         # bit for bit, the rays near a tie included


def test_empty_mesh_and_no_rays():
    c = S.case("f_empty")
    o, d, skip = S.random_rays("f_off", n=50)
    hit, status = _occluded(c, o, d, skip, 0.0, math.inf, None)
    assert not hit.any() and set(np.unique(status)) <= {0, 1}
    hit, status = _occluded(S.case("a_slab"), np.zeros((0, 3)), np.zeros((0, 3)), None, 0.0, 1.0, None)
    assert hit.shape == status.shape == (0,)


@pytest.mark.parametrize("name", [n for n in S.CASES])
def test_mask_is_the_same_on_every_grid(name):
    ref, _ = device_mask(name)
    for dims in S.WALK_GRIDS[:-1]:
        got, _ = device_mask(name, dims)
        assert np.array_equal(got, ref), (name, dims, int((got != ref).sum()))


@pytest.mark.parametrize("name", S.IMAGE_CASES)
def test_every_pixel_is_the_subset_render_its_mask_byte_names(name):
    c = S.case(name)
    lights = np.asarray(c["lights"])
    assert len(lights) == 3
    for passes in ("shaded", "geo"):
        shadowed, bufs = _render(c, shadows=True, passes=passes, return_buffers=True)
        lit = bufs[0]["lit"].cpu().numpy()
        shadowed = shadowed.cpu().numpy()[0]
        subsets = [_render(c, lights=lights[[k for k in range(3) if m >> k & 1]].reshape(-1, 4), passes=passes).cpu().numpy()[0] for m in range(8)]
        want = np.zeros_like(shadowed)
        for m in range(8):
            want[lit == m] = subsets[m][lit == m]
        assert len(np.unique(lit)) >= 4 and np.array_equal(shadowed, want), (name, passes, int((shadowed != want).any(-1).sum()))
        # supersample 2: the covered share does not change, and a shadow only darkens
        a, b = _render(c, ss=2, shadows=True, passes=passes).cpu().numpy(), _render(c, ss=2, passes=passes).cpu().numpy()
        assert np.array_equal(a[..., 3], b[..., 3]) and (a[..., :3] <= b[..., :3]).all()
        assert (a[..., :3] < b[..., :3]).any() == (name != "b_convex")                # (a convex body casts no shadow on itself)


def test_nothing_else_moves():
    c = S.case("c_concave")
    for shading in ("flat", "smooth", "pbr"):
        kw = {} if shading == "flat" else {"shading": shading}
        plain = rasterizer.render_views(_dev(c["verts"], np.float32), _dev(c["faces"], np.int32), vertex_colors=_dev(c["vertex_colors"], np.float32),
                                        views=[camera.View(c["matrix"], near=c["near"])], resolution=(Ws, Hs), supersample=1, **kw)
        off = rasterizer.render_views(_dev(c["verts"], np.float32), _dev(c["faces"], np.int32), vertex_colors=_dev(c["vertex_colors"], np.float32),
                                      views=[camera.View(c["matrix"], near=c["near"])], resolution=(Ws, Hs), supersample=1, shadows=False, **kw)
        assert torch.equal(plain, off), shading
    unlit = ("albedo", "metallic", "roughness", "normal")
    a, b = _render(c, passes=unlit + ("shaded",), shading="smooth"), _render(c, passes=unlit + ("shaded",), shading="smooth", shadows=True)
    for p in unlit:
        assert torch.equal(a[p], b[p]), p
    assert not torch.equal(a["shaded"], b["shaded"])
    again = _render(c, passes=unlit + ("shaded",), shading="smooth", shadows=True)
    assert all(torch.equal(again[p], b[p]) for p in b)                             # same input, same bytes
    m1, _ = device_mask("c_concave")
    device_mask.cache_clear()
    assert np.array_equal(device_mask("c_concave")[0], m1)


def test_shade_entry_without_a_mask_is_the_shade_entry():
    c = S.case("b_convex")
    lib = _lib.load()
    v, t, col = _dev(c["verts"], np.float32), _dev(c["faces"], np.int32), _dev(c["vertex_colors"], np.float32)
    xy, iw = rasterizer.project(v, c["matrix"], Ws, Hs, c["near"])
    r = rasterizer.rasterize(xy, iw, t, Ws, Hs)
    lights = np.asarray(c["lights"], dtype=np.float64)
    light_arr = (C.c_float * 12)(*[float(x) for x in lights.reshape(-1)])
    eye = rasterizer._f3(rasterizer.eye_of(c["matrix"]))
    head = (_lib.ptr(v), _lib.ptr(xy), _lib.ptr(iw), v.shape[0], _lib.ptr(t), t.shape[0], _lib.ptr(r["face_id"]), Ws, Hs, 1, rasterizer._f16(c["matrix"]),
            _lib.ptr(col), None, None, None, None, 0, None, 0, None, None, None, None, eye, light_arr, 3, 0.1, 0)
    out = [torch.zeros((Hs, Ws, 4), device="cuda", dtype=torch.uint8) for _ in range(3)]
    full = torch.full((Hs, Ws), 7, device="cuda", dtype=torch.uint8)
    _lib.check(lib.s3d_pbr_shade(*head, _lib.ptr(out[0]), _lib.stream_ptr()))
    _lib.check(lib.s3d_pbr_shade_lit(*head, None, _lib.ptr(out[1]), _lib.stream_ptr()))
    _lib.check(lib.s3d_pbr_shade_lit(*head, _lib.ptr(full), _lib.ptr(out[2]), _lib.stream_ptr()))
    torch.cuda.synchronize()
    assert out[0][..., 3].any() and torch.equal(out[0], out[1]) and torch.equal(out[0], out[2])     # (every bit set: every light, in order)


def test_command_lines_and_sampler_hook(tmp_path, monkeypatch):
    from sin3dm_amd import sample
    from sin3dm_amd.encoding.isosurface import export_obj
    from sin3dm_amd.rendering import render_multiview, render_pbr
    c = S.case("c_concave")
    obj = str(tmp_path / "m" / "object.obj")
    export_obj(obj, torch.from_numpy(c["verts"]), torch.from_numpy(c["faces"]), torch.from_numpy(c["vertex_colors"]))
    size = ["--image_resolution", "48", "40"]
    plain = render_pbr.main(["-s", obj, "-o", str(tmp_path / "plain.png"), *size])
    shadowed = render_pbr.main(["-s", obj, "-o", str(tmp_path / "shadowed.png"), *size, "--shadows"])
    assert [os.path.basename(p) for p in shadowed] == ["shadowed.png", "shadowed_albedo.png", "shadowed_geo.png"]
    for k, same in enumerate((False, True, False)):                                   # shaded and geo darken, the albedo pass does not move
        a, b = _read_png(plain[k]), _read_png(shadowed[k])
        assert a.shape == (40, 48, 4) and np.array_equal(a[..., 3], b[..., 3]) and (b[..., :3] <= a[..., :3]).all()
        assert np.array_equal(a, b) == same, shadowed[k]
    a = render_multiview.main(["-s", obj, "-o", str(tmp_path / "mv"), *size, "--shading", "smooth"])
    b = render_multiview.main(["-s", obj, "-o", str(tmp_path / "mv_shadows"), *size, "--shading", "smooth", "--shadows"])
    assert len(a) == len(b) == 8
    assert all((_read_png(q)[..., :3] <= _read_png(p)[..., :3]).all() for p, q in zip(a, b)) and any(not np.array_equal(_read_png(p), _read_png(q)) for p, q in zip(a, b))
    flat = render_multiview.main(["-s", obj, "-o", str(tmp_path / "mv_flat_shadows"), *size, "--shadows"])
    assert len(flat) == 8 and _read_png(flat[0])[..., 3].max() == 255
    # the sampler hook: S3D_RENDER_SHADOWS=1 reaches render_views, unset it does not
    seen = []
    real = rasterizer.render_views
    monkeypatch.setattr(rasterizer, "render_views", lambda *a, **kw: (seen.append(kw), real(*a, **kw))[1])
    mesh = (torch.from_numpy(c["verts"]).cuda(), torch.from_numpy(c["faces"]).cuda(), torch.from_numpy(c["vertex_colors"]).cuda())
    monkeypatch.delenv("S3D_RENDER_SHADOWS", raising=False)
    monkeypatch.delenv("S3D_RENDER_SHADING", raising=False)
    p0 = sample.render_sample(str(tmp_path / "000"), mesh)
    monkeypatch.setenv("S3D_RENDER_SHADOWS", "1")
    p1 = sample.render_sample(str(tmp_path / "001"), mesh)
    assert "shadows" not in seen[0] and seen[1]["shadows"] is True and len(p0) == len(p1) == 8
    assert not np.array_equal(_read_png(p0[0]), _read_png(p1[0]))
