"""GPU: the PBR renders (s3d_render_pbr.hip, sin3dm_amd/rendering) against the restatement of tests/render_pbr_cases.py.
Vertex normals and face tangents against float64 within ten times the measured float32 gap.  Images of every case, view and pass
within max(1, 2 * the measured float32 gap) levels on the pixels whose samples all agree in face_id and hold no sample the
restatement flags as ill-conditioned (at most render_cases.MAX_LEFT_OUT of a case's covered samples).  The light model's float
value through the gain ladder of render_pbr_cases.py: the same views under light intensities times 2^0 ... 2^24, every
pixel-channel read at the largest gain that does not clip, within LADDER_BOUND levels of a level in [128, 255).  Same input, same bits; the
default call is the flat shader's call, byte for byte; the command line and the sampler hook end to end."""
import functools
import os

import numpy as np
import pytest
import torch

import render_cases as R
import render_pbr_cases as P
from sin3dm_amd import _lib
from sin3dm_amd.rendering import camera, rasterizer
from test_render_gpu import _read_png

pytestmark = pytest.mark.gpu
NAMES_GRIDS = [(n, g) for n in P.CASES for g in P.GRIDS]


def _dev(x, dtype):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=dtype))).cuda()


def _views(c):
    return [camera.View(m, near=c["near"]) for m in c["matrices"]]


def _render(c, views, W, H, ss, passes=P.PASSES, **kw):
    return rasterizer.render_views(_dev(c["verts"], np.float32), _dev(c["faces"], np.int32), uvs=_dev(c.get("uvs"), np.float32),
                                   face_mat=_dev(c.get("face_mat"), np.int32), materials=c.get("materials"),
                                   vertex_colors=_dev(c.get("vertex_colors"), np.float32), views=views, resolution=(W, H), supersample=ss,
                                   shading=c["shading"], passes=passes, lights=c["lights"], ambient=c.get("ambient"), **kw)


@functools.lru_cache(maxsize=None)
def device_run(name, grid):
    """Every view and pass of a case in one call: ({pass: uint8 [n_views, H, W, 4]}, per view the buffers as NumPy arrays)."""
    c = P.case(name, grid)
    Ws, Hs, ss = P.GRIDS[grid]
    images, bufs = _render(c, _views(c), Ws // ss, Hs // ss, ss, return_buffers=True)
    return {p: v.cpu().numpy() for p, v in images.items()}, [{k: v.cpu().numpy() for k, v in b.items() if torch.is_tensor(v)} for b in bufs]


@pytest.mark.parametrize("name", list(P.CASES))
def test_vertex_normals_and_tangents_against_float64(name, record_property):
    c = P.case(name, "g64")
    got = rasterizer.vertex_normals(_dev(c["verts"], np.float32), _dev(c["faces"], np.int32)).cpu().numpy()
    want = P.vertex_normals(c["verts"], c["faces"])
    assert got.dtype == np.float32 and got.shape == want.shape
    gap = P.relative_gap(got, want)                               # (asserts the zero normals to be exactly zero)
    record_property("normal_relative_error", gap)
    print(name, "normals: largest relative error", gap, "bound", P.NORMAL_BOUND)
    assert gap <= P.NORMAL_BOUND
    if "zero_normals" in c:
        assert not got[c["zero_normals"]].any()
    if c.get("uvs") is not None:
        got = rasterizer.face_tangents(_dev(c["verts"], np.float32), _dev(c["faces"], np.int32), _dev(c["uvs"], np.float32)).cpu().numpy()
        want = P.face_tangents(c["verts"], c["faces"], c["uvs"])
        assert got.dtype == np.float32 and got.shape == want.shape == (len(c["faces"]), 2, 3)
        gap = P.relative_gap(got, want)
        record_property("tangent_relative_error", gap)
        print(name, "tangents: largest relative error", gap, "bound", P.TANGENT_BOUND)
        assert gap <= P.TANGENT_BOUND
        assert np.array_equal(got.any((1, 2)), want.any((1, 2)))


@pytest.mark.parametrize("name,grid", NAMES_GRIDS)
def test_images_of_every_view_and_pass(name, grid, record_property):
    c = P.case(name, grid)
    Ws, Hs, ss = P.GRIDS[grid]
    images, bufs = device_run(name, grid)
    worst = {p: 0 for p in P.PASSES}
    for k, b in enumerate(bufs):
        xy, iw = b["xy_fixed"].astype(np.int64), b["inv_w"].astype(np.float64)
        r = R.raster(xy, iw, c["faces"], Ws, Hs)
        want, flagged = P.shade_pbr(c, c["matrices"][k], P.gather_samples(c, xy, iw, r["face_id"]), Ws, Hs, ss)
        covered = r["face_id"] >= 0
        assert flagged.sum() <= R.MAX_LEFT_OUT * covered.sum(), (name, grid, k, int(flagged.sum()))
        per_pixel = lambda a: a.reshape(Hs // ss, ss, Ws // ss, ss)          # noqa: E731
        keep = per_pixel(b["face_id"] == r["face_id"]).all((1, 3)) & ~per_pixel(flagged).any((1, 3))
        assert keep.mean() >= 1 - 4 * R.MAX_LEFT_OUT
        for p in P.PASSES:
            got = images[p][k]
            assert got.shape == want[p].shape == (Hs // ss, Ws // ss, 4) and got.dtype == np.uint8
            diff = int(np.abs(got.astype(np.int64) - want[p])[keep].max(initial=0))
            worst[p] = max(worst[p], diff)
            print(name, grid, "view", k, p, "pixels compared", int(keep.sum()), "largest difference", diff, "levels; bound", P.IMAGE_BOUND[p])
            assert np.array_equal(got[..., 3] > 0, per_pixel(covered).any((1, 3)))
    for p in P.PASSES:
        record_property("levels_" + p, worst[p])
    assert all(worst[p] <= P.IMAGE_BOUND[p] for p in P.PASSES), worst


# ------------------------------------------------------------------ the light model through the gain ladder
def _ladder_render(name):
    """One render_views call per gain, each with every view of the case and the passes shaded and geo:
    ({pass: uint8 [G, n_views, H, W, 4]}, per view the buffers of the first call; the projection does not depend on the lights)."""
    c = P.ladder_case(name)
    Ws, Hs, ss = P.GRIDS[c["grid"]]
    views, lights = _views(c), np.asarray(c["lights"], dtype=np.float64)
    out, bufs = {p: [] for p in P.LADDER_PASSES}, None
    for g in P.LADDER_GAINS:
        scaled = dict(c, lights=lights * np.array([1.0, 1.0, 1.0, g]))           # a power of two: exact, in float64 and in float32
        res = _render(scaled, views, Ws // ss, Hs // ss, ss, passes=P.LADDER_PASSES, return_buffers=bufs is None)
        if bufs is None:
            res, first = res
            bufs = [{k: v.cpu().numpy() for k, v in b.items() if torch.is_tensor(v)} for b in first]
        for p in P.LADDER_PASSES:
            out[p].append(res[p].cpu().numpy())
    return {p: np.stack(v) for p, v in out.items()}, bufs


ladder_run = functools.lru_cache(maxsize=None)(_ladder_render)


@pytest.mark.parametrize("name", list(P.LADDER_CASES))
def test_light_model_through_the_gain_ladder(name, record_property):
    """Every pixel-channel of shaded and geo at the largest gain at which the float64 restatement does not clip (a level in
    [128, 255), so the difference is relative) within LADDER_BOUND levels, on the device's own projection."""
    c = P.ladder_case(name)
    Ws, Hs, ss = P.GRIDS[c["grid"]]
    levels, bufs = ladder_run(name)
    worst, share, own_share = {p: 0 for p in P.LADDER_PASSES}, {p: 1.0 for p in P.LADDER_PASSES}, {p: 1.0 for p in P.LADDER_PASSES}
    for k, b in enumerate(bufs):
        ref = P.ladder_reference(name, k, xy=b["xy_fixed"].astype(np.int64), iw=b["inv_w"].astype(np.float64))
        assert ref["n_flagged"] <= R.MAX_LEFT_OUT * ref["n_covered"], (name, k, ref["n_flagged"])
        agree = (b["face_id"] == ref["raster"]["face_id"]).reshape(Hs // ss, ss, Ws // ss, ss).all((1, 3))
        assert (agree & ~ref["left_out"]).mean() >= 1 - 4 * R.MAX_LEFT_OUT
        got = {p: levels[p][:, k, :, :, :3] for p in P.LADDER_PASSES}
        assert all(got[p].shape == ref["levels"][p].shape and got[p].dtype == np.uint8 for p in got)
        res = P.ladder_compare(got, ref, agree)
        for p in P.LADDER_PASSES:
            assert np.array_equal(levels[p][0, k, :, :, 3] > 0, ref["covered"])
            own = float(P.ladder_readout(got[p], got[p])[2][ref["covered"]].mean())          # what the device's own images let one read
            worst[p], share[p], own_share[p] = max(worst[p], res[p][0]), min(share[p], res[p][1]), min(own_share[p], own)
            print(name, "view", k, p, "largest difference", res[p][0], "levels; bound", P.LADDER_BOUND[p], "; read share", round(res[p][1], 4),
                  "the device's own", round(own, 4), "; gains 2^%d to 2^%d" % (res[p][2].min(), res[p][2].max()))
    for p in P.LADDER_PASSES:
        record_property("ladder_levels_" + p, worst[p])
        record_property("ladder_read_share_" + p, share[p])
    assert all(share[p] >= 0.95 and own_share[p] >= 0.95 for p in P.LADDER_PASSES), (share, own_share)
    assert all(worst[p] <= P.LADDER_BOUND[p] for p in P.LADDER_PASSES), worst


def test_ladder_gain_changes_nothing_but_the_intensity():
    """level = floor(255 g x + 0.5): doubling g doubles the level to within 1 wherever the higher gain does not clip; and the
    same ladder twice gives the same bits."""
    levels, _ = ladder_run("m1_near_mirror")
    pairs = 0
    for p in P.LADDER_PASSES:
        lev = levels[p][..., :3].astype(np.int64)
        both = lev[1:] < 255
        pairs += int((both & (lev[:-1] > 0)).sum())
        assert np.abs(lev[1:] - 2 * lev[:-1])[both].max() <= 1, p
        assert np.array_equal(levels[p][1:, ..., 3], levels[p][:-1, ..., 3])
    assert pairs > 20000
    again, _ = _ladder_render("m1_near_mirror")
    assert all(np.array_equal(again[p], levels[p]) for p in P.LADDER_PASSES)


def test_same_input_same_bits_and_views_and_passes_separately():
    c = P.case("a_sphere", "g64")
    views = _views(c)
    one = _render(c, views, 32, 24, 2, return_buffers=True)
    two = _render(c, views, 32, 24, 2, return_buffers=True)
    assert sorted(one[0]) == sorted(P.PASSES) and one[0]["shaded"].shape == (8, 24, 32, 4)
    for p in P.PASSES:
        assert torch.equal(one[0][p], two[0][p]), p
    for k, view in enumerate(views):                               # eight calls with one view each
        alone = _render(c, [view], 32, 24, 2, passes=("shaded", "normal"))
        assert torch.equal(alone["shaded"][0], one[0]["shaded"][k]) and torch.equal(alone["normal"][0], one[0]["normal"][k]), k
    assert len({one[0]["shaded"][k].cpu().numpy().tobytes() for k in range(8)}) == 8
    m = P.case("b_quads", "g64")
    both = _render(m, _views(m), 32, 24, 2, passes=("shaded", "metallic"))
    for p in ("shaded", "metallic"):                               # passes=(a, b) equals two single-pass calls
        single = _render(m, _views(m), 32, 24, 2, passes=(p,))
        assert torch.is_tensor(single) and torch.equal(single, both[p]), p
    n1 = rasterizer.vertex_normals(_dev(c["verts"], np.float32), _dev(c["faces"], np.int32))
    n2 = rasterizer.vertex_normals(_dev(c["verts"], np.float32), _dev(c["faces"], np.int32))
    assert torch.equal(n1, n2)


def test_pbr_without_materials_keeps_the_vertex_colours():
    """A vertex-coloured mesh under shading="pbr" (what S3D_RENDER_SHADING=pbr meets in the sampler's default export mode, and
    render_multiview --shading pbr on a vertex-coloured OBJ): the colours are the albedo, so the render is the smooth one."""
    c = P.case("a_sphere", "g64")
    views = _views(c)[:2]
    smooth = _render(c, views, 32, 24, 2, passes=("shaded", "albedo"))
    for shading, other in (("pbr", smooth), ("pbr_flat", _render(dict(c, shading="flat"), views, 32, 24, 2, passes=("shaded", "albedo")))):
        got = _render(dict(c, shading=shading), views, 32, 24, 2, passes=("shaded", "albedo"))
        for p in ("shaded", "albedo"):
            assert torch.equal(got[p], other[p]), (shading, p)
    solid = smooth["albedo"][..., 3] == 255
    rgb = smooth["albedo"][solid][:, :3].float()
    assert int(solid.sum()) > 100 and float(rgb.std(0).min()) > 10 and float(rgb.min()) < 200          # coloured, not white
    # materials come before vertex colours under pbr
    both = rasterizer.render_views(_dev(c["verts"], np.float32), _dev(c["faces"], np.int32), vertex_colors=_dev(c["vertex_colors"], np.float32),
                                   materials=[{"Kd": (0.25, 0.5, 0.75)}], views=views, resolution=(32, 24), shading="pbr", passes=("albedo",),
                                   lights=c["lights"])
    assert both[both[..., 3] == 255][:, :3].cpu().unique(dim=0).tolist() == [[64, 128, 191]]


@pytest.mark.parametrize("name", ["b_sphere", "i_textured", "a_fan"])
def test_default_call_is_the_flat_shader_byte_for_byte(name):
    """render_views without the new arguments against the same stages driven here through the entry points the flat path has
    always used (project, rasterize, s3d_render_shade)."""
    import ctypes as C
    c = R.case(name, "g64")
    Ws, Hs, ss = R.GRIDS["g64"]
    v, t = _dev(c["verts"], np.float32), _dev(c["faces"], np.int32)
    view = camera.View(c["matrix"], c["light"], c["near"])
    kw = dict(uvs=_dev(c.get("uvs"), np.float32), face_mat=_dev(c.get("face_mat"), np.int32), materials=c.get("materials"),
              vertex_colors=_dev(c.get("vertex_colors"), np.float32))
    got = rasterizer.render_views(v, t, views=[view], resolution=(Ws // ss, Hs // ss), supersample=ss, **kw)
    explicit = rasterizer.render_views(v, t, views=[view], resolution=(Ws // ss, Hs // ss), supersample=ss, shading="flat", passes=("shaded",),
                                       lights=None, ambient=None, **kw)
    xy, iw = rasterizer.project(v, view.matrix, Ws, Hs, view.near)
    r = rasterizer.rasterize(xy, iw, t, Ws, Hs)
    vcol = kw["vertex_colors"]
    table = kd = images = None
    n_mats = nbytes = 0
    if vcol is None and c.get("materials"):
        table, kd, images, nbytes = rasterizer.pack_materials(c["materials"], v.device)
        n_mats = table.shape[0]
    out = torch.empty((Hs // ss, Ws // ss, 4), device=v.device, dtype=torch.uint8)
    _lib.check(_lib.load().s3d_render_shade(_lib.ptr(v), _lib.ptr(xy), _lib.ptr(iw), v.shape[0], _lib.ptr(t), t.shape[0], _lib.ptr(r["face_id"]), Ws, Hs,
                                            ss, rasterizer._f16(view.matrix), rasterizer._f3(view.light), _lib.ptr(vcol),
                                            _lib.ptr(kw["uvs"]) if n_mats else None, _lib.ptr(kw["face_mat"]) if n_mats else None, _lib.ptr(table),
                                            _lib.ptr(kd), n_mats, _lib.ptr(images) if nbytes else C.c_void_p(0), nbytes, _lib.ptr(out),
                                            _lib.stream_ptr()))
    torch.cuda.synchronize()
    assert int((out[..., 3] > 0).sum()) > 100
    assert torch.equal(got[0], out) and torch.equal(explicit[0], out)
    want, _ = R.shade(c, xy.cpu().numpy().astype(np.int64), iw.cpu().numpy().astype(np.float64), r["face_id"].cpu().numpy(), Ws, Hs, ss)
    assert np.abs(out.cpu().numpy().astype(np.int64) - want).max() <= 1


def _pbr_asset(path, metallic_level=180):
    """An export_pbr_obj asset: an icosphere with a spherical uv map, 16 x 16 maps, constant metallic."""
    from sin3dm_amd.encoding.isosurface import export_pbr_obj
    v, f = R.icosphere(1)
    verts = torch.from_numpy((v * [0.3, 0.5, 0.4] + [1.0, 2.0, 3.0]).astype(np.float32))
    corners = v[f.reshape(-1)]
    uvs = torch.from_numpy(np.stack([np.arctan2(corners[:, 1], corners[:, 0]) / (2 * np.pi) + 0.5, corners[:, 2] * 0.5 + 0.5], 1).astype(np.float32))
    albedo = np.zeros((16, 16, 3), dtype=np.uint8)
    albedo[..., 0], albedo[..., 1], albedo[..., 2] = np.arange(16)[None, :] * 16, np.arange(16)[:, None] * 16, 200
    normal = np.zeros((16, 16, 3), dtype=np.uint8)
    normal[..., :2], normal[..., 2] = 128, 255
    export_pbr_obj(path, verts, torch.from_numpy(f), uvs, albedo, np.full((16, 16), metallic_level, dtype=np.uint8),
                   (np.arange(256).reshape(16, 16) // 2 + 60).astype(np.uint8), normal)


def test_pbr_command_line_end_to_end(tmp_path):
    from sin3dm_amd.rendering import render_pbr
    from sin3dm_amd.rendering.render_multiview import main as rm_main
    _pbr_asset(str(tmp_path / "object.obj"))
    paths = render_pbr.main(["-s", str(tmp_path / "object.obj"), "-o", str(tmp_path / "out" / "view.png"), "--image_resolution", "48", "40"])
    assert [os.path.basename(p) for p in paths] == ["view.png", "view_albedo.png", "view_metallic.png", "view_roughness.png", "view_normal.png",
                                                    "view_geo.png"]
    ims = {os.path.basename(p)[4:-4].lstrip("_") or "shaded": _read_png(p) for p in paths}
    for name, im in ims.items():
        assert im.shape == (40, 48, 4) and im[..., 3].max() == 255 and im[0, 0, 3] == 0 and (im[..., 3] == 255).sum() > 200, name
    solid = ims["shaded"][..., 3] == 255
    # constant metallic 180: a bilinear mix of equal texels is that texel, up to the rounding of the mean: half a level
    assert np.abs(ims["metallic"][solid][:, :3].astype(np.float64) - 180).max() <= 0.5
    assert ims["geo"][solid][:, :3].std(1).max() == 0 and ims["shaded"][solid][:, :3].std(0).min() > 3
    flat = render_pbr.main(["-s", str(tmp_path / "object.obj"), "-o", str(tmp_path / "flat.png"), "--image_resolution", "48", "40", "--shading", "flat",
                            "-az", "200", "-el", "70", "--rot", "20"])
    assert len(flat) == 6 and not np.array_equal(_read_png(flat[4]), ims["normal"])
    # a vertex-coloured OBJ: its colours are the albedo, under the PBR command line and under render_multiview --shading pbr
    from sin3dm_amd.encoding.isosurface import export_obj
    v, f = R.icosphere(1)
    export_obj(str(tmp_path / "col" / "object.obj"), torch.from_numpy(v.astype(np.float32)), torch.from_numpy(f), torch.from_numpy((0.5 + 0.5 * v).astype(np.float32)))
    col = render_pbr.main(["-s", str(tmp_path / "col" / "object.obj"), "--image_resolution", "48", "40"])
    assert [os.path.basename(p) for p in col] == ["object.png", "object_albedo.png", "object_geo.png"]
    for path in (col[1], rm_main(["-s", str(tmp_path / "col" / "object.obj"), "-o", str(tmp_path / "col" / "mv"), "--image_resolution", "48", "40",
                                  "--shading", "pbr"])[0]):
        im = _read_png(path)
        rgb = im[im[..., 3] == 255][:, :3].astype(np.float64)
        assert len(rgb) > 200 and rgb.std(0).min() > 10, path                                       # coloured, not one white or grey
    # the multi-view script with the same materials: eight views, the PBR look differs from the flat default
    from sin3dm_amd.rendering import render_multiview as rm
    a = rm.main(["-s", str(tmp_path / "object.obj"), "-o", str(tmp_path / "mv_flat"), "--image_resolution", "48", "40"])
    b = rm.main(["-s", str(tmp_path / "object.obj"), "-o", str(tmp_path / "mv_pbr"), "--image_resolution", "48", "40", "--shading", "pbr"])
    assert len(a) == len(b) == 8 and not np.array_equal(_read_png(a[0])[..., :3], _read_png(b[0])[..., :3])
    assert np.array_equal(_read_png(a[0])[..., 3], _read_png(b[0])[..., 3])


def test_sampler_hook_renders_pbr_from_device_arrays(tmp_path, monkeypatch):
    from sin3dm_amd import sample
    v, f = R.icosphere(1)
    verts, tris = torch.from_numpy(v.astype(np.float32)).cuda(), torch.from_numpy(f).cuda()
    corners = v[f.reshape(-1)]
    uvs = torch.from_numpy(np.stack([np.arctan2(corners[:, 1], corners[:, 0]) / (2 * np.pi) + 0.5, corners[:, 2] * 0.5 + 0.5], 1).astype(np.float32)).cuda()
    image = torch.zeros((32, 32, 8), dtype=torch.uint8)
    image[..., :3], image[..., 3], image[..., 4], image[..., 5:7], image[..., 7] = 200, 30, 128, 128, 255
    mesh = {"verts": verts, "tris": tris, "uvs": uvs, "image": image.cuda()}
    monkeypatch.delenv("S3D_RENDER_SHADING", raising=False)
    plain = sample.render_sample(str(tmp_path / "000"), mesh)
    monkeypatch.setenv("S3D_RENDER_SHADING", "pbr")
    paths = sample.render_sample(str(tmp_path / "001"), mesh)
    assert [os.path.relpath(p, tmp_path) for p in paths] == [os.path.join("001", "renderings", f"{i:03d}.png") for i in range(8)]
    a, b = _read_png(plain[0]), _read_png(paths[0])
    assert a.shape == b.shape == (512, 512, 4) and np.array_equal(a[..., 3], b[..., 3]) and not np.array_equal(a[..., :3], b[..., :3])
    assert b[..., 3].max() == 255 and b[b[..., 3] == 255][:, :3].max() > 60
    cols = torch.from_numpy((0.5 + 0.5 * v).astype(np.float32)).cuda()
    pbr_cols = sample.render_sample(str(tmp_path / "002"), (verts, tris, cols))           # still "pbr": the default export mode's arrays
    monkeypatch.setenv("S3D_RENDER_SHADING", "smooth")
    smooth_cols = sample.render_sample(str(tmp_path / "004"), (verts, tris, cols))
    assert len(pbr_cols) == len(smooth_cols) == 8
    a, b = _read_png(pbr_cols[0]), _read_png(smooth_cols[0])
    assert np.array_equal(a, b) and a[a[..., 3] == 255][:, :3].astype(np.float64).std(0).min() > 10
    monkeypatch.setenv("S3D_RENDER_SHADING", "phong")
    with pytest.raises(ValueError):
        sample.render_sample(str(tmp_path / "003"), mesh)
