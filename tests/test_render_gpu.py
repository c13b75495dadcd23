"""GPU: the mesh rasteriser (s3d_render.hip, sin3dm_amd/rendering) against the restatement of tests/render_cases.py.
Raster stage, on the device's own snapped coordinates: the count buffer equals the integer restatement on every sample of every
case; face_id equals it wherever the two nearest covering triangles are further apart than the measured depth band (at most 0.5 %
of a case's covered samples left out, none for the duplicated faces).  Projection: within one unit of the float64 rounding.
Images: within one level wherever face_id agrees on all samples of a pixel.  Same input, same bits."""
import functools
import os
import struct
import zlib

import numpy as np
import pytest
import torch

import render_cases as R
from sin3dm_amd.rendering import camera, rasterizer

pytestmark = pytest.mark.gpu
ALL = [(n, g) for n in R.CASES for g in R.GRIDS]


def _dev(x, dtype):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=dtype))).cuda()


def _render(c, views, W, H, ss, **kw):
    return rasterizer.render_views(_dev(c["verts"], np.float32), _dev(c["faces"], np.int32), uvs=_dev(c.get("uvs"), np.float32),
                                   face_mat=_dev(c.get("face_mat"), np.int32), materials=c.get("materials"),
                                   vertex_colors=_dev(c.get("vertex_colors"), np.float32), views=views, resolution=(W, H), supersample=ss, **kw)


@functools.lru_cache(maxsize=None)
def device_run(name, grid):
    """One render of a case: (rgba uint8 [H, W, 4], buffers of the view as NumPy arrays, info)."""
    c = R.case(name, grid)
    Ws, Hs, ss = R.GRIDS[grid]
    rgba, bufs = _render(c, [camera.View(c["matrix"], c["light"], c["near"])], Ws // ss, Hs // ss, ss, return_buffers=True)
    b = {k: v.cpu().numpy() for k, v in bufs[0].items() if torch.is_tensor(v)}
    return rgba[0].cpu().numpy(), b, bufs[0]["info"]


@functools.lru_cache(maxsize=None)
def restated_on_device_coordinates(name, grid):
    c = R.case(name, grid)
    Ws, Hs, _ = R.GRIDS[grid]
    _, b, _ = device_run(name, grid)
    return R.raster(b["xy_fixed"].astype(np.int64), b["inv_w"].astype(np.float64), c["faces"], Ws, Hs)


@pytest.mark.parametrize("name,grid", ALL)
def test_projection_is_within_one_unit(name, grid):
    c = R.case(name, grid)
    Ws, Hs, _ = R.GRIDS[grid]
    _, b, _ = device_run(name, grid)
    xy, iw = R.project(c["verts"], c["matrix"], Ws, Hs, c["near"])
    assert b["xy_fixed"].dtype == np.int32 and b["xy_fixed"].shape == xy.shape and b["inv_w"].dtype == np.float32
    assert np.array_equal(b["inv_w"] == 0, iw == 0)                                  # the same vertices are flagged
    seen = iw > 0
    assert np.abs(xy[seen]).max(initial=0) < R.MAX_COORD                             # where float32 carries more than a unit
    err = np.abs(b["xy_fixed"].astype(np.int64) - xy)[seen]
    print(name, grid, "largest snapping difference", err.max(initial=0), "units of 1/256 sample")
    assert err.max(initial=0) <= 1
    assert np.allclose(b["inv_w"][seen], iw[seen], rtol=1e-6, atol=0)


@pytest.mark.parametrize("name,grid", ALL)
def test_raster_stage_against_the_integer_restatement(name, grid):
    _, b, info = device_run(name, grid)
    r = restated_on_device_coordinates(name, grid)
    assert b["count"].dtype == np.uint8 and b["face_id"].dtype == np.int32 and b["depth"].dtype == np.float32
    assert np.array_equal(b["count"], np.minimum(r["count"], 255)), (name, grid, int((b["count"] != np.minimum(r["count"], 255)).sum()))
    covered = r["count"] > 0
    assert np.array_equal(b["face_id"] >= 0, covered)
    clear = ~r["unclear"]
    left = int(r["unclear"].sum())
    print(name, grid, "covered", int(covered.sum()), "left out of the face_id comparison", left, "differing inside it",
          int((b["face_id"] != r["face_id"])[r["unclear"]].sum()))
    assert left <= R.MAX_LEFT_OUT * covered.sum()
    if name in R.COMPARED_IN_FULL:
        assert left == 0
    assert np.array_equal(b["face_id"][clear], r["face_id"][clear]), (name, grid, int((b["face_id"] != r["face_id"])[clear].sum()))
    same = covered & (b["face_id"] == r["face_id"])
    assert np.all(np.abs(b["depth"][same] - r["depth"][same]) <= R.DEPTH_BAND * r["depth"][same])
    assert not b["depth"][~covered].any()
    assert np.array_equal(b["status"], r["status"])
    st = np.bincount(r["status"], minlength=4)
    assert (info["near"], info["out_of_range"], info["degenerate"], info["dropped"]) == (st[1], st[2], st[3], st[1] + st[2] + st[3])
    if name == "e_crowd":
        assert 4 * 128 < info["longest_tile_list"] == info["n_pairs"] <= st[0]        # one tile, several LDS chunks
    if name == "f_twice":
        assert (b["face_id"][covered] < len(R.case(name, grid)["faces"]) // 2).all()
    if name == "h_behind":
        assert info["near"] == 1 and info["dropped"] == 1
    if name in ("g_off", "g_empty"):
        rgba, _, _ = device_run(name, grid)
        assert not rgba.any() and info["n_pairs"] == 0


@pytest.mark.parametrize("name,grid", ALL)
def test_images_are_within_one_level(name, grid):
    c = R.case(name, grid)
    Ws, Hs, ss = R.GRIDS[grid]
    rgba, b, _ = device_run(name, grid)
    r = restated_on_device_coordinates(name, grid)
    want, _ = R.shade(c, b["xy_fixed"].astype(np.int64), b["inv_w"].astype(np.float64), r["face_id"], Ws, Hs, ss)
    assert rgba.shape == want.shape == (Hs // ss, Ws // ss, 4) and rgba.dtype == np.uint8
    agree = (b["face_id"] == r["face_id"]).reshape(Hs // ss, ss, Ws // ss, ss).all((1, 3))
    diff = np.abs(rgba.astype(np.int64) - want)[agree]
    print(name, grid, "pixels compared", int(agree.sum()), "of", agree.size, "largest difference", diff.max(initial=0), "levels;",
          int((diff > 0).sum()), "channel values differ")
    assert agree.mean() >= 1 - 4 * R.MAX_LEFT_OUT and diff.max(initial=0) <= 1
    assert np.array_equal(rgba[..., 3] > 0, (r["count"] > 0).reshape(Hs // ss, ss, Ws // ss, ss).any((1, 3)))


def test_rasterize_on_given_coordinates():
    """The lower-level entry on the restatement's own snapped coordinates: exact counts, the fan's tiling covered once."""
    for g, (Ws, Hs, _) in R.GRIDS.items():
        c = R.case("a_fan", g)
        xy, iw, r = R.restated("a_fan", g)
        out = rasterizer.rasterize(_dev(xy, np.int32), _dev(iw, np.float32), _dev(c["faces"], np.int32), Ws, Hs)
        assert np.array_equal(out["count"].cpu().numpy(), r["count"]) and out["count"].max() == 1
        assert np.array_equal(out["face_id"].cpu().numpy(), r["face_id"])


def test_same_input_same_bits():
    c = R.case("b_sphere", "g64")
    one = _render(c, None, 32, 24, 2, return_buffers=True)
    two = _render(c, None, 32, 24, 2, return_buffers=True)
    assert one[0].shape == (8, 24, 32, 4) and torch.equal(one[0], two[0])
    for a, b in zip(one[1], two[1]):
        for k in ("face_id", "depth", "count", "xy_fixed", "inv_w"):
            assert torch.equal(a[k], b[k]), k
    v = c["verts"].astype(np.float64)
    views = camera.standard_views(v.min(0), v.max(0), (32, 24))
    for k, view in enumerate(views):                               # eight calls with one view each
        alone = _render(c, [view], 32, 24, 2)
        assert torch.equal(alone[0], one[0][k]), k
        assert int((alone[0][..., 3] > 0).sum()) > 50
    assert len({one[0][k].cpu().numpy().tobytes() for k in range(8)}) == 8           # eight different views


def _read_png(path):
    """uint8 [H, W, C] of an 8-bit PNG whose rows are unfiltered (what isosurface.png_bytes writes)."""
    data = open(path, "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, idat, head = 8, b"", None
    while pos < len(data):
        n, tag = struct.unpack(">I", data[pos:pos + 4])[0], data[pos + 4:pos + 8]
        body = data[pos + 8:pos + 8 + n]
        assert struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])[0] == zlib.crc32(tag + body) & 0xFFFFFFFF
        if tag == b"IHDR":
            head = struct.unpack(">IIBBBBB", body)
        elif tag == b"IDAT":
            idat += body
        pos += 12 + n
    w, h, depth, colour = head[:4]
    ch = {0: 1, 4: 2, 2: 3, 6: 4}[colour]
    rows = np.frombuffer(zlib.decompress(idat), dtype=np.uint8).reshape(h, 1 + w * ch)
    assert depth == 8 and not rows[:, 0].any()
    return rows[:, 1:].reshape(h, w, ch)


def test_command_line_end_to_end(tmp_path):
    from sin3dm_amd.encoding.isosurface import export_obj, export_textured_obj
    from sin3dm_amd.rendering import render_multiview as rm
    v, f = R.icosphere(1)
    verts = torch.from_numpy((v * [0.3, 0.5, 0.4] + [1.0, 2.0, 3.0]).astype(np.float32))
    tris = torch.from_numpy(f)
    corners = v[f.reshape(-1)]
    uvs = torch.from_numpy(np.stack([np.arctan2(corners[:, 1], corners[:, 0]) / (2 * np.pi) + 0.5, corners[:, 2] * 0.5 + 0.5], 1).astype(np.float32))
    image = np.zeros((16, 16, 3), dtype=np.uint8)
    image[..., 0], image[..., 1], image[..., 2] = np.arange(16)[None, :] * 16, np.arange(16)[:, None] * 16, 200
    export_textured_obj(str(tmp_path / "tex" / "object.obj"), verts, tris, uvs, torch.from_numpy(image))
    paths = rm.main(["-s", str(tmp_path / "tex" / "object.obj"), "-o", str(tmp_path / "tex" / "renderings"), "--image_resolution", "48", "40"])
    assert [os.path.basename(p) for p in paths] == [f"{i:03d}.png" for i in range(8)]
    seen = set()
    for p in paths:
        im = _read_png(p)
        assert im.shape == (40, 48, 4) and im[..., 3].max() == 255 and im[0, 0, 3] == 0            # no view is empty; the corner is background
        assert (im[..., 3] == 255).sum() > 200 and im[im[..., 3] == 255][:, 2].mean() > 60         # blue 200 times the shade
        seen.add(im.tobytes())
    assert len(seen) == 8
    # the vertex-coloured OBJ of export_obj, at the default size of the reference's flag
    export_obj(str(tmp_path / "col" / "object.obj"), verts, tris, torch.from_numpy((0.5 + 0.5 * v).astype(np.float32)))
    paths = rm.main(["-s", str(tmp_path / "col" / "object.obj"), "-o", str(tmp_path / "col" / "renderings"), "--supersample", "1"])
    assert len(paths) == 8
    im = _read_png(paths[3])
    solid = im[im[..., 3] == 255][:, :3].astype(np.float64)
    assert im.shape == (512, 512, 4) and len(solid) > 20000 and solid.std(0).min() > 5            # coloured, not one grey


def test_sample_hook_renders_from_device_arrays(tmp_path):
    from sin3dm_amd import sample
    v, f = R.icosphere(1)
    verts, tris = torch.from_numpy(v.astype(np.float32)).cuda(), torch.from_numpy(f).cuda()
    cols = torch.from_numpy((0.5 + 0.5 * v).astype(np.float32)).cuda()
    paths = sample.render_sample(str(tmp_path / "000"), (verts, tris, cols))
    assert [os.path.relpath(p, tmp_path) for p in paths] == [os.path.join("000", "renderings", f"{i:03d}.png") for i in range(8)]
    assert _read_png(paths[0]).shape == (512, 512, 4)
    image = torch.full((32, 32, 3), 128, dtype=torch.uint8).cuda()
    uvs = torch.rand(3 * len(f), 2).cuda()
    paths = sample.render_sample(str(tmp_path / "001"), {"verts": verts, "tris": tris, "uvs": uvs, "image": image})
    im = _read_png(paths[7])
    assert len(paths) == 8 and im[..., 3].max() == 255 and im[..., :3].max() <= 129
    assert sample.render_sample(str(tmp_path / "002"), None) == [] and not os.path.exists(tmp_path / "002")


def test_sampler_writes_renderings_only_when_asked(tmp_path, monkeypatch):
    """S3D_RENDER=views: renderings/ beside the mesh of every sample, vertex-coloured and textured; unset: the same files, the same bits."""
    from test_cli_gpu import make_experiment
    from sin3dm_amd import sample
    from sin3dm_amd.utils import parser_util as pu
    tag = make_experiment(str(tmp_path))
    argv = ["--tag", tag, "--n_samples", "1", "--use_ddim", "True", "--timestep_respacing", "5", "--reso", "48", "--n_faces", "2000", "--texreso", "512"]
    monkeypatch.delenv("S3D_MESH", raising=False)
    monkeypatch.delenv("S3D_RENDER", raising=False)
    plain = os.path.dirname(sample.main(argv + ["--output", "plain"])[0])
    monkeypatch.setenv("S3D_RENDER", "views")
    paths = sample.main(argv + ["--output", "views"])
    views = os.path.dirname(paths[0])
    assert sorted(os.listdir(plain) + ["renderings"]) == sorted(os.listdir(views)) and "object.obj" in os.listdir(plain)
    for name in os.listdir(plain):
        assert open(os.path.join(plain, name), "rb").read() == open(os.path.join(views, name), "rb").read(), name
    assert sorted(os.listdir(os.path.join(views, "renderings"))) == [f"{i:03d}.png" for i in range(8)]
    first = _read_png(os.path.join(views, "renderings", "000.png"))
    assert first.shape == (512, 512, 4) and (first[..., 3] == 255).sum() > 5000
    # the textured export of the same latent, decoded again with the views on
    monkeypatch.setenv("S3D_MESH", "textured")
    os.rename(os.path.join(views, "renderings"), os.path.join(views, "renderings_vertex"))
    sample.decode(pu.sample_args(argv), paths)
    assert {"object.mtl", "object.png", "renderings"} <= set(os.listdir(views))
    tex = _read_png(os.path.join(views, "renderings", "000.png"))
    assert tex.shape == (512, 512, 4) and (tex[..., 3] == 255).sum() > 5000 and tex[..., :3].max() > 40       # drawn, and not black
    monkeypatch.setenv("S3D_RENDER", "blender")
    with pytest.raises(ValueError):
        sample.decode(pu.sample_args(argv), [])
