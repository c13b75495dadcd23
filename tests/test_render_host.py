"""CPU-only: the host half of the mesh rasteriser (sin3dm_amd/rendering, s3d_render.hip).  The restatement of
tests/render_cases.py has the properties the kernels are held to on the GPU (every sample of a tiling covered once, the lower
face on equal depth, the measured depth band), the camera rig is the reference's, and the command line, the OBJ colour reader,
the header, the binding and the argument checks are what the issue asks."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import render_cases as R
from conftest import REPO
from sin3dm_amd import _lib
from sin3dm_amd.rendering import camera

ENTRY_POINTS = ("s3d_render_project", "s3d_render_bin_count", "s3d_render_bin_fill", "s3d_render_raster", "s3d_render_shade")
ALL = [(n, g) for n in R.CASES for g in R.GRIDS]


def test_constants_agree_with_the_header_and_the_kernel():
    header = open(os.path.join(REPO, "include", "sin3dm_hip.h")).read()

    def define(name):
        return re.search(r"#define " + name + r" (.+)", header).group(1).strip()
    assert int(define("S3D_RENDER_TILE")) == R.TILE == _lib.RENDER_TILE
    assert int(define("S3D_RENDER_SUBPIXEL")) == R.SUB == _lib.RENDER_SUBPIXEL and R.HALF * 2 == R.SUB
    assert define("S3D_RENDER_MAX_COORD") == "(1 << 20)" and R.MAX_COORD == _lib.RENDER_MAX_COORD == 1 << 20
    assert define("S3D_RENDER_MAX_PAIRS") == "(1LL << 27)" and _lib.RENDER_MAX_PAIRS == 1 << 27
    assert int(define("S3D_RENDER_MAX_GRID")) == _lib.RENDER_MAX_GRID
    assert float(define("S3D_RENDER_AMBIENT").rstrip("f")) == R.AMBIENT == _lib.RENDER_AMBIENT
    assert float(define("S3D_RENDER_DIFFUSE").rstrip("f")) == R.DIFFUSE == _lib.RENDER_DIFFUSE
    design = open(os.path.join(REPO, "DESIGN.md")).read()
    assert "ambient 0.35" in design and "diffuse 0.65" in design
    # case (e) must loop over LDS chunks
    src = open(os.path.join(REPO, "sin3dm_amd", "csrc", "s3d_render.hip")).read()
    chunk = int(re.search(r"constexpr int kRasterChunk = (\d+);", src).group(1))
    for g in R.GRIDS:
        st = R.restated("e_crowd", g)[2]["status"]
        assert (st == R.OK).sum() > 4 * chunk


def test_every_sample_of_a_tiling_is_covered_once():
    """(a): a fan around a vertex ON a sample centre, with spokes through sample centres, and a quad whose diagonal passes through
    sample centres.  No sample is covered twice; every sample inside the outline (closed triangles, the outer edges open) once."""
    for g, (Ws, Hs, _) in R.GRIDS.items():
        c = R.case("a_fan", g)
        xy, iw, r = R.restated("a_fan", g)
        assert r["count"].max() == 1 and (r["status"] == R.OK).all()
        inside = np.zeros((Hs, Ws), dtype=bool)
        on_shared = 0
        for f in range(len(c["faces"])):
            _, tri, swapped = R.setup(xy, iw, c["faces"], f)
            ed = R.edges(tri)
            # edges() lists the edges opposite the ordered corners 0, 1, 2; in the face's own order edge k joins corners k, k + 1
            own = {0: 2, 1: 0, 2: 1} if not swapped else {0: 1, 1: 0, 2: 2}
            outer = {own[k] for k in c["outer"][f]}
            for j in range(Hs):
                for i in range(Ws):
                    E = R.edge_values(ed, i * R.SUB + R.HALF, j * R.SUB + R.HALF)
                    if all(e >= 0 for e in E) and all(E[k] > 0 for k in outer):
                        inside[j, i] = True
                        on_shared += any(e == 0 for e in E)
        assert on_shared >= 20, on_shared                        # the shared edges and the fan's centre do pass through samples
        assert inside.sum() > 400 and (r["count"][inside] == 1).all()
        assert r["count"][18, 14] == 1                           # the fan's centre vertex


def test_equal_depth_goes_to_the_lower_face():
    for g in R.GRIDS:
        c = R.case("f_twice", g)
        _, _, r = R.restated("f_twice", g)
        half = len(c["faces"]) // 2
        cov = r["count"] > 0
        assert cov.sum() > 500 and (r["count"][cov] % 2 == 0).all()
        assert (r["face_id"][cov] < half).all() and (r["face_id"][cov] >= 0).all() and not r["unclear"].any()


def test_depth_band_is_the_measured_one():
    gap = R.measure_depth_gap()
    print("largest relative float32 / float64 gap of the depth formula", gap, "recorded", R.DEPTH_GAP, "band", R.DEPTH_BAND)
    assert 0.5 * R.DEPTH_GAP < gap <= R.DEPTH_GAP and R.DEPTH_BAND == 10 * R.DEPTH_GAP
    text = open(os.path.join(REPO, "profiles", "render.txt")).read()
    assert f"{R.DEPTH_GAP:.1e}" in text and f"{R.DEPTH_BAND:.1e}" in text
    for n, g in ALL:
        r = R.restated(n, g)[2]
        covered, left = int((r["count"] > 0).sum()), int(r["unclear"].sum())
        print(n, g, "covered", covered, "left out", left)
        assert left <= R.MAX_LEFT_OUT * covered, (n, g)
        if n in R.COMPARED_IN_FULL:
            assert left == 0


def test_cases_are_what_they_claim():
    for g, (Ws, Hs, ss) in R.GRIDS.items():
        assert Ws % ss == 0 and Hs % ss == 0
        assert len(R.case("b_sphere", g)["faces"]) == 320
        r = R.restated("c_slivers", g)[2]
        hit = np.bincount(r["face_id"][r["face_id"] >= 0], minlength=8)
        assert hit[3] == 0 and hit[4] == 0 and hit[5] == 1 and hit[0] > 0 and hit[2] > 0         # no centre inside / exactly one / slivers seen
        assert (R.restated("d_clamped", g)[2]["count"] >= 1).all()                               # larger than the grid
        for n in ("g_off", "g_empty"):
            assert not R.restated(n, g)[2]["count"].any()
        st = R.restated("h_behind", g)[2]["status"]
        assert list(st) == [R.OK, R.NEAR]
        r = R.restated("k_stack", g)[2]
        assert r["count"].max() == 300 > 255 and (r["face_id"][r["count"] > 0] == 0).all()          # past the clamp of the uint8 count
        c = R.case("e_crowd", g)
        xy = R.restated("e_crowd", g)[0]
        assert len(c["faces"]) == 600 and xy.min() >= 16 * R.SUB and xy.max() < 32 * R.SUB          # one tile


def test_texture_lookup_convention():
    """(i): v = 0 is the bottom row of the image, texel centres at (i + 0.5) / W, clamp to edge."""
    img = R.texture_image()
    assert len({tuple(t) for t in img.reshape(-1, 3)}) == 64
    for i in range(8):
        for j in range(8):
            assert np.allclose(R.tex_bilinear(img, (i + 0.5) / 8, 1 - (j + 0.5) / 8) * 255, img[j, i], atol=1e-9)
    assert np.allclose(R.tex_bilinear(img, 1.0 / 8, 1 - 0.5 / 8) * 255, (img[0, 0].astype(float) + img[0, 1]) / 2)
    assert np.allclose(R.tex_bilinear(img, -3.0, 7.0) * 255, img[0, 0]) and np.allclose(R.tex_bilinear(img, 2.0, -1.0) * 255, img[7, 7])
    Ws, Hs, ss = R.GRIDS["g64"]
    c = R.case("i_textured", "g64")
    xy, iw, r = R.restated("i_textured", "g64")
    rgba, base = R.shade(c, xy, iw, r["face_id"], Ws, Hs, ss)
    assert np.allclose(base[7, 9] * 255, img[0, 0], atol=12) and np.allclose(base[28, 9] * 255, img[7, 0], atol=12)      # upright
    assert rgba[..., 3].max() == 255 and rgba[0, 0, 3] == 0 and rgba.shape == (Hs // ss, Ws // ss, 4)
    assert np.allclose(base[18, 45], np.float32([0.2, 0.6, 0.9]))                    # the second material has no image: its Kd
    # the right edge is twice as far: the quad's middle on the screen shows u = 0.35, not 0.5 (perspective-correct interpolation)
    mid = base[18, 24, 0] * 255
    assert img[0, 2, 0] < mid < img[0, 3, 0], mid


def test_camera_rig_is_the_reference_s():
    assert camera.DISTANCE == 3.0 and (camera.FOCAL_MM, camera.SENSOR_MM) == (45.0, 36.0)
    assert camera.VIEW_ANGLES == tuple((float(a), 45.0) for a in (0, 45, 90, 135, 180, 225, 270, 315))
    for az, el in camera.VIEW_ANGLES:
        phi, theta, d = az / 180 * math.pi, el / 180 * math.pi, 3.0
        want = [d * math.sin(theta) * math.cos(phi), d * math.sin(theta) * math.sin(phi), d * math.cos(theta)]     # blender_render_multiview.py:98-100
        assert np.array_equal(camera.camera_position(az, el), np.asarray(want))
        assert abs(np.linalg.norm(want) - 3.0) < 1e-12
    rng = np.random.default_rng(0)
    pts = rng.uniform(-1, 1, (50, 3)) * [2.0, 0.7, 1.1] + [0.3, -2.0, 5.0]
    for res in ((512, 512), (32, 24), (37, 50)):
        views = camera.standard_views(pts.min(0), pts.max(0), res)
        assert len(views) == 8
        world = R.rig_normalize(pts)
        for (az, el), view in zip(camera.VIEW_ANGLES, views):
            assert np.allclose(view.matrix, R.rig_matrix(pts, az, el, *res), rtol=0, atol=1e-12)
            clip = pts @ view.matrix[:, :3].T + view.matrix[:, 3]
            x, y, w = R.rig_project(world, R.rig_camera_position(az, el), *res)
            assert np.allclose(clip[:, 0] / clip[:, 3], x, atol=1e-12) and np.allclose(clip[:, 1] / clip[:, 3], y, atol=1e-12)
            assert np.allclose(clip[:, 3], w, atol=1e-12) and (w > 1.0).all() and view.near == camera.NEAR
            assert np.allclose(view.light, R.RIG_LIGHT)
            # the bounding-box centre is looked at, from distance 3
            centre = np.append((pts.min(0) + pts.max(0)) / 2, 1.0)
            assert np.allclose(view.matrix @ centre, [0, 0, 3, 3], atol=1e-12)
    # a 45 mm lens on a 36 mm sensor: a point 0.4 off axis at distance 1 lands on the image border
    m = camera.view_projection(camera.camera_position(0, 45), (512, 512))
    r, u, f = camera.look_at(camera.camera_position(0, 45))
    edge = m @ np.append(camera.camera_position(0, 45) + f + 0.4 * r, 1.0)
    assert np.allclose(edge[0] / edge[3], 1.0) and abs(u[2]) > 0.5 and np.allclose(np.cross(r, u), -f)


def test_mesh_normalisation():
    rng = np.random.default_rng(1)
    pts = rng.uniform(-1, 1, (200, 3)) * [0.5, 3.0, 1.0] + [4.0, 1.0, -2.0]
    m = camera.normalization_matrix(pts.min(0), pts.max(0))
    got = pts @ m[:3, :3].T + m[:3, 3]
    assert np.allclose(got, R.rig_normalize(pts), atol=1e-12)
    lo, hi = got.min(0), got.max(0)
    assert np.allclose(lo + hi, 0, atol=1e-12) and np.isclose((hi - lo).max(), 2 / 1.03)
    assert np.isclose((hi - lo)[2], 2 / 1.03)                  # the longest axis was y: it stands up (z) after the rotation
    assert np.allclose(m[:3, :3] @ [0, 1, 0], np.array([0, 0, 1]) * m[2, 1]) and m[2, 1] > 0


def test_front_faces_are_told_by_the_screen_area():
    """The shading turns the flat normal towards the camera by the sign of the integer screen area times the handedness of the
    matrix; on the closed sphere that must agree with the geometric test n . (eye - a) > 0 for every face that is not edge-on."""
    for g, (Ws, Hs, ss) in R.GRIDS.items():
        c = R.case("b_sphere", g)
        xy, iw, _ = R.restated("b_sphere", g)
        v = c["verts"].astype(np.float64)
        model = camera.normalization_matrix(v.min(0), v.max(0))
        eye = np.linalg.solve(model, np.append(R.rig_camera_position(45.0, 45.0), 1.0))[:3]
        front_sign = -1 if np.linalg.det(np.asarray(c["matrix"])[[0, 1, 3]][:, :3]) < 0 else 1
        assert front_sign == -1
        checked = 0
        for f, (a, b, d) in enumerate(c["faces"]):
            n = np.cross(v[b] - v[a], v[d] - v[a])
            facing = float(n @ (eye - v[a])) / np.linalg.norm(n) / np.linalg.norm(eye - v[a])
            st, _, swapped = R.setup(xy, iw, c["faces"], f)
            if st != R.OK or abs(facing) < 0.05:
                continue
            assert ((-1 if swapped else 1) * front_sign > 0) == (facing > 0), f
            checked += 1
        assert checked > 250


def test_cli_parsing():
    from sin3dm_amd.rendering import render_multiview as rm
    a = rm.parse_args(["-s", "mesh.obj", "-o", "out"])
    assert (a.mesh_path, a.output_dir, a.image_resolution, a.supersample) == ("mesh.obj", "out", (512, 512), 2)
    b = rm.parse_args(["--mesh_path", "m.obj", "--output_dir", "o", "--image_resolution", "640", "480", "--supersample", "1"])
    assert (b.mesh_path, b.output_dir, b.image_resolution, b.supersample) == ("m.obj", "o", (640, 480), 1)
    for bad in (["-s", "m.obj"], ["-o", "o"], ["-s", "m", "-o", "o", "--supersample", "0"], ["-s", "m", "-o", "o", "--supersample", "9"],
                ["-s", "m", "-o", "o", "--image_resolution", "0", "5"], ["-s", "m", "-o", "o", "--image_resolution", "5"]):
        with pytest.raises(SystemExit):
            rm.parse_args(bad)
    from sin3dm_amd import sample
    assert sample.render_mode("") == "" and sample.render_mode("views") == "views"
    with pytest.raises(ValueError, match="blender"):
        sample.render_mode("blender")


def test_obj_vertex_colours(tmp_path):
    import torch
    from sin3dm_amd.data import obj_io
    from sin3dm_amd.encoding.isosurface import export_obj
    from sin3dm_amd.rendering import render_multiview as rm
    v = torch.tensor([[0.0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]])
    t = torch.tensor([[0, 1, 2], [0, 2, 3]], dtype=torch.int32)
    col = torch.tensor([[0.1, 0.2, 0.3], [1.0, 0.0, 0.5], [0.25, 0.75, 1.5], [0.0, 0.0, 0.0]])
    path = str(tmp_path / "object.obj")
    export_obj(path, v, t, col)
    text = open(path).read()
    got = rm.read_vertex_colors(text)
    assert got.shape == (4, 3) and np.allclose(got, np.clip(col.numpy(), 0, 1), atol=1e-4)
    mesh = rm.load_mesh(path)
    assert np.allclose(mesh["vertex_colors"], got) and not mesh["textured"] and mesh["faces"].shape == (2, 3)
    # parse_obj is what it was: the same keys, no colours
    assert sorted(obj_io.parse_obj(text)) == ["face_mat", "faces", "materials", "n_degenerate", "uvs", "verts"]
    export_obj(path, v, t)
    assert rm.read_vertex_colors(open(path).read()) is None
    assert rm.read_vertex_colors("v 0 0 0 1 0 0\nv 1 0 0\nf 1 2 2\n") is None and rm.read_vertex_colors("") is None


def test_header_binding_and_abi_agree():
    import sin3dm_amd.rendering as rd
    for name in ("render_views", "rasterize", "project", "standard_views", "View"):
        assert callable(getattr(rd, name)), name
    lib = _lib.load()
    header = open(os.path.join(REPO, "include", "sin3dm_hip.h")).read()
    for name in ENTRY_POINTS:
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
        decl = re.search(r"S3D_API int " + name + r"\(([^;]*)\);", header)
        assert decl, name
        assert len(decl.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name
    assert sorted(n for n in _lib.SIGNATURES if n.startswith("s3d_render_")) == sorted(ENTRY_POINTS)
    assert int(re.search(r"#define S3D_ABI_VERSION (\d+)", header).group(1)) == _lib.ABI_VERSION == lib.s3d_abi_version() == 13


def test_argument_errors_launch_nothing():
    """Validation happens before any launch or allocation, so it can be checked without a GPU (the pointers are never read)."""
    lib = _lib.load()
    fake = C.c_void_p(256)
    eye = (C.c_float * 16)(*np.eye(4, dtype=np.float32).reshape(-1))
    nan = (C.c_float * 16)(*([float("nan")] + [0.0] * 15))
    light = (C.c_float * 3)(0, 0, 1)
    inv, uns = _lib.ERR_INVALID, _lib.ERR_UNSUPPORTED
    assert lib.s3d_render_project(fake, 3, eye, 0, 48, 0.1, fake, fake, None) == inv and b"sample grid" in lib.s3d_last_error()
    assert lib.s3d_render_project(fake, 3, eye, 64, _lib.RENDER_MAX_GRID + 1, 0.1, fake, fake, None) == inv
    assert lib.s3d_render_project(fake, 3, nan, 64, 48, 0.1, fake, fake, None) == inv and b"matrix" in lib.s3d_last_error()
    assert lib.s3d_render_project(fake, 3, None, 64, 48, 0.1, fake, fake, None) == inv
    assert lib.s3d_render_project(fake, 3, eye, 64, 48, 0.0, fake, fake, None) == inv and b"near" in lib.s3d_last_error()
    assert lib.s3d_render_project(fake, 3, eye, 64, 48, 0.1, None, fake, None) == inv
    assert lib.s3d_render_project(fake, -1, eye, 64, 48, 0.1, fake, fake, None) == inv
    assert lib.s3d_render_project(None, 0, eye, 64, 48, 0.1, None, None, None) == 0                    # nothing to do
    assert lib.s3d_render_bin_count(fake, fake, 3, fake, 1, 64, 0, fake, fake, None) == inv
    assert lib.s3d_render_bin_count(fake, fake, 3, None, 1, 64, 48, fake, fake, None) == inv and b"face" in lib.s3d_last_error()
    assert lib.s3d_render_bin_count(fake, fake, 3, fake, 1, 64, 48, fake, None, None) == inv
    assert lib.s3d_render_bin_count(fake, fake, 3, None, 0, 64, 48, None, None, None) == 0
    assert lib.s3d_render_bin_fill(fake, fake, 3, fake, 1, 64, 48, fake, _lib.RENDER_MAX_PAIRS + 1, fake, fake, None) == uns
    assert b"pairs" in lib.s3d_last_error() and b"GiB" in lib.s3d_last_error()
    assert lib.s3d_render_bin_fill(fake, fake, 3, fake, 1, 64, 48, fake, -1, fake, fake, None) == inv
    assert lib.s3d_render_bin_fill(fake, fake, 3, fake, 1, 64, 48, None, 5, fake, fake, None) == inv
    assert lib.s3d_render_bin_fill(fake, fake, 3, fake, 1, 64, 48, None, 0, None, None, None) == 0
    assert lib.s3d_render_raster(fake, fake, 3, fake, 1, 64, 48, None, fake, 5, fake, fake, fake, None) == inv
    assert lib.s3d_render_raster(fake, fake, 3, fake, 1, 64, 48, fake, None, 5, fake, fake, fake, None) == inv
    assert lib.s3d_render_raster(fake, fake, 3, fake, 1, 64, 48, fake, fake, 5, fake, None, fake, None) == inv
    assert lib.s3d_render_raster(fake, fake, 3, fake, 1, 5000, 48, fake, fake, 5, fake, fake, fake, None) == inv

    def shade(ws=64, hs=48, ss=2, m=eye, li=light, n_mats=0, table=None, kd=None, images=None, image_bytes=0, rgba=fake, face_id=fake):
        return lib.s3d_render_shade(fake, fake, fake, 3, fake, 1, face_id, ws, hs, ss, m, li, None, None, None, table, kd, n_mats, images,
                                    image_bytes, rgba, None)
    assert shade(ss=0) == inv and b"supersample" in lib.s3d_last_error()
    assert shade(ss=9) == inv and shade(ws=50, hs=37, ss=2) == inv
    assert shade(m=nan) == inv and shade(m=None) == inv and shade(li=None) == inv
    assert shade(n_mats=1) == inv and b"material" in lib.s3d_last_error()
    assert shade(image_bytes=12) == inv and b"image" in lib.s3d_last_error()
    assert shade(rgba=None) == inv and shade(face_id=None) == inv
