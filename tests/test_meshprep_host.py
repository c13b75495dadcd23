"""CPU-only: the host half of the mesh preprocessing (sin3dm_amd/data): normalize_aabb / sample_grid_points_aabb against the
reference's data/utils.py (tests/golden/prepare_host.npz, written by tests/golden/make_golden_prepare.py), the OBJ/MTL reader on
texts written here, the command line's defaults, and the refusal to run without a GPU."""
import warnings

import numpy as np
import pytest
import torch

from conftest import golden
from sin3dm_amd.data import mesh_sampler, obj_io
from sin3dm_amd.data.utils import normalize_aabb, sample_grid_points_aabb

SETS = ("towerruins_bbox", "cube", "slab", "needle", "offset")


def test_utils_match_the_reference():
    g = golden("prepare_host")
    for name in SETS:
        v = g[f"{name}/verts"]
        for i, (reso, mult, enlarge) in enumerate(g["configs"]):
            aabb, translation, scale = normalize_aabb(v, int(reso), enlarge_scale=float(enlarge), mult=int(mult))
            for got, key in ((aabb, "aabb"), (translation, "translation"), (scale, "scale")):
                np.testing.assert_allclose(got, g[f"{name}/{i}/{key}"], rtol=1e-13, atol=0, err_msg=f"{name}/{i}/{key}")
            grid = sample_grid_points_aabb(aabb, int(reso))
            assert grid.dtype == np.float64 and tuple(grid.shape) == tuple(g[f"{name}/{i}/shape"]), (name, i)
            for got, key in ((grid[:, 0, 0, 0], "xs"), (grid[0, :, 0, 1], "ys"), (grid[0, 0, :, 2], "zs"), (grid[-1, -1, -1], "corner")):
                np.testing.assert_allclose(got, g[f"{name}/{i}/{key}"], rtol=1e-13, atol=0, err_msg=f"{name}/{i}/{key}")
            assert np.array_equal(grid[3, 2, 1], [grid[3, 0, 0, 0], grid[0, 2, 0, 1], grid[0, 0, 1, 2]])       # indexing="ij"
    assert np.array_equal(g["towerruins_bbox/0/aabb"], [-0.71875, -1, -0.71875, 0.71875, 1, 0.71875])
    assert tuple(g["towerruins_bbox/0/shape"]) == (184, 256, 184, 3)


OBJ = """# two materials, a quad, negative indices, a corner without vt, a degenerate face
mtllib scene.mtl
v 0 0 0
v 1 0 0
v 1 1 0
v 0 1 0
v 0 0 1
vt 0 0
vt 1 0
vt 1 1
vt 0 1
vn 0 0 1
usemtl painted
f 1/1/1 2/2/1 3/3/1 4/4/1
usemtl plain
f -1 -5 -4
f 1//1 2//1 5//1
f 1/1 2/2 2/2
f 5/4 3 4/1
"""
MTL = """newmtl painted
Ka 0.1 0.2 0.3
Kd 0.4 0.5 0.6
Ks 0.7 0.8 0.9
Ns 33
map_Kd -s 1 1 1 missing_texture.png
newmtl plain
Kd 0.25 0.5 0.75
"""


def test_obj_reader(tmp_path):
    m = obj_io.parse_obj(OBJ, lambda name: MTL if name == "scene.mtl" else None)
    assert m["verts"].shape == (5, 3) and m["n_degenerate"] == 1
    assert m["faces"].tolist() == [[0, 1, 2], [0, 2, 3], [4, 0, 1], [0, 1, 4], [4, 2, 3]]          # the quad as a fan, -1 = the last vertex
    assert m["face_mat"].tolist() == [0, 0, 1, 1, 1] and [n for n, _ in m["materials"]] == ["painted", "plain"]
    assert m["uvs"][0].tolist() == [[0, 0], [1, 0], [1, 1]] and m["uvs"][1].tolist() == [[0, 0], [1, 1], [0, 1]]
    assert (m["uvs"][2] == 0).all() and (m["uvs"][3] == 0).all()                                # no vt: uv 0
    assert m["uvs"][4].tolist() == [[0, 1], [0, 0], [0, 0]]                                      # one corner without vt
    painted, plain = (d for _, d in m["materials"])
    assert painted["Ka"] == (0.1, 0.2, 0.3) and painted["Kd"] == (0.4, 0.5, 0.6) and painted["Ks"] == (0.7, 0.8, 0.9) and painted["Ns"] == 33
    assert painted["map_Kd"] == "missing_texture.png" and plain["map_Kd"] is None
    assert plain["Kd"] == (0.25, 0.5, 0.75) and plain["Ns"] == obj_io.DEFAULT_MATERIAL["Ns"]
    with pytest.raises(ValueError):
        obj_io.parse_obj("v 0 0 0\nf 1 2 3\n")
    # from files: an unreadable map_Kd falls back to Kd with a warning
    (tmp_path / "scene.obj").write_text(OBJ)
    (tmp_path / "scene.mtl").write_text(MTL.replace("missing_texture.png", "broken.png"))
    (tmp_path / "broken.png").write_bytes(b"not a png")
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        mesh = obj_io.load_obj(str(tmp_path / "scene.obj"))
    assert any("broken.png" in str(x.message) and "Kd" in str(x.message) for x in w), [str(x.message) for x in w]
    assert mesh["materials"][0][1]["image"] is None and mesh["materials"][1][1]["image"] is None
    ms = mesh_sampler.MeshSampler(str(tmp_path / "scene.obj"))
    assert ms.fs.shape == (5, 3) and ms.n_degenerate == 1 and np.array_equal(ms.Kds, [[0.4, 0.5, 0.6], [0.25, 0.5, 0.75]])
    assert ms.Nss.tolist() == [33, 10] and ms.materials[0]["image"] is None
    ms.normalize(reso=16, mult=4)
    assert np.abs(ms.vs).max() <= 1 and ms.aabb.shape == (6,)


def test_obj_reader_reads_an_image(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    img = np.arange(4 * 6 * 3, dtype=np.uint8).reshape(4, 6, 3)
    Image.fromarray(img).save(tmp_path / "tex.png")
    (tmp_path / "a.mtl").write_text("newmtl m\nKd 1 1 1\nmap_Kd tex.png\n")
    (tmp_path / "a.obj").write_text("mtllib a.mtl\nusemtl m\nv 0 0 0\nv 1 0 0\nv 0 1 0\nvt 0 0\nvt 1 0\nvt 0 1\nf 1/1 2/2 3/3\n")
    mesh = obj_io.load_obj(str(tmp_path / "a.obj"))
    assert np.array_equal(mesh["materials"][0][1]["image"], img)


def test_cli_defaults():
    a = mesh_sampler.parse_args(["-s", "a.obj", "-d", "b.npz"])
    assert (a.reso, a.n_surf, a.mult, a.enlarge_scale, a.only_vol, a.seed) == (256, 2_000_000, 8, 1.03, False, 0)
    assert a.threshold == 2. / 256 * 3
    assert mesh_sampler.parse_args(["-s", "a", "-d", "b", "--reso", "64"]).threshold == 2. / 64 * 3
    assert mesh_sampler.parse_args(["-s", "a", "-d", "b", "--reso", "64", "--threshold", "0.1"]).threshold == 0.1
    b = mesh_sampler.parse_args(["-s", "a", "-d", "b", "-wt", "--watertight_reso", "5000", "--only_vol"])      # accepted, do nothing
    assert b.watertight and b.watertight_reso == 5000 and b.only_vol
    text = mesh_sampler.build_parser().format_help()
    assert text.count("does nothing") == 2


def test_no_gpu_is_refused_loudly(tmp_path, monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    (tmp_path / "t.obj").write_text("v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 3\n")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mesh_sampler.main(["-s", str(tmp_path / "t.obj"), "-d", str(tmp_path / "t.npz")])
    assert not (tmp_path / "t.npz").exists()
    ms = mesh_sampler.MeshSampler(str(tmp_path / "t.obj"))
    for call in (lambda: ms.query_sdf(np.zeros((4, 3)), 0.1), lambda: ms.query_tex(np.zeros((4, 3)), 0.1), lambda: ms.sample_surf(10)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
