"""CPU-only: the host half of the PBR mesh preprocessing (sin3dm_amd/data/mesh_sampler_pbr.py): where the maps of a path come from
(textures/ first, then the MTL's entries, then the scalars), the float64 restatement of the texel rule on texel-centre uvs, the
command line's defaults, and the refusal to run without a GPU."""
import os
import warnings

import numpy as np
import pytest
import torch
from PIL import Image

from meshprep_pbr_cases import COLUMNS, FIELDS, FLAT_NORMAL, centre_uv, coded_plane, coded_rgb, near_border, texels8
from sin3dm_amd.data import mesh_sampler_pbr
from sin3dm_amd.data.mesh_sampler_pbr import MeshSamplerPBR

OBJ = "mtllib m.mtl\nv 0 0 0\nv 1 0 0\nv 0 1 0\nv 0 0 1\nvt 0 0\nvt 1 0\nvt 0 1\nusemtl a\nf 1/1 2/2 3/3\nusemtl b\nf 1/1 2/2 4/3\n"
MTL_PLAIN = "newmtl a\nKd 0.2 0.4 0.6\nPm 0.25\nPr 0.5\nnewmtl b\nKd 0.1 0.1 0.1\n"
MTL_MAPS = ("newmtl a\nKd 0.2 0.4 0.6\nmap_Kd own_albedo.png\nmap_Pm own_metal.png\nmap_Pr own_rough.png\nmap_Bump -bm 1.0 own_normal.png\n"
            "newmtl b\nKd 0.1 0.1 0.1\nnorm own_normal.png\n")


def scene(tmp_path, mtl=MTL_PLAIN, **textures):
    """m.obj / m.mtl in tmp_path and the given files in textures/ (name with extension -> array)."""
    (tmp_path / "m.obj").write_text(OBJ)
    (tmp_path / "m.mtl").write_text(mtl)
    if textures:
        os.makedirs(tmp_path / "textures", exist_ok=True)
    for name, img in textures.items():
        Image.fromarray(img).save(tmp_path / "textures" / name.replace("_", ".", 1))
    return str(tmp_path / "m.obj")


def own_maps(tmp_path):
    Image.fromarray(coded_rgb(4, 4, 5)).save(tmp_path / "own_albedo.png")
    Image.fromarray(coded_plane(3, 3, 1)).save(tmp_path / "own_metal.png")
    Image.fromarray(coded_plane(2, 2, 2)).save(tmp_path / "own_rough.png")
    Image.fromarray(coded_rgb(5, 5, 6)).save(tmp_path / "own_normal.png")


def maps_of(ms, i):
    return [ms.materials[i].get(k) for k in ("image", "metallic_image", "roughness_image", "normal_image")]


# ------------------------------------------------------------------ discovery
def test_metallic_roughness_file_wins_and_its_channels(tmp_path):
    """metallicRoughness.*: channel 0 is metallic, channel 1 roughness (the reference's [..., :2], not glTF's G / B), and the
    separate files beside it are not looked at; the found set applies to every material."""
    packed = np.stack([coded_plane(6, 4, 1), coded_plane(6, 4, 2), np.full((4, 6), 99, np.uint8)], -1)
    path = scene(tmp_path, albedo_png=coded_rgb(8, 4, 1), metallicRoughness_png=packed, metallic_png=coded_plane(3, 3, 3),
                 roughness_png=coded_plane(3, 3, 0), normal_png=coded_rgb(5, 7, 2))
    ms = MeshSamplerPBR(path)
    assert len(ms.materials) == 2
    for i in range(2):
        albedo, metallic, roughness, normal = maps_of(ms, i)
        assert np.array_equal(albedo, coded_rgb(8, 4, 1)) and np.array_equal(normal, coded_rgb(5, 7, 2))
        assert np.array_equal(metallic, packed[..., 0]) and np.array_equal(roughness, packed[..., 1])
    assert ms.materials[0]["Pm"] == 0.25 and ms.materials[0]["Pr"] == 0.5 and ms.materials[1]["Pm"] == 0.0 and ms.materials[1]["Pr"] == 0.0


def test_separate_metallic_and_roughness_files(tmp_path):
    path = scene(tmp_path, albedo_png=coded_rgb(8, 4, 1), metallic_png=coded_plane(3, 5, 3), roughness_png=coded_plane(5, 3, 0),
                 normal_png=coded_rgb(5, 7, 2))
    _, metallic, roughness, _ = maps_of(MeshSamplerPBR(path), 1)
    assert np.array_equal(metallic, coded_plane(3, 5, 3)) and np.array_equal(roughness, coded_plane(5, 3, 0))


@pytest.mark.parametrize("missing", ["metallic", "roughness"])
def test_one_of_the_two_separate_files_missing(tmp_path, missing):
    """The missing one falls back to the scalar (Pm / Pr, or 0), the other is read."""
    files = {"metallic_png": coded_plane(3, 5, 3), "roughness_png": coded_plane(5, 3, 0)}
    del files[missing + "_png"]
    ms = MeshSamplerPBR(scene(tmp_path, albedo_png=coded_rgb(8, 4, 1), normal_png=coded_rgb(5, 7, 2), **files))
    _, metallic, roughness, _ = maps_of(ms, 0)
    if missing == "metallic":
        assert metallic is None and np.array_equal(roughness, coded_plane(5, 3, 0))
    else:
        assert roughness is None and np.array_equal(metallic, coded_plane(3, 5, 3))
    row = texels8([0, 1], np.array([[1.0, 0, 0]] * 2), ms.uvs, ms.face_mat, ms.materials)
    col, scalars = (3, (0.25, 0.0)) if missing == "metallic" else (4, (0.5, 0.0))
    assert row[:, col].tolist() == [np.float32(s) for s in scalars]


def test_no_textures_folder_uses_the_mtl_entries(tmp_path):
    own_maps(tmp_path)
    ms = MeshSamplerPBR(scene(tmp_path, mtl=MTL_MAPS))
    albedo, metallic, roughness, normal = maps_of(ms, 0)
    assert np.array_equal(albedo, coded_rgb(4, 4, 5)) and np.array_equal(metallic, coded_plane(3, 3, 1))
    assert np.array_equal(roughness, coded_plane(2, 2, 2)) and np.array_equal(normal, coded_rgb(5, 5, 6))
    albedo, metallic, roughness, normal = maps_of(ms, 1)                      # material b: only `norm`
    assert albedo is None and metallic is None and roughness is None and np.array_equal(normal, coded_rgb(5, 5, 6))


def test_a_file_in_textures_overrides_the_mtl_entry_per_channel(tmp_path):
    own_maps(tmp_path)
    ms = MeshSamplerPBR(scene(tmp_path, mtl=MTL_MAPS, roughness_png=coded_plane(5, 3, 0)))
    for i in range(2):
        assert np.array_equal(ms.materials[i]["roughness_image"], coded_plane(5, 3, 0))
    assert np.array_equal(ms.materials[0]["image"], coded_rgb(4, 4, 5)) and ms.materials[1]["image"] is None
    assert np.array_equal(ms.materials[0]["metallic_image"], coded_plane(3, 3, 1))


def test_no_maps_at_all_gives_the_scalars_and_the_flat_normal(tmp_path):
    ms = MeshSamplerPBR(scene(tmp_path))
    assert all(x is None for i in range(2) for x in maps_of(ms, i))
    rows = texels8([0, 1, -1], np.array([[0.2, 0.3, 0.5]] * 3), ms.uvs, ms.face_mat, ms.materials)
    flat = FLAT_NORMAL.astype(np.float32) / np.float32(255)
    assert np.array_equal(rows[0], np.concatenate([np.float32([0.2, 0.4, 0.6, 0.25, 0.5]), flat]))
    assert np.array_equal(rows[1], np.concatenate([np.float32([0.1, 0.1, 0.1, 0.0, 0.0]), flat]))
    assert (rows[2] == 0).all()


def test_an_unreadable_file_warns_and_falls_back(tmp_path):
    """textures/albedo.png is not an image: the MTL's map_Kd is used; textures/normal.png neither, and material b has `norm`."""
    own_maps(tmp_path)
    path = scene(tmp_path, mtl=MTL_MAPS, metallic_png=coded_plane(3, 5, 3))
    (tmp_path / "textures" / "albedo.png").write_bytes(b"not a png")
    (tmp_path / "own_normal.png").write_bytes(b"not a png either")
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        ms = MeshSamplerPBR(path)
    text = [str(x.message) for x in w]
    assert any("textures" in t and "albedo.png" in t for t in text) and any("own_normal.png" in t for t in text), text
    assert np.array_equal(ms.materials[0]["image"], coded_rgb(4, 4, 5)) and ms.materials[1]["image"] is None
    assert ms.materials[0]["normal_image"] is None and ms.materials[1]["normal_image"] is None
    assert np.array_equal(ms.materials[1]["metallic_image"], coded_plane(3, 5, 3))


def test_first_match_in_sorted_order(tmp_path):
    path = scene(tmp_path, albedo_png=coded_rgb(8, 4, 1), normal_png=coded_rgb(5, 7, 2))
    Image.fromarray(coded_rgb(6, 6, 3)).save(tmp_path / "textures" / "albedo.bmp")          # "albedo.bmp" < "albedo.png"
    Image.fromarray(coded_rgb(7, 7, 4)).save(tmp_path / "textures" / "normal.tga")          # "normal.png" < "normal.tga"
    ms = MeshSamplerPBR(path)
    assert np.array_equal(ms.materials[0]["image"], coded_rgb(6, 6, 3)) and np.array_equal(ms.materials[0]["normal_image"], coded_rgb(5, 7, 2))
    found = mesh_sampler_pbr.discover_maps(path)
    assert sorted(found) == ["image", "normal_image"]


def test_images_are_read_as_rgb_or_l(tmp_path):
    """An RGBA albedo loses its alpha, a palette normal map is expanded, an RGB metallic map is read as luma (PIL's L)."""
    rgba = np.concatenate([coded_rgb(4, 3, 1), np.full((3, 4, 1), 17, np.uint8)], -1)
    grey3 = np.repeat(coded_plane(4, 3, 1)[..., None], 3, -1)
    path = scene(tmp_path, albedo_png=rgba, metallic_png=grey3)
    Image.fromarray(coded_rgb(4, 4, 2)).convert("P").save(tmp_path / "textures" / "normal.png")
    ms = MeshSamplerPBR(path)
    assert np.array_equal(ms.materials[0]["image"], rgba[..., :3])
    assert np.array_equal(ms.materials[0]["metallic_image"], coded_plane(4, 3, 1))           # luma of a grey RGB texel is the grey
    assert ms.materials[0]["normal_image"].shape == (4, 4, 3)


# ------------------------------------------------------------------ the restatement at texel centres
def _one_face_per_uv(uv):
    """Faces whose three corners all carry uv[k]: any barycentrics give that uv."""
    uvs = np.repeat(np.asarray(uv, dtype=np.float64)[:, None, :], 3, 1)
    return np.arange(len(uvs)), np.tile([[0.25, 0.5, 0.25]], (len(uvs), 1)), uvs, np.zeros(len(uvs), dtype=np.int64)


@pytest.mark.parametrize("sizes", [((16, 8), (5, 7), (7, 5), (12, 12)), ((1, 1), (1, 1), (1, 1), (1, 1)), ((1, 6), (6, 1), (1, 3), (4, 1)),
                                   ((8, 8), (8, 8), (8, 8), (8, 8))])
def test_restatement_returns_the_stored_texel_at_texel_centres(sizes):
    """Every texel of every map, at its centre uv and at that uv shifted so that the rounded coordinate lies k W (k H) texels
    away, k in -2 .. 2 (uv outside [0, 1]: wrapped)."""
    imgs = [coded_rgb(*sizes[0], 1), coded_plane(*sizes[1], 2), coded_plane(*sizes[2], 3), coded_rgb(*sizes[3], 4)]
    mat = {"Kd": (0.5, 0.5, 0.5), "image": imgs[0], "metallic_image": imgs[1], "roughness_image": imgs[2], "normal_image": imgs[3]}
    for img, field, (W, H), (c0, c1) in zip(imgs, FIELDS, sizes, COLUMNS):
        ys, xs = (a.reshape(-1) for a in np.mgrid[0:H, 0:W])
        alone = [{field: img}]                                                              # (a centre of this map is none of the others')
        for k in (-2, -1, 0, 1, 2):
            uv = centre_uv(xs + k * W, ys - k * H, W, H)
            assert k == 0 or W == 1 or (uv[:, 0] < 0).any() or (uv[:, 0] > 1).any()
            face, bary, uvs, face_mat = _one_face_per_uv(uv)
            assert not near_border(face, bary, uvs, face_mat, alone).any()
            got = texels8(face, bary, uvs, face_mat, [mat])[:, c0:c1]
            want = img.reshape(H, W, -1)[ys, xs].astype(np.float32) / np.float32(255)
            assert np.array_equal(got, want), (W, H, k)


def test_restatement_fallbacks():
    """NaN uv component -> the texel of 0; an infinite or runaway one -> the map's fallback; a map past image_bytes -> absent."""
    mat = {"Kd": (0.5, 0.25, 0.125), "Pm": 0.75, "Pr": 0.375, "image": coded_rgb(4, 4, 1), "metallic_image": coded_plane(4, 4, 2),
           "roughness_image": coded_plane(1, 1, 3), "normal_image": coded_rgb(4, 4, 4)}
    uv = np.array([[np.nan, 1.0], [1.0, np.nan], [np.inf, 0.5], [0.5, -2e9], [1.0, 0.0]])
    face, bary, uvs, face_mat = _one_face_per_uv(uv)
    rows = texels8(face, bary, uvs, face_mat, [mat])
    b = lambda v: np.float32(v) / np.float32(255)                                          # noqa: E731
    assert rows[0, 0] == b(1) and rows[0, 1] == b(1)                                        # u = 0, v = 1: texel (0, 0)
    assert rows[1, 0] == b(3 * 16 + 1) and rows[1, 1] == b(3 * 16 + 1)                      # u = 1, v = 0: texel (3, 3)
    flat = FLAT_NORMAL.astype(np.float32) / np.float32(255)
    # u = inf: every map falls back, the 1 x 1 one too (inf * 0 is a NaN); v = -2e9: (1 - v) (H - 1) is 0 on the 1 x 1 map, which is read
    assert np.array_equal(rows[2], np.concatenate([np.float32([0.5, 0.25, 0.125, 0.75, 0.375]), flat]))
    assert np.array_equal(rows[3], np.concatenate([np.float32([0.5, 0.25, 0.125, 0.75]), [b(3)], flat]))
    assert rows[4, 4] == b(3)                                                               # the 1 x 1 roughness map
    total = 48 + 16 + 1 + 48
    cut = texels8(face, bary, uvs, face_mat, [mat], image_bytes=total - 1)
    assert np.array_equal(cut[:, :5], rows[:, :5]) and np.array_equal(cut[[0, 1, 4], 5:], np.tile(flat, (3, 1)))
    assert np.array_equal(texels8(face, bary, uvs, face_mat, [mat], image_bytes=total), rows)


# ------------------------------------------------------------------ the command line
def test_cli_defaults():
    a = mesh_sampler_pbr.parse_args(["-s", "a.obj", "-d", "b.npz"])
    assert (a.reso, a.watertight_reso, a.n_surf, a.mult, a.enlarge_scale, a.watertight, a.only_vol, a.seed) == (256, 100_000, 2_000_000, 8, 1.03,
                                                                                                                 False, False, 0)
    assert a.threshold == 2. / 256 * 3                                                      # reference :148-149
    assert mesh_sampler_pbr.parse_args(["-s", "a", "-d", "b", "--reso", "64"]).threshold == 2. / 64 * 3
    assert mesh_sampler_pbr.parse_args(["-s", "a", "-d", "b", "--reso", "64", "--threshold", "0.1"]).threshold == 0.1
    b = mesh_sampler_pbr.parse_args(["-s", "a", "-d", "b", "-wt", "--watertight_reso", "5000", "--only_vol"])      # accepted, do nothing
    assert b.watertight and b.watertight_reso == 5000 and b.only_vol
    text = mesh_sampler_pbr.build_parser().format_help()
    assert text.count("does nothing") == 2 and "mesh_sampler_pbr" in text
    assert mesh_sampler_pbr.KEYS_ALL == ("pts_grid", "sdf_grid", "tex_grid", "aabb", "threshold", "pts_on_surf", "tex_on_surf", "pts_near_surf",
                                         "sdf_near_surf", "tex_near_surf")


def test_no_gpu_is_refused_loudly(tmp_path, monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    (tmp_path / "t.obj").write_text("v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 3\n")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mesh_sampler_pbr.main(["-s", str(tmp_path / "t.obj"), "-d", str(tmp_path / "out" / "t.npz")])
    assert not (tmp_path / "out").exists()                                                  # refused before any work
    ms = MeshSamplerPBR(str(tmp_path / "t.obj"))
    face, bary = torch.zeros(4, dtype=torch.int32), torch.zeros((4, 3))
    for call in (lambda: ms.materials8(face, bary), lambda: ms.query_tex(np.zeros((4, 3)), 0.1), lambda: ms.query_sdf(np.zeros((4, 3)), 0.1)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
