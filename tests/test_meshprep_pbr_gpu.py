"""GPU tests of the PBR mesh preprocessing (sin3dm_amd/data/mesh_sampler_pbr.py, s3d_meshpbr.hip) against the float64 / integer
restatement of tests/meshprep_pbr_cases.py.  Everything is held bit for bit: the outputs are bytes / 255 (one correctly rounded
division) or material factors passed through; the only place float32 and float64 can differ is the rounding of a texel
coordinate next to a half-integer, and the queries where that can happen are chosen on the host (near_border) and counted."""
import ctypes as C
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO
from meshprep_cases import rotation, torus
from meshprep_pbr_cases import (BORDER_CAP, FIELDS, FLAT_NORMAL, centre_uv, coded_plane, coded_rgb, material0, material1, near_border, pbr_case,
                                texels8)

pytestmark = pytest.mark.gpu
FLAT = FLAT_NORMAL.astype(np.float32) / np.float32(255)


def _dev(face, bary):
    import torch
    return (torch.from_numpy(np.ascontiguousarray(face, dtype=np.int32)).cuda(), torch.from_numpy(np.ascontiguousarray(bary, dtype=np.float32)).cuda())


# ------------------------------------------------------------------ 1, 2: the shared query set
def test_materials8_equals_the_restatement():
    """6000 Dirichlet barycentrics on random faces of the torus, uv = ((x + 1) / 2, (z + 1) / 2); material 0: albedo 16 x 8,
    metallic 5 x 7, roughness 7 x 5, normal 12 x 12, material 1: scalars.  Queries whose float64 texel coordinate of some map is
    within 1e-3 of a half-integer are left out: about 0.4 % per distinct map size, 38 of 3123 = 1.2 % here, at most 2 %."""
    pc = pbr_case()
    share = pc.border.sum() / pc.on0.sum()
    print(f"{len(pc.face)} queries, {int(pc.on0.sum())} on material 0, {int(pc.border.sum())} left out near a texel border ({share:.4f})")
    assert share <= BORDER_CAP and pc.on0.sum() > 2000 and (~pc.on0).sum() > 2000 and not pc.border[~pc.on0].any()
    got = pc.sampler().materials8(*_dev(pc.face, pc.bary32))
    assert got.dtype.is_floating_point and tuple(got.shape) == (len(pc.face), 8) and got.is_cuda
    got = got.cpu().numpy()
    assert got.dtype == np.float32
    keep = ~pc.border
    assert np.array_equal(got[keep], pc.expect[keep])
    assert len(np.unique(got[pc.on0][:, :3], axis=0)) > 50 and len(np.unique(got[pc.on0][:, 5:], axis=0)) > 50       # the maps were read
    assert (got[~pc.on0] == np.concatenate([np.float32([0.25, 0.5, 0.125, 0.3, 0.7]), FLAT])).all()


def test_albedo_columns_equal_the_three_channel_kernel():
    """Columns 0:3 against MeshSampler.colors on the same queries and maps, every query, bit for bit."""
    pc = pbr_case()
    ms = pc.sampler()
    face, bary = _dev(pc.face, pc.bary32)
    assert np.array_equal(ms.materials8(face, bary)[:, :3].cpu().numpy(), ms.colors(face, bary).cpu().numpy())
    assert tuple(ms.colors(face, bary).shape) == (len(pc.face), 3)                           # the base class's colours are what they were


# ------------------------------------------------------------------ 3: edges
@pytest.mark.parametrize("n", [0, 1, 255, 256, 257])
def test_block_edges(n):
    pc = pbr_case()
    got = pc.sampler().materials8(*_dev(pc.face[:n], pc.bary32[:n])).cpu().numpy()
    keep = ~pc.border[:n]
    assert got.shape == (n, 8) and np.array_equal(got[keep], pc.expect[:n][keep])


class EdgeMesh:
    """One face per uv: the three corners of face k all carry uv[k], so barycentrics (1, 0, 0) give uv[k] exactly; material k % 3,
    the LAST one with maps (so its normal map ends the packed buffer), material 1 with a 1 x 1 and a 1 x H map."""

    def __init__(self, uv, corner1=None):
        from sin3dm_amd.data.mesh_sampler_pbr import MeshSamplerPBR
        uv = np.asarray(uv, dtype=np.float32)
        n = len(uv)
        self.uvs = np.repeat(uv[:, None, :], 3, 1)
        if corner1 is not None:
            self.uvs[:, 1] = corner1                                                         # weight 0, but 0 * NaN is a NaN
        self.face_mat = (np.arange(n) % 3).astype(np.int32)
        self.materials = [material1(), {"Kd": (0.5, 0.5, 0.5), "metallic_image": coded_plane(1, 1, 1), "roughness_image": coded_plane(1, 6, 2)},
                          material0()]
        verts = np.stack([np.arange(n)[:, None] + np.array([0.0, 1.0, 0.0])[None], np.tile([0.0, 0.0, 1.0], (n, 1)), np.zeros((n, 3))], -1)
        self.ms = MeshSamplerPBR(verts=verts.reshape(-1, 3), faces=np.arange(3 * n).reshape(n, 3), uvs=self.uvs.astype(np.float64),
                                 face_mat=self.face_mat, materials=self.materials)
        self.face = np.arange(n, dtype=np.int32)
        self.bary = np.tile(np.float32([1, 0, 0]), (n, 1))

    def expect(self, **kw):
        return texels8(self.face, self.bary.astype(np.float64), self.uvs.astype(np.float64), self.face_mat, self.materials, **kw)

    def border(self):
        return near_border(self.face, self.bary.astype(np.float64), self.uvs.astype(np.float64), self.face_mat, self.materials)


def test_missing_face_nan_uv_and_wrapping():
    rng = np.random.Generator(np.random.PCG64(3))
    uv = rng.uniform(-1.5, 2.5, size=(600, 2))
    em = EdgeMesh(uv)
    keep = ~em.border()
    assert keep.mean() > 0.9 and ((uv < 0).any(1) | (uv > 1).any(1))[keep].mean() > 0.5
    face = em.face.copy()
    face[::7] = -1
    got = em.ms.materials8(*_dev(face, em.bary)).cpu().numpy()
    want = em.expect()
    want[::7] = 0
    assert (got[::7] == 0).all() and np.array_equal(got[keep], want[keep])
    # a NaN corner (weight 0) makes the interpolated component a NaN: the texel of 0 in that component
    nan_u, nan_v = np.array([np.nan, 0.0], dtype=np.float32), np.array([0.0, np.nan], dtype=np.float32)
    for corner1, zeroed in ((nan_u, 0), (nan_v, 1), (np.float32([np.nan, np.nan]), None)):
        em = EdgeMesh(uv, corner1)
        twin_uv = uv.copy()
        twin_uv[:, [0, 1] if zeroed is None else [zeroed]] = 0.0
        twin = EdgeMesh(twin_uv)
        keep = ~twin.border()
        got = em.ms.materials8(*_dev(em.face, em.bary)).cpu().numpy()
        assert np.array_equal(got[keep], twin.expect()[keep]) and np.array_equal(em.expect()[keep], twin.expect()[keep])
    # an infinite or runaway uv: every map falls back like an absent one
    # (all three weights non-zero: 0 * inf would be a NaN, the case above).  The last uv, (0.5, 0.5), is exact in both precisions
    # and lies on texel borders of the 16 x 8 and 12 x 12 maps: half to even
    em = EdgeMesh(np.repeat(np.array([[np.inf, 0.5], [0.5, -np.inf], [3e9, 0.5], [-3e9, 3e9], [0.5, 0.5]]), 3, 0))
    em.bary = np.tile(np.float32([0.25, 0.5, 0.25]), (len(em.face), 1))
    got = em.ms.materials8(*_dev(em.face, em.bary)).cpu().numpy()
    assert np.array_equal(got, em.expect())
    fallback = np.concatenate([np.float32([1.0, 0.0, 1.0, 0.75, 0.375]), FLAT])                           # material 0 of the shared case, no texel
    assert (got[2:12:3] == fallback).all() and (got[14] != fallback).all()
    assert np.array_equal(got[14, :3], coded_rgb(16, 8, 1)[4, 8].astype(np.float32) / np.float32(255))   # 7.5 -> 8, 3.5 -> 4


def test_last_material_and_the_end_of_the_buffer():
    """The last table row is a material with maps; its normal map is the last thing in the packed buffer, and uv (1, 0) reads that
    map's last texel — the buffer's last three bytes.  Told one byte less, the device treats the map as absent."""
    import torch
    from sin3dm_amd import _lib
    W, H = 12, 12
    uv = np.concatenate([centre_uv(W - 1, H - 1, W, H)[None], centre_uv(np.arange(W), np.arange(H)[::-1], W, H), [[1.0, 0.0]] * 3])
    uv = np.repeat(uv, 3, 0)                                                                # every uv on each of the three materials
    em = EdgeMesh(uv)
    d = em.ms._device()
    total = d["pbr_img_bytes"]
    assert total == 1 + 6 + sum(material0()[k].size for k in FIELDS) and int(d["pbr_table"][2, 3, 0]) + W * H * 3 == total
    assert d["pbr_img"].numel() == total
    got = em.ms.materials8(*_dev(em.face, em.bary)).cpu().numpy()
    assert np.array_equal(got, em.expect()) and not em.border()[2::3].any()
    assert np.array_equal(got[2, 5:], coded_rgb(W, H, 4)[H - 1, W - 1].astype(np.float32) / np.float32(255))
    face, bary = _dev(em.face, em.bary)
    out = torch.empty((len(em.face), 8), device="cuda", dtype=torch.float32)
    for told in (total - 1, total - W * H * 3, 0):
        _lib.check(_lib.load().s3d_meshsdf_texture_pbr(_lib.ptr(face), _lib.ptr(bary), len(em.face), _lib.ptr(d["uv"]), _lib.ptr(d["face_mat"]),
                                                       d["uv"].shape[0], _lib.ptr(d["pbr_table"]), _lib.ptr(d["pbr_factors"]), 3,
                                                       _lib.ptr(d["pbr_img"]), told, _lib.ptr(out), _lib.stream_ptr()))
        cut = out.cpu().numpy()
        assert np.array_equal(cut, em.expect(image_bytes=told)), told
        assert (cut[2::3, 5:] == FLAT).all() and np.array_equal(cut[2::3, :5], got[2::3, :5]) == (told != 0)


def test_misaligned_out_is_refused():
    import torch
    from sin3dm_amd import _lib
    pc = pbr_case()
    ms = pc.sampler()
    face, bary = _dev(pc.face[:16], pc.bary32[:16])
    buf = torch.full((16 * 8 + 4,), -1.0, device="cuda", dtype=torch.float32)
    assert buf.data_ptr() % 16 == 0
    with pytest.raises(AssertionError, match="16-byte aligned"):                            # S3D_ERR_INVALID
        ms.materials8(face, bary, out=buf[1:1 + 16 * 8])
    torch.cuda.synchronize()
    assert (buf == -1).all()                                                                 # nothing was launched
    got = ms.materials8(face, bary, out=buf[4:4 + 16 * 8])                                   # 16 bytes further: aligned
    assert np.array_equal(got.cpu().numpy(), ms.materials8(face, bary).cpu().numpy()) and (buf[:4] == -1).all()
    with pytest.raises(AssertionError):
        _lib.check(_lib.load().s3d_meshsdf_texture_pbr(_lib.ptr(face), _lib.ptr(bary), 16, None, None, 5, None, None, 0, None, 0, _lib.ptr(buf),
                                                       _lib.stream_ptr()))                   # a null face table, as s3d_meshsdf_texture refuses
    assert _lib.load().s3d_meshsdf_texture_pbr(None, None, 0, None, None, 0, None, None, 0, None, 0, None, C.c_void_p(0)) == 0


# ------------------------------------------------------------------ 4: round trip through the exporter
def test_round_trip_through_export_pbr_obj(tmp_path):
    """export_pbr_obj writes row 0 of its arrays as the BOTTOM row of each PNG; the sampler reads the PNGs (row 0 on top) from
    textures/, where the MTL's own entries point as well.  At the centre uv of PNG texel (x, y) materials8 returns that texel."""
    from PIL import Image
    from sin3dm_amd.data.mesh_sampler_pbr import MeshSamplerPBR
    from sin3dm_amd.encoding.isosurface import export_pbr_obj
    T = 8
    maps = {"albedo": coded_rgb(T, T, 1), "metallic": coded_plane(T, T, 2), "roughness": coded_plane(T, T, 3), "normal": coded_rgb(T, T, 4)}
    ys, xs = (a.reshape(-1) for a in np.mgrid[0:T, 0:T])
    n = T * T
    uv = centre_uv(xs, ys, T, T)                                                            # texel (x, y) of the PNG, row 0 on top
    verts = np.stack([np.arange(n)[:, None] + np.array([0.0, 1.0, 0.0])[None], np.tile([0.0, 0.0, 1.0], (n, 1)), np.zeros((n, 3))], -1).reshape(-1, 3)
    tris = np.arange(3 * n).reshape(n, 3)
    path = str(tmp_path / "asset" / "mesh.obj")
    export_pbr_obj(path, verts, tris, np.repeat(uv, 3, 0), maps["albedo"], maps["metallic"], maps["roughness"], maps["normal"])
    png = {k: np.asarray(Image.open(tmp_path / "asset" / "textures" / f"{k}.png")) for k in maps}
    for k in maps:
        assert np.array_equal(png[k], maps[k][::-1])                                        # the writer's bottom-row convention
    ms = MeshSamplerPBR(path)
    assert len(ms.materials) == 1 and ms.fs.shape == (n, 3)
    for field, k in zip(FIELDS, maps):
        assert np.array_equal(ms.materials[0][field], png[k])
    face = np.arange(n, dtype=np.int32)
    for bary in ([1, 0, 0], [0, 0, 1], [0.25, 0.5, 0.25]):
        got = ms.materials8(*_dev(face, np.tile(np.float32(bary), (n, 1)))).cpu().numpy()
        want = np.concatenate([png["albedo"][ys, xs], png["metallic"][ys, xs, None], png["roughness"][ys, xs, None], png["normal"][ys, xs]], 1)
        assert np.array_equal(got, want.astype(np.float32) / np.float32(255)), bary


# ------------------------------------------------------------------ 5: the command line, end to end
def test_cli_end_to_end(tmp_path):
    from PIL import Image
    from sin3dm_amd.data import mesh_sampler, mesh_sampler_pbr
    from sin3dm_amd.data.utils import normalize_aabb, sample_grid_points_aabb
    V0, F = torus()
    V = V0 @ rotation().T * 3.0 + np.array([1.0, -2.0, 0.5])
    lo, hi = V.min(0), V.max(0)
    vt = ((V - lo) / (hi - lo))[:, [0, 2]]
    root = tmp_path / "asset"
    (root / "textures").mkdir(parents=True)
    for name, img in (("albedo", coded_rgb(16, 8, 1)), ("metallic", coded_plane(5, 7, 2)), ("roughness", coded_plane(7, 5, 3)),
                      ("normal", coded_rgb(12, 12, 4))):
        Image.fromarray(img).save(root / "textures" / f"{name}.png")
    (root / "model.mtl").write_text("newmtl red\nKd 0.8 0.1 0.2\nnewmtl blue\nKd 0.1 0.2 0.9\n")
    with open(root / "model.obj", "w") as fh:
        fh.write("mtllib model.mtl\n" + "".join(f"v {x:.9f} {y:.9f} {z:.9f}\n" for x, y, z in V) + "".join(f"vt {u:.9f} {v:.9f}\n" for u, v in vt))
        half = len(F) // 2
        fh.write("usemtl red\n" + "".join(f"f {a + 1}/{a + 1} {b + 1}/{b + 1} {c + 1}/{c + 1}\n" for a, b, c in F[:half]))
        fh.write("usemtl blue\n" + "".join(f"f {a + 1}/{a + 1} {b + 1}/{b + 1} {c + 1}/{c + 1}\n" for a, b, c in F[half:]))
    src = str(root / "model.obj")
    common = ["-s", src, "--reso", "32", "--n_surf", "5000", "--seed", "3"]

    dst = str(tmp_path / "out" / "shape.npz")
    r = subprocess.run([sys.executable, "-m", "sin3dm_amd.data.mesh_sampler_pbr", *common, "-d", dst, "-wt", "--watertight_reso", "7"], cwd=REPO,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    data = np.load(dst)
    assert sorted(data.files) == sorted(mesh_sampler_pbr.KEYS_ALL)
    Vr = np.asarray([[float(x) for x in line.split()[1:]] for line in open(src) if line.startswith("v ")])
    aabb, _, _ = normalize_aabb(Vr, reso=32)
    grid = sample_grid_points_aabb(aabb, 32)
    thr = 2. / 32 * 3
    assert np.array_equal(data["aabb"], aabb) and float(data["threshold"]) == thr and np.array_equal(data["pts_grid"], grid)
    assert data["sdf_grid"].shape == grid.shape[:3] and data["sdf_grid"].dtype == np.float32
    assert data["tex_grid"].shape == grid.shape[:3] + (8,)
    for k, shape in (("tex_grid", grid.shape[:3] + (8,)), ("pts_on_surf", (5000, 3)), ("tex_on_surf", (5000, 8)), ("pts_near_surf", (5000, 3)),
                     ("sdf_near_surf", (5000,)), ("tex_near_surf", (5000, 8))):
        assert data[k].shape == shape and data[k].dtype == np.float32 and np.isfinite(data[k]).all(), k
    sdf = data["sdf_grid"]
    outside = np.abs(sdf) == np.float32(thr)
    assert outside.any() and (~outside).any()
    assert (data["tex_grid"][outside] == 0).all() and (data["tex_grid"][~outside][:, 7] > 0).all()           # the normal map's blue is 204 / 255
    assert (data["tex_on_surf"][:, 7] == np.float32(204) / np.float32(255)).all()
    assert len(np.unique(data["tex_on_surf"][:, 3])) > 10 and len(np.unique(data["tex_on_surf"][:, 4])) > 10   # the planes were read

    # the same seed again, --only_vol and the three-channel command, in this process (the entry point is the same main)
    again, vol, plain = (str(tmp_path / "out" / f"{k}.npz") for k in ("again", "vol", "plain"))
    assert mesh_sampler_pbr.main([*common, "-d", again]) == 0
    assert mesh_sampler_pbr.main([*common, "-d", vol, "--only_vol"]) == 0
    assert mesh_sampler.main([*common, "-d", plain]) == 0
    again, vol, plain = np.load(again), np.load(vol), np.load(plain)
    for k in mesh_sampler_pbr.KEYS_ALL:
        assert np.array_equal(data[k], again[k]), k
    assert sorted(vol.files) == sorted(mesh_sampler_pbr.KEYS_VOL) == sorted(["pts_grid", "sdf_grid", "tex_grid", "aabb", "threshold"])
    assert np.array_equal(vol["sdf_grid"], sdf) and np.array_equal(vol["tex_grid"], data["tex_grid"])
    for k in ("sdf_grid", "pts_on_surf", "sdf_near_surf", "pts_near_surf"):                  # the geometry path is unchanged
        assert np.array_equal(data[k], plain[k]), k
    assert plain["tex_grid"].shape == grid.shape[:3] + (3,) and sorted(plain.files) == sorted(mesh_sampler.KEYS_ALL)
