"""GPU: the textured mesh export — vertex-clustering decimation, texel positions of the per-face atlas, texture
finishing, decode_texmesh and the S3D_MESH=textured CLI — against NumPy restatements and bounds derived from the layout.
Parity with open3d / xatlas / nvdiffrast is not claimed and not tested."""
import math
import os

import numpy as np
import pytest
import torch

from test_texmesh_host import decode_png, parse_obj, rasterise
from texmesh_cases import np_faces

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------ restatements
def _field(kind, n=40):
    """the analytic fields of tests/test_isosurface.py"""
    ax = np.linspace(-1, 1, n)
    x, y, z = np.meshgrid(ax, ax * 0.9, ax * 1.1, indexing="ij")
    if kind == "sphere":
        return (np.sqrt(x * x + y * y + z * z) - 0.7).astype(np.float32)
    if kind == "torus":
        return (np.sqrt((np.sqrt(x * x + y * y) - 0.6) ** 2 + z * z) - 0.22).astype(np.float32)
    if kind == "two":
        a = np.sqrt((x - 0.45) ** 2 + y * y + z * z) - 0.3
        b = np.sqrt((x + 0.45) ** 2 + y * y + z * z) - 0.35
        return np.minimum(a, b).astype(np.float32)
    raise KeyError(kind)


def _mesh(kind):
    from sin3dm_amd.encoding.isosurface import marching_cubes
    v, t, _ = marching_cubes(torch.from_numpy(_field(kind)).cuda(), 0.0, 1.0)
    return v, t


def np_cluster_keys(v, R):
    """float32 restatement of the grid: s = fp32(extent_max / R), cells per axis min(R, max(1, ceil(extent / s))),
    index min(R_axis - 1, floor((v - lo) / s)), key = (ix * Ry + iy) * Rz + iz"""
    v = v.astype(np.float32)
    lo = v.min(0)
    ext = v.max(0) - lo
    s = np.float32(ext.max()) / np.float32(R)
    dims = np.asarray([min(R, max(1, math.ceil(float(np.float32(e) / s)))) for e in ext], np.int64)
    idx = np.minimum(dims - 1, np.floor((v - lo) / s).astype(np.int64))
    return (idx[:, 0] * dims[1] + idx[:, 1]) * dims[2] + idx[:, 2], s, dims, lo, ext


def signed_volume(v, t):
    a, b, c = v[t[:, 0]], v[t[:, 1]], v[t[:, 2]]
    return float(np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6)


# ------------------------------------------------------------------ simplify_mesh
@pytest.mark.parametrize("n_faces", [200, 1000])
@pytest.mark.parametrize("kind", ["sphere", "torus", "two"])
def test_simplify_mesh(kind, n_faces):
    from sin3dm_amd.encoding.isosurface import simplify_mesh
    v, t = _mesh(kind)
    attrs = torch.sin(v * 0.37 + 1.0)[:, :2].contiguous()
    v2, t2, info = simplify_mesh(v, t, n_faces, attrs=attrs)
    vn, tn = v.cpu().numpy(), t.cpu().numpy()
    v2n, t2n = v2.cpu().numpy(), t2.cpu().numpy()
    vmap = info["vmap"].cpu().numpy().astype(np.int64)
    assert len(tn) > n_faces                                             # (the input is over the budget: something happens)
    assert len(t2n) <= n_faces and t2.dtype == torch.int32 and v2.dtype == torch.float32
    assert info["R"] == info["lo"] >= 1
    # the next finer grid is over the budget (bisection invariant), recomputed in NumPy
    k1 = np_cluster_keys(vn, info["lo"] + 1)[0]
    n1 = len(np_faces(tn, np.unique(k1, return_inverse=True)[1]))
    print(f"{kind} n_faces={n_faces}: input {len(tn)} faces, R={info['lo']} -> {len(t2n)} faces, R+1 -> {n1}")
    assert n1 > n_faces
    # every vertex lies in the cell of its cluster (cell boundaries widened by 1e-5 extent_max), clusters numbered by ascending key
    key, s, dims, lo, ext = np_cluster_keys(vn, info["lo"])
    dkey = info["keys"].cpu().numpy()
    assert abs(info["s"] - float(s)) == 0 and list(info["dims"]) == dims.tolist()
    cell = np.stack([dkey // (dims[1] * dims[2]), (dkey // dims[2]) % dims[1], dkey % dims[2]], 1)
    assert (cell >= 0).all() and (cell < dims).all()
    eps = 1e-5 * float(ext.max())
    rel = vn.astype(np.float64) - lo.astype(np.float64)
    upper = np.where(cell == dims - 1, np.inf, (cell + 1) * float(s))    # the last cell of an axis takes what is beyond it
    assert (rel >= cell * float(s) - eps).all() and (rel <= upper + eps).all()
    assert np.array_equal(vmap, np.unique(dkey, return_inverse=True)[1])
    # faces: exactly the NumPy remap / drop / dedupe through vmap, then unreferenced clusters dropped
    fn = np_faces(tn, vmap)
    used = np.unique(fn)
    assert np.array_equal(t2n, np.searchsorted(used, fn))
    assert len(v2n) == len(used) and np.array_equal(np.unique(t2n), np.arange(len(v2n)))
    # vertices: float64 means of the members
    cnt = np.bincount(vmap, minlength=vmap.max() + 1).astype(np.float64)
    for vals, got in ((vn, v2n), (attrs.cpu().numpy(), info["attrs"].cpu().numpy())):
        mean = np.stack([np.bincount(vmap, weights=vals[:, j].astype(np.float64), minlength=len(cnt)) / cnt for j in range(vals.shape[1])], 1)
        err = np.abs(got - mean[used]).max()
        print(f"  mean error {err:.3e} (bound {eps:.3e}), largest cluster {int(cnt.max())}")
        assert err <= eps
    if kind == "sphere":
        assert signed_volume(v2n.astype(np.float64), t2n) > 0
    # a mesh under the budget comes back as it is
    v3, t3, info3 = simplify_mesh(v2, t2, n_faces)
    assert torch.equal(v3, v2) and torch.equal(t3, t2)
    assert np.array_equal(info3["vmap"].cpu().numpy(), np.arange(len(v2n)))


# ------------------------------------------------------------------ bake_texture
@pytest.fixture(scope="module")
def small_sphere():
    from sin3dm_amd.encoding.isosurface import simplify_mesh
    v, t = _mesh("sphere")
    v = v / 39.0 * 2.0 - 1.0 + torch.tensor([0.3, -0.2, 0.1], device=v.device)      # off-centre, so that max|v| is not symmetric
    v2, t2, _ = simplify_mesh(v.contiguous(), t, 1000)
    assert 300 < len(t2) <= 1000
    return v2, t2


def _chart_frames(F, T, n, c):
    """origin [F,2] and corners [F,3,2] of every face's chart in texels, restated from the layout"""
    k = np.arange(F)
    cell = k // 2
    org = np.stack([(cell % n) * c, (cell // n) * c], 1)
    lower = np.asarray([[1, 1], [c - 4, 1], [1, c - 4]])
    upper = np.asarray([[c - 1, c - 1], [4, c - 1], [c - 1, 4]])
    return org, org[:, None, :] + np.where((k % 2 == 0)[:, None, None], lower[None], upper[None])


def test_texel_positions_and_mask(small_sphere):
    from sin3dm_amd.encoding.isosurface import atlas_texels, bake_texture
    v, t = small_sphere
    T = 512
    vn, tn = v.cpu().numpy().astype(np.float64), t.cpu().numpy()
    F = len(tn)
    face_ref, claims, n, c = rasterise(F, T)
    L = c - 5
    face_id, pos, corner0, atlas = atlas_texels(v, t, T)
    fid = face_id.cpu().numpy().reshape(T, T)
    assert np.array_equal(fid, face_ref)
    image, mask, gb_pos, uvs, corner0b = bake_texture(v, t, T, lambda p: 0.5 + 0.0 * p)
    assert np.array_equal(mask.cpu().numpy(), face_ref >= 0) and torch.equal(corner0b, corner0)
    assert torch.equal(gb_pos.view(-1, 3), pos) and image.shape == (T, T, 3) and image.dtype == torch.uint8
    r = corner0.cpu().numpy().astype(np.int64)
    assert r.min() >= 0 and r.max() <= 2
    # corner 0 sits opposite the longest edge
    elen = np.stack([np.linalg.norm(vn[tn[:, (j + 1) % 3]] - vn[tn[:, j]], axis=1) for j in range(3)], 1)      # v0v1, v1v2, v2v0
    opposite = elen[np.arange(F), (r + 1) % 3]                            # the edge from vertex r+1 to vertex r+2
    assert (opposite >= (1 - 1e-6) * elen.max(1)).all()
    # positions: float64 barycentric formula
    ys, xs = np.nonzero(face_ref >= 0)
    k = face_ref[ys, xs]
    org, corners = _chart_frames(F, T, n, c)
    lx, ly = xs - org[k, 0], ys - org[k, 1]
    low = k % 2 == 0
    b1 = np.where(low, lx + 0.5 - 1, c - 1 - (lx + 0.5)) / L
    b2 = np.where(low, ly + 0.5 - 1, c - 1 - (ly + 0.5)) / L
    b0 = 1 - b1 - b2
    assert b0.min() >= -1e-12 and b1.min() > 0 and b2.min() > 0
    V = [vn[tn[k, (r[k] + j) % 3]] for j in range(3)]
    want = b0[:, None] * V[0] + b1[:, None] * V[1] + b2[:, None] * V[2]
    got = gb_pos.cpu().numpy()[ys, xs].astype(np.float64)
    M = np.abs(vn).max()
    err = np.abs(got - want).max()
    print(f"F={F} n={n} c={c}: position error {err:.3e} (bound {1e-6 * M:.3e})")
    assert err <= 1e-6 * M
    assert (gb_pos.cpu().numpy()[face_ref < 0] == 0).all()
    # uvs: vertex j of face k shows chart corner (j - corner0) mod 3
    which = (np.arange(3)[None, :] - r[:, None]) % 3
    assert np.allclose(uvs.cpu().numpy().reshape(F, 3, 2) * T, np.take_along_axis(corners, which[:, :, None], 1), atol=1e-4)


def test_bake_texture_colours(small_sphere):
    from sin3dm_amd.encoding.isosurface import bake_texture
    v, t = small_sphere
    T = 512
    vn, tn = v.cpu().numpy().astype(np.float64), t.cpu().numpy()
    F = len(tn)
    M = float(np.abs(vn).max())
    decode_fn = lambda p: 0.5 + 0.25 * p / M
    calls = []

    def counted(p):
        calls.append(p.shape[0])
        return decode_fn(p)
    image, mask, gb_pos, uvs, corner0 = bake_texture(v, t, T, counted)
    face_ref, _, n, c = rasterise(F, T)
    L = c - 5
    assert calls == [int((face_ref >= 0).sum())]                            # one decode call over the covered texels
    img = image.cpu().numpy()
    m = mask.cpu().numpy()
    want = (decode_fn(gb_pos[mask]) * 255.0).clamp(0, 255).to(torch.uint8).cpu().numpy()
    assert np.array_equal(img[m], want)
    q = np.zeros((T + 2, T + 2, 3), np.uint8)
    q[1:-1, 1:-1][m] = want
    dil = np.max([q[1 + dy:T + 1 + dy, 1 + dx:T + 1 + dx] for dy in (-1, 0, 1) for dx in (-1, 0, 1)], axis=0)
    assert np.array_equal(img[~m], dil[~m])
    assert (dil[~m].max(1) > 0).any() and (img[~m] == 0).any()              # gutters are filled, far texels stay black
    # what a viewer samples: the texel under uv(p') for random interior points p'
    rng = np.random.Generator(np.random.PCG64(11))
    N = 10000
    k = rng.integers(0, F, N)
    b = rng.dirichlet(np.ones(3), N)
    assert (b > 0).all()
    r = corner0.cpu().numpy().astype(np.int64)
    _, corners = _chart_frames(F, T, n, c)
    V = [vn[tn[k, (r[k] + j) % 3]] for j in range(3)]                       # chart corner j shows vertex (corner0 + j) mod 3
    p = b[:, :1] * V[0] + b[:, 1:2] * V[1] + b[:, 2:] * V[2]
    uv = (b[:, :, None] * corners[k]).sum(1)
    x, y = np.floor(uv[:, 0]).astype(np.int64), np.floor(uv[:, 1]).astype(np.int64)
    assert np.array_equal(face_ref[y, x], k)                                # the containing texel is covered, by that face
    colour = img[y, x].astype(np.float64) / 255.0
    legs = np.linalg.norm(V[1] - V[0], axis=1) + np.linalg.norm(V[2] - V[0], axis=1)
    bound = 0.25 / M * 0.5 * legs / L + 1.0 / 255.0
    diff = np.abs(colour - (0.5 + 0.25 * p / M)).max(1)
    print(f"F={F} c={c} L={L}: worst colour error / bound = {(diff / bound).max():.3f}")
    assert (diff <= bound).all()


# ------------------------------------------------------------------ decode_texmesh and the CLI
@pytest.fixture(scope="module")
def sampled(tmp_path_factory):
    """an experiment directory and one sampled triplane; the run leaves the DEFAULT mesh output behind (no S3D_MESH)"""
    from test_cli_gpu import make_experiment
    from sin3dm_amd import sample
    tag = make_experiment(str(tmp_path_factory.mktemp("texmesh")))
    with pytest.MonkeyPatch.context() as mp:
        mp.delenv("S3D_MESH", raising=False)
        paths = sample.main(["--tag", tag, "--n_samples", "1", "--use_ddim", "True", "--timestep_respacing", "5", "--reso", "48",
                             "--n_faces", "2000", "--texreso", "512"])
    return tag, paths[0]


def _autoencoder(tag):
    from sin3dm_amd.encoding.model import ShapeAutoEncoder
    from sin3dm_amd.utils import parser_util as pu
    args = pu.sample_args(["--tag", tag])
    ae = ShapeAutoEncoder(pu.encoding_log_dir(tag), args, device=torch.device("cuda:0"))
    ae.load_ckpt("final")
    return ae


def _check_textured_obj(folder, T, aabb_lo, aabb_hi, reso, n_faces):
    pv, pvt, pf, other = parse_obj(os.path.join(folder, "object.obj"))
    assert other == ["mtllib object.mtl", "usemtl material_0"]
    assert 0 < len(pf) <= n_faces and pf.shape[1:] == (3, 2) and len(pvt) == 3 * len(pf)
    assert pf[:, :, 0].min() >= 1 and pf[:, :, 0].max() <= len(pv) and np.array_equal(pf[:, :, 1].reshape(-1), np.arange(3 * len(pf)) + 1)
    assert pv.shape[1] == 3 and pvt.min() >= 0 and pvt.max() <= 1
    cell = (aabb_hi - aabb_lo).max() / reso
    assert (pv >= aabb_lo - cell).all() and (pv <= aabb_hi + cell).all()
    mtl = [l.strip() for l in open(os.path.join(folder, "object.mtl"))]
    assert mtl[0] == "newmtl material_0" and mtl[-1] == "map_Kd object.png" and "illum 2" in mtl
    assert any(l.startswith("Kd ") for l in mtl)
    png = decode_png(open(os.path.join(folder, "object.png"), "rb").read())
    assert png.shape == (T, T, 3)
    return pv, pvt, pf, png


def test_decode_texmesh(sampled, tmp_path):
    from sin3dm_amd.utils.triplane_util import load_triplane_data
    tag, feat = sampled
    ae = _autoencoder(tag)
    fm = [f.unsqueeze(0) for f in load_triplane_data(feat, device="cuda:0", compose=False)]
    out_dir = str(tmp_path / "obj")
    out = ae.decode_texmesh(out_dir, fm, 48, n_faces=2000, texture_reso=512)
    assert out is not None and sorted(os.listdir(out_dir)) == ["object.mtl", "object.obj", "object.png", "voxel.npz"]
    H, W = fm[0].shape[-2:]
    aabb = ae._resize_aabb((H, W, fm[1].shape[-1]))
    mask, image = out["mask"], out["image"]
    assert 0 < len(out["tris"]) <= 2000 and int(mask.sum()) > 0
    cols = ae.decode_batch(fm, out["gb_pos"][mask], aabb=aabb)[..., 1:]
    want = (cols * 255.0).clamp(0, 255).to(torch.uint8)
    assert torch.equal(image[mask], want)                                   # same kernel, same inputs
    lo, hi = aabb[:3].cpu().numpy().astype(np.float64), aabb[3:].cpu().numpy().astype(np.float64)
    pv, pvt, pf, png = _check_textured_obj(out_dir, 512, lo, hi, 48, 2000)
    assert np.array_equal(png, image.cpu().numpy()[::-1])
    assert np.allclose(pv, out["verts"].cpu().numpy(), atol=1e-6) and np.array_equal(pf[:, :, 0], out["tris"].cpu().numpy() + 1)
    assert np.allclose(pvt, out["uvs"].cpu().numpy(), atol=1e-6)
    assert np.load(os.path.join(out_dir, "voxel.npz"))["vox_grid"].dtype == bool
    # glb: only object.glb; same texture
    import json
    import struct
    glb_dir = str(tmp_path / "glb")
    out2 = ae.decode_texmesh(glb_dir, fm, 48, n_faces=2000, texture_reso=512, save_voxel=False, file_format="glb")
    assert os.listdir(glb_dir) == ["object.glb"] and torch.equal(out2["image"], image)
    data = open(os.path.join(glb_dir, "object.glb"), "rb").read()
    magic, version, total = struct.unpack("<III", data[:12])
    jlen = struct.unpack("<I", data[12:16])[0]
    g = json.loads(data[20:20 + jlen])
    assert magic == 0x46546C67 and version == 2 and total == len(data)
    assert g["accessors"][0]["count"] == g["accessors"][1]["count"] == 3 * len(out2["tris"])
    bv = g["bufferViews"][g["images"][0]["bufferView"]]
    blob = data[28 + jlen:]
    assert blob[bv["byteOffset"]:bv["byteOffset"] + bv["byteLength"]] == open(os.path.join(out_dir, "object.png"), "rb").read()
    with pytest.raises(NotImplementedError):
        ae.decode_texmesh(glb_dir, fm, 48, file_format="ply")
    with pytest.raises(ValueError) as e:                                    # 2000 faces do not fit a 64-texel atlas
        ae.decode_texmesh(str(tmp_path / "small"), fm, 48, n_faces=2000, texture_reso=64)
    assert "--texreso" in str(e.value)


def test_sample_cli_textured(sampled, monkeypatch):
    from sin3dm_amd import sample
    tag, feat = sampled
    # the default run of the fixture: six-column vertex-coloured OBJ, nothing else
    plain = os.path.dirname(feat)
    assert not os.path.exists(os.path.join(plain, "object.mtl")) and not os.path.exists(os.path.join(plain, "object.png"))
    rows = [l.split() for l in open(os.path.join(plain, "object.obj"))]
    assert {r[0] for r in rows} == {"v", "f"} and all(len(r) == 7 for r in rows if r[0] == "v")
    assert all(len(r) == 4 and "/" not in "".join(r) for r in rows if r[0] == "f")
    monkeypatch.setenv("S3D_MESH", "textured")
    paths = sample.main(["--tag", tag, "--n_samples", "1", "--use_ddim", "True", "--timestep_respacing", "5", "--reso", "48",
                         "--n_faces", "2000", "--texreso", "512", "--output", "textured"])
    folder = os.path.dirname(paths[0])
    assert {"object.obj", "object.mtl", "object.png"} <= set(os.listdir(folder))
    lo, hi = np.asarray([-0.72, -1.0, -0.72]), np.asarray([0.72, 1.0, 0.72])
    pv, pvt, pf, png = _check_textured_obj(folder, 512, lo, hi, 48, 2000)
    assert len(pvt) > 0 and png.max() > 0
    monkeypatch.setenv("S3D_MESH", "foo")
    with pytest.raises(ValueError):
        sample.decode(None, [])
