"""GPU tests of the mesh preprocessing (sin3dm_amd/data, s3d_meshsdf.hip) against a float64 NumPy brute force (tests/meshprep_cases.py):
all points x all faces with the kernels' formulas (Ericson's region test, the Van Oosterom-Strackee solid angle).

Tolerances.  The same brute force run in float32 (`python tests/meshprep_cases.py` prints the figures, CPU only) differs from
float64, over every mesh and query set used below, by at most
    FP32_GAP_DIST = 1.3e-7 in the distance (measured 1.288e-7)   and   FP32_GAP_WN = 8.4e-7 in the winding number (8.345e-7);
the device is allowed 8x that (FMA contraction, device sqrt, division and atan2): TOL_DIST = 1.04e-6, TOL_WN = 6.72e-6.
"""
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO
from meshprep_cases import (FP32_GAP_DIST, FP32_GAP_WN, R_MAJOR, R_MINOR, TOL_DIST, TOL_WN, Case, box_mesh, brute_closest,  # noqa: F401
                            brute_winding, case, check_closest, pair_closest, rotation, torus)


def torus_phi(p0):
    """Signed distance to the analytic torus in its own frame."""
    return np.sqrt((np.sqrt(p0[..., 0] ** 2 + p0[..., 2] ** 2) - R_MAJOR) ** 2 + p0[..., 1] ** 2) - R_MINOR


pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------ 1, 2: closest point
@pytest.mark.parametrize("band", [0.25, 0.05])
def test_closest_point(band):
    """Grid, 1000 random points (some outside the aabb) and points exactly on vertices, edge midpoints and centroids; band 0.05
    leaves most cells empty.  Tolerance 8 x FP32_GAP_DIST (module docstring: fp32 NumPy vs float64 1.3e-7 -> 1.04e-6)."""
    c = case()
    d_or, _ = c.memo("closest", lambda: brute_closest(c.queries.astype(np.float64), c.T))
    dist, face, _ = check_closest(c.sampler(), c.T, c.queries, d_or, band)
    assert (face >= 0).sum() > 500 and (face < 0).sum() > 500


def test_closest_point_large_triangles():
    """A 12-triangle box that fills the aabb: every triangle spans most cells of the grid."""
    from sin3dm_amd.data.mesh_sampler import MeshSampler
    c = case()
    d_or, _ = brute_closest(c.queries.astype(np.float64), c.box_T)
    ms = MeshSampler(verts=c.box_V.astype(np.float32).astype(np.float64), faces=c.box_F)
    for band in (0.25, 0.05):
        check_closest(ms, c.box_T, c.queries, d_or, band)


# ------------------------------------------------------------------ 3: winding number
def test_winding_number():
    """Closed torus (9216 + 7 points: no multiple of the block), the torus with 40 faces removed, one triangle, the flipped torus.
    Tolerance 8 x FP32_GAP_WN (module docstring: fp32 NumPy vs float64 8.4e-7 -> 6.72e-6)."""
    from sin3dm_amd.data.mesh_sampler import MeshSampler
    c = case()
    P = c.wn_points
    flipped = c.F[:, ::-1].copy()
    masks, closed_or = {}, None
    for name, F, max_excluded in (("closed", c.F, 0.0), ("open", c.F[c.open_keep], 0.01), ("triangle", c.F[:1], 1.0), ("flipped", flipped, 0.0)):
        T = c.V32[F].reshape(-1, 9).astype(np.float64)
        # (reversing every face negates every solid angle exactly)
        wn_or = -closed_or if name == "flipped" else brute_winding(P.astype(np.float64), T)
        closed_or = wn_or if name == "closed" else closed_or
        sure = np.abs(np.abs(wn_or) - 0.5) > 10 * TOL_WN
        assert 1 - sure.mean() <= max_excluded, (name, 1 - sure.mean())            # the oracle alone: the mask is decided almost everywhere
        wn = MeshSampler(verts=c.V32.astype(np.float64), faces=F).winding_number(P).cpu().numpy()
        err = np.abs(wn - wn_or).max()
        print(f"{name}: {len(F)} faces, winding number error max {err:.3e} (tol {TOL_WN:.3e}), undecided share {1 - sure.mean():.4f}, "
              f"range [{wn_or.min():.3f}, {wn_or.max():.3f}]")
        assert err <= TOL_WN, name
        masks[name] = np.abs(wn) >= 0.5
        assert np.array_equal(masks[name][sure], (np.abs(wn_or) >= 0.5)[sure]), name
    assert np.array_equal(masks["closed"], masks["flipped"])
    assert 0 < masks["closed"].sum() < len(P) and masks["triangle"].sum() == 0


# ------------------------------------------------------------------ 4: the signed grid against the analytic torus
def test_signed_grid_against_the_analytic_torus():
    """|sdf_grid - clip(phi)| <= 2 h + tol, h = the mesh's sag: the largest |phi| over a 10 x 10 barycentric lattice on every face
    (float64); the factor 2 covers both directions of the Hausdorff distance.  The float64 oracle must satisfy the bound first."""
    c = case()
    P = c.grid.reshape(-1, 3).astype(np.float32)
    phi = np.clip(torus_phi(c.to_torus_frame(P)) * c.scale, -c.band, c.band)
    lat = np.array([[i, j, 9 - i - j] for i in range(10) for j in range(10 - i)], dtype=np.float64) / 9
    h = float(np.abs(torus_phi(c.to_torus_frame(np.einsum("lk,fkd->fld", lat, c.V32[c.F].astype(np.float64))))).max() * c.scale)
    d_or = c.memo("closest", lambda: brute_closest(c.queries.astype(np.float64), c.T))[0][:len(P)]       # the queries start with the grid
    wn_or = brute_winding(P.astype(np.float64), c.T)
    sdf_or = np.where(np.abs(wn_or) >= 0.5, -1, 1) * np.minimum(d_or, c.band)
    print(f"sag h = {h:.5f}; oracle vs analytic {np.abs(sdf_or - phi).max():.5f} (bound {2 * h:.5f})")
    assert np.abs(sdf_or - phi).max() <= 2 * h
    sdf = c.sampler().query_sdf(P, c.band).cpu().numpy()
    print(f"device vs analytic {np.abs(sdf - phi).max():.5f}; device vs oracle {np.abs(sdf - sdf_or).max():.3e}")
    assert np.abs(sdf - phi).max() <= 2 * h + TOL_DIST
    assert (sdf < 0).sum() > 50 and np.abs(sdf).max() <= np.float32(c.band)


# ------------------------------------------------------------------ 5: texture
def test_texture():
    """uv = ((x + 1) / 2, (z + 1) / 2) of the position, so a tie between faces does not change the texel; material 0 (faces whose
    centroid has x < 0) has a 16 x 8 image whose texel holds its own (x, y), material 1 only a Kd.  The expected colour is computed
    in float64 from the closest point on the face the device reports, after that face is checked to be at the brute-force minimum
    (a tie between faces of two materials is decided by rounding, not by the formulas).  Queries whose float64 texel coordinate is
    within 1e-3 of a half-integer are left out: at most 2 % of them."""
    c = case()
    W, H = 16, 8
    img = np.zeros((H, W, 3), dtype=np.uint8)
    img[..., 0] = np.arange(W)[None, :] * 16
    img[..., 1] = np.arange(H)[:, None] * 32
    img[..., 2] = 7
    kd1 = (0.25, 0.5, 0.125)
    tri = c.V32[c.F].astype(np.float64)
    face_mat = (tri.mean(1)[:, 0] >= 0).astype(np.int32)
    uvs = np.stack([(tri[..., 0] + 1) / 2, (tri[..., 2] + 1) / 2], -1)
    ms = c.sampler(uvs=uvs, face_mat=face_mat, materials=[{"Kd": (1.0, 0.0, 1.0), "image": img}, {"Kd": kd1}])
    rng = np.random.Generator(np.random.PCG64(5))
    bc = rng.dirichlet(np.ones(3), size=3000)
    on = np.einsum("nk,nkd->nd", bc, tri[rng.integers(0, len(c.F), size=3000)])
    G = c.grid.reshape(-1, 3)
    P = np.concatenate([G, on + 0.01 * rng.standard_normal(on.shape)]).astype(np.float32)
    dist, face, bary = (t.cpu().numpy() for t in ms.closest(P, c.band))
    col = ms.query_tex(P, c.band).cpu().numpy()
    assert col.dtype == np.float32 and col.shape == (len(P), 3)
    d_or = np.concatenate([c.memo("closest", lambda: brute_closest(c.queries.astype(np.float64), c.T))[0][:len(G)],
                           brute_closest(P[len(G):].astype(np.float64), c.T)[0]])
    hit = face >= 0
    assert (col[~hit] == 0).all() and hit[d_or < c.band - TOL_DIST].all() and (~hit[d_or >= c.band + TOL_DIST]).all()
    Ph, fh = P[hit].astype(np.float64), face[hit]
    d_face, b64 = pair_closest(Ph, c.T[fh])
    assert np.max(d_face - d_or[hit]) <= TOL_DIST
    cp = np.einsum("nk,nkd->nd", b64, tri[fh])
    tx, ty = (cp[:, 0] + 1) / 2 * (W - 1), (1 - (cp[:, 2] + 1) / 2) * (H - 1)
    m0 = face_mat[fh] == 0
    edge = m0 & ((np.abs(tx - np.floor(tx) - 0.5) < 1e-3) | (np.abs(ty - np.floor(ty) - 0.5) < 1e-3))
    print(f"{hit.sum()} coloured queries, {m0.sum()} on the image, {edge.sum()} left out near a texel border")
    assert edge.mean() <= 0.02 and m0.sum() > 500 and (~m0).sum() > 500
    expect = np.empty((len(fh), 3), dtype=np.float32)
    expect[:] = np.asarray(kd1, dtype=np.float32)
    xi, yi = np.round(tx).astype(np.int64) % W, np.round(ty).astype(np.int64) % H
    expect[m0] = img[yi[m0], xi[m0]].astype(np.float32) / np.float32(255)
    assert np.array_equal(col[hit][~edge], expect[~edge])


# ------------------------------------------------------------------ 6: surface samples
def test_surface_sampling():
    import torch
    c = case()
    tri = c.V32[c.F].astype(np.float64)
    ms = c.sampler()
    n = 20000

    def draw():
        g = torch.Generator(device="cuda")
        g.manual_seed(1234)
        return [t.cpu().numpy() for t in ms.sample_surf(n, g)]
    pts, face, bary = draw()
    again = draw()
    assert all(np.array_equal(a, b) for a, b in zip((pts, face, bary), again))
    assert pts.shape == (n, 3) and face.min() >= 0 and face.max() < len(c.F) and (bary >= 0).all()
    d, _ = pair_closest(pts.astype(np.float64), c.T[face])
    recon = np.einsum("nk,nkd->nd", bary.astype(np.float64), tri[face])
    print(f"samples off their face by {d.max():.3e}, off sum bary v by {np.abs(recon - pts).max():.3e}")
    assert d.max() <= TOL_DIST and np.abs(recon - pts).max() <= TOL_DIST
    area = 0.5 * np.linalg.norm(np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]), axis=1)
    region = tri.mean(1)[:, 0] >= 0                                # the two material regions of the texture test
    p = area[region].sum() / area.sum()
    got = region[face].mean()
    sigma = np.sqrt(p * (1 - p) / n)
    print(f"share of samples in region 1: {got:.4f}, area share {p:.4f}, sigma {sigma:.4f}")
    assert abs(got - p) <= 5 * sigma
    assert abs(bary[:, 0].mean() - 1 / 3) < 0.01 and abs(bary[:, 1].mean() - 1 / 3) < 0.01     # uniform inside a face: mean 1/3, sd 0.24/sqrt(n)


# ------------------------------------------------------------------ 7: the command line, end to end
def test_cli_end_to_end(tmp_path):
    import torch
    from types import SimpleNamespace
    from sin3dm_amd.data.mesh_sampler import KEYS_ALL, KEYS_VOL
    from sin3dm_amd.data.utils import normalize_aabb, sample_grid_points_aabb
    from sin3dm_amd.encoding.model import ShapeAutoEncoder
    V0, F = torus()
    V = V0 @ rotation().T * 3.0 + np.array([1.0, -2.0, 0.5])
    with open(tmp_path / "model.mtl", "w") as fh:
        fh.write("newmtl red\nKa 0.1 0.1 0.1\nKd 0.8 0.1 0.2\nKs 0.5 0.5 0.5\nNs 96\nnewmtl blue\nKd 0.1 0.2 0.9\n")
    with open(tmp_path / "model.obj", "w") as fh:
        fh.write("mtllib model.mtl\n" + "".join(f"v {x:.9f} {y:.9f} {z:.9f}\n" for x, y, z in V))
        half = len(F) // 2
        fh.write("usemtl red\n" + "".join(f"f {a + 1} {b + 1} {c + 1}\n" for a, b, c in F[:half]))
        fh.write("usemtl blue\n" + "".join(f"f {a + 1} {b + 1} {c + 1}\n" for a, b, c in F[half:]))

    def run(*extra):
        dst = str(tmp_path / f"out{len(extra)}" / "shape.npz")
        r = subprocess.run([sys.executable, "-m", "sin3dm_amd.data.mesh_sampler", "-s", str(tmp_path / "model.obj"), "-d", dst, "--reso", "32",
                            "--n_surf", "5000", *extra], cwd=REPO, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
        return dst, np.load(dst)

    path, data = run()
    assert sorted(data.files) == sorted(KEYS_ALL)
    Vr = np.asarray([[float(x) for x in line.split()[1:]] for line in open(tmp_path / "model.obj") if line.startswith("v ")])
    aabb, _, _ = normalize_aabb(Vr, reso=32)
    grid = sample_grid_points_aabb(aabb, 32)
    thr = 2. / 32 * 3
    assert np.array_equal(data["aabb"], aabb) and float(data["threshold"]) == thr and np.array_equal(data["pts_grid"], grid)
    assert data["sdf_grid"].shape == grid.shape[:3] and data["sdf_grid"].dtype == np.float32
    assert data["tex_grid"].shape == grid.shape and data["tex_grid"].dtype == np.float32
    for k, shape in (("pts_on_surf", (5000, 3)), ("tex_on_surf", (5000, 3)), ("pts_near_surf", (5000, 3)), ("sdf_near_surf", (5000,)),
                     ("tex_near_surf", (5000, 3))):
        assert data[k].shape == shape and data[k].dtype == np.float32 and np.isfinite(data[k]).all(), k
    sdf = data["sdf_grid"]
    assert np.abs(sdf).max() == np.float32(thr) and (sdf < 0).any() and (sdf > 0).any()
    outside = np.abs(sdf) == np.float32(thr)
    assert (data["tex_grid"][outside] == 0).all() and (data["tex_grid"][~outside].max(-1) > 0).all()
    colours = {tuple(round(float(x), 4) for x in c) for c in np.unique(data["tex_on_surf"], axis=0)}
    assert colours == {(0.8, 0.1, 0.2), (0.1, 0.2, 0.9)}
    assert (data["pts_near_surf"] >= aabb[:3].astype(np.float32)).all() and (data["pts_near_surf"] <= aabb[3:].astype(np.float32)).all()
    assert np.allclose(data["Kd"], (0.8, 0.1, 0.2)) and np.allclose(data["Ka"], 0.1) and float(data["Ns"]) == 96
    _, vol = run("--only_vol")
    assert sorted(vol.files) == sorted(KEYS_VOL) and np.array_equal(vol["sdf_grid"], sdf)

    cfg = SimpleNamespace(enc_net_type="skip", fdim_geo=4, fdim_tex=8, fdim_up=64, hidden_dim=256, n_hidden_layers=4, data_type="sdftex",
                          enc_batch_size=2048, enc_n_iters=60, vol_ratio=0.1, fm_reso=32, sdf_loss="weightedl1", tex_loss="l1",
                          tex_weight=1.0, tex_threshold_ratio=0.999, sdf_renorm=0, enc_lr=5e-3, enc_lr_split=0.2, enc_lr_decay=0.1, gpu_id=0)
    ae = ShapeAutoEncoder(str(tmp_path / "encoding"), cfg)
    ae._load_data(path)
    assert ae.sdf_threshold == thr and tuple(ae.pts_near_surf.shape) == (5000, 3)
    ae.net.reset_aabb(ae.aabb)
    ae._set_optimizer(ae.init_lr, ae.min_lr_ratio)
    for i in range(3):
        ae.step = i
        losses = ae.train_step(ae._sample_batch(ae.batch_size))
        assert all(np.isfinite(float(v)) for v in losses.values()), losses
    torch.cuda.synchronize()
