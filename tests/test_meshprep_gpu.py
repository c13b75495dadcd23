"""GPU tests of the mesh preprocessing (sin3dm_amd/data, s3d_meshsdf.hip) against a float64 NumPy brute force written here: all
points x all faces with the kernels' formulas (Ericson's region test, the Van Oosterom-Strackee solid angle).

Tolerances.  The same brute force run in float32 (`python tests/test_meshprep_gpu.py` prints the figures, CPU only) differs from
float64, over every mesh and query set used below, by at most
    FP32_GAP_DIST = 1.3e-7 in the distance (measured 1.288e-7)   and   FP32_GAP_WN = 8.4e-7 in the winding number (8.345e-7);
the device is allowed 8x that (FMA contraction, device sqrt, division and atan2): TOL_DIST = 1.04e-6, TOL_WN = 6.72e-6.
"""
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO

FP32_GAP_DIST, FP32_GAP_WN = 1.3e-7, 8.4e-7
TOL_DIST, TOL_WN = 8 * FP32_GAP_DIST, 8 * FP32_GAP_WN
R_MAJOR, R_MINOR = 0.55, 0.22


# ------------------------------------------------------------------ meshes
def torus(nu=24, nv=12):
    """Vertices [nu * nv, 3] on the torus around the y axis and 2 * nu * nv outward-oriented faces."""
    u, v = np.meshgrid(np.arange(nu) * 2 * np.pi / nu, np.arange(nv) * 2 * np.pi / nv, indexing="ij")
    V = np.stack([(R_MAJOR + R_MINOR * np.cos(v)) * np.cos(u), R_MINOR * np.sin(v), (R_MAJOR + R_MINOR * np.cos(v)) * np.sin(u)], -1).reshape(-1, 3)
    F = []
    for i in range(nu):
        for j in range(nv):
            a, b, c, d = i * nv + j, ((i + 1) % nu) * nv + j, ((i + 1) % nu) * nv + (j + 1) % nv, i * nv + (j + 1) % nv
            F += [[a, c, b], [a, d, c]]
    return V, np.asarray(F, dtype=np.int64)


def rotation():
    cz, sz, cx, sx = np.cos(0.3), np.sin(0.3), np.cos(0.2), np.sin(0.2)
    return np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]) @ np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])


def torus_phi(p0):
    """Signed distance to the analytic torus in its own frame."""
    return np.sqrt((np.sqrt(p0[..., 0] ** 2 + p0[..., 2] ** 2) - R_MAJOR) ** 2 + p0[..., 1] ** 2) - R_MINOR


def box_mesh(aabb):
    lo, hi = aabb[:3], aabb[3:]
    V = np.array([[(lo, hi)[(i >> k) & 1][k] for k in range(3)] for i in range(8)], dtype=np.float64)
    F = [[0, 2, 1], [1, 2, 3], [4, 5, 6], [5, 7, 6], [0, 1, 4], [1, 5, 4], [2, 6, 3], [3, 6, 7], [0, 4, 2], [2, 4, 6], [1, 3, 5], [3, 7, 5]]
    return V, np.asarray(F, dtype=np.int64)


# ------------------------------------------------------------------ the oracle (dtype float64) and its float32 restatement
def pair_closest(P, T, dtype=np.float64):
    """Closest point of triangles T [..., 9] to points P [..., 3] (broadcast): (distance, barycentrics [..., 3])."""
    P, T = np.asarray(P, dtype=dtype), np.asarray(T, dtype=dtype)
    a, b, c = T[..., 0:3], T[..., 3:6], T[..., 6:9]
    ab, ac, ap, bp, cp = b - a, c - a, P - a, P - b, P - c
    dot = lambda x, y: (x * y).sum(-1)                    # noqa: E731
    d1, d2, d3, d4, d5, d6 = dot(ab, ap), dot(ac, ap), dot(ab, bp), dot(ac, bp), dot(ab, cp), dot(ac, cp)
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    zero, one = np.zeros_like(d1), np.ones_like(d1)
    with np.errstate(divide="ignore", invalid="ignore"):
        vab, wac, wbc, den = d1 / (d1 - d3), d2 / (d2 - d6), (d4 - d3) / ((d4 - d3) + (d5 - d6)), va + vb + vc
        conds = [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (vc <= 0) & (d1 >= 0) & (d3 <= 0), (d6 >= 0) & (d5 <= d6),
                 (vb <= 0) & (d2 >= 0) & (d6 <= 0), (va <= 0) & ((d4 - d3) >= 0) & ((d5 - d6) >= 0)]
        v = np.select(conds, [zero, one, vab, zero, zero, one - wbc], vb / den)
        w = np.select(conds, [zero, zero, zero, one, wac, wbc], vc / den)
    q = a + ab * v[..., None] + ac * w[..., None] - P
    return np.sqrt(dot(q, q)), np.stack([1 - v - w, v, w], -1)


def brute_closest(P, T, dtype=np.float64, chunk=1024):
    """Per point: (distance to the mesh, first face at that distance)."""
    d, f = np.empty(len(P), dtype=dtype), np.empty(len(P), dtype=np.int64)
    for s in range(0, len(P), chunk):
        dd, _ = pair_closest(P[s:s + chunk, None, :], T[None], dtype)
        f[s:s + chunk] = dd.argmin(1)
        d[s:s + chunk] = dd.min(1)
    return d, f


def brute_winding(P, T, dtype=np.float64, chunk=1024):
    out = np.empty(len(P), dtype=dtype)
    T = np.asarray(T, dtype=dtype)
    for s in range(0, len(P), chunk):
        p = np.asarray(P[s:s + chunk], dtype=dtype)[:, None, :]
        a, b, c = T[None, :, 0:3] - p, T[None, :, 3:6] - p, T[None, :, 6:9] - p
        la, lb, lc = np.sqrt((a * a).sum(-1)), np.sqrt((b * b).sum(-1)), np.sqrt((c * c).sum(-1))
        num = (a * np.cross(b, c)).sum(-1)
        den = la * lb * lc + (a * b).sum(-1) * lc + (b * c).sum(-1) * la + (c * a).sum(-1) * lb
        out[s:s + chunk] = (2 * np.arctan2(num, den)).sum(1) / dtype(4 * np.pi)
    return out


# ------------------------------------------------------------------ the shared case: mesh, queries, oracle results (computed once)
class Case:
    def __init__(self):
        from sin3dm_amd.data.utils import normalize_aabb, sample_grid_points_aabb
        V0, self.F = torus()
        self.rot = rotation()
        V = V0 @ self.rot.T
        self.aabb, self.translation, self.scale = normalize_aabb(V, reso=24, mult=4)
        self.V = (V + self.translation) * self.scale
        self.grid = sample_grid_points_aabb(self.aabb, 24)
        assert self.grid.shape[:3] == (24, 16, 24)
        self.band = 2. / 24 * 3
        self.V32 = self.V.astype(np.float32)                       # what the device sees; the oracle reads the same values
        self.T = self.V32[self.F].reshape(-1, 9).astype(np.float64)
        rng = np.random.Generator(np.random.PCG64(11))
        tri = self.V32[self.F].astype(np.float64)
        exact = np.concatenate([self.V32.astype(np.float64), (tri[:, [0, 1, 2]] + tri[:, [1, 2, 0]]).reshape(-1, 3) / 2, tri.mean(1)])
        self.queries = np.concatenate([self.grid.reshape(-1, 3), rng.uniform(-1.3, 1.3, size=(1000, 3)), exact]).astype(np.float32)
        self.box_V, self.box_F = box_mesh(self.aabb)
        self.box_T = self.box_V.astype(np.float32)[self.box_F].reshape(-1, 9).astype(np.float64)
        self.wn_points = np.concatenate([self.grid.reshape(-1, 3), rng.uniform(-1, 1, size=(7, 3))]).astype(np.float32)
        self.open_keep = np.ones(len(self.F), dtype=bool)
        self.open_keep[100:140] = False
        self._memo = {}

    def memo(self, key, fn):
        if key not in self._memo:
            self._memo[key] = fn()
        return self._memo[key]

    def to_torus_frame(self, p):
        return (np.asarray(p, dtype=np.float64) / self.scale - self.translation) @ self.rot

    def sampler(self, **kw):
        from sin3dm_amd.data.mesh_sampler import MeshSampler
        return MeshSampler(verts=self.V32.astype(np.float64), faces=self.F, **kw)


_CASE = None


def case():
    global _CASE
    if _CASE is None:
        _CASE = Case()
    return _CASE


def check_closest(ms, T, queries, d_or, band):
    """The per-query assertions of the closest-point kernel (tests 1 and 2); returns (dist, face, bary) as NumPy arrays."""
    dist, face, bary = (t.cpu().numpy() for t in ms.closest(queries, band))
    band32 = np.float32(band)
    P = queries.astype(np.float64)
    err = np.abs(dist - np.minimum(d_or, float(band32)))
    print(f"band {band}: {len(P)} queries, {int((face >= 0).sum())} within the band, distance error max {err.max():.3e} (tol {TOL_DIST:.3e})")
    assert err.max() <= TOL_DIST
    hit = face >= 0
    far, near = d_or >= float(band32) + TOL_DIST, d_or < float(band32) - TOL_DIST     # rounding may decide either way in between
    assert (dist[far] == band32).all() and (face[far] == -1).all() and (bary[far] == 0).all()
    assert hit[near].all()
    assert (dist[~hit] == band32).all() and (face < len(T)).all()
    bc = bary[hit].astype(np.float64)
    assert (bary[hit] >= 0).all() and np.abs(bc.sum(1) - 1).max() <= 4 * 2.0 ** -23
    tri = T[face[hit]]
    recon = bc[:, 0:1] * tri[:, 0:3] + bc[:, 1:2] * tri[:, 3:6] + bc[:, 2:3] * tri[:, 6:9]
    gap = np.abs(np.linalg.norm(P[hit] - recon, axis=1) - dist[hit])
    d_face, _ = pair_closest(P[hit], tri)
    print(f"   |p - sum bc v| vs distance: {gap.max():.3e}; reported face above the minimum by {np.max(d_face - d_or[hit]):.3e}")
    assert gap.max() <= TOL_DIST
    assert np.max(d_face - d_or[hit]) <= TOL_DIST              # the reported face is one at the minimum distance (not: the same index)
    return dist, face, bary


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


if __name__ == "__main__":                                  # the fp32 restatement's gap to float64 (CPU): the source of the tolerances
    c = Case()
    Q = c.queries.astype(np.float64)
    worst_d = worst_w = 0.0
    for name, T in (("torus", c.T), ("box", c.box_T)):
        d64, _ = brute_closest(Q, T)
        d32, _ = brute_closest(Q, T, np.float32)
        worst_d = max(worst_d, float(np.abs(d64 - d32).max()))
        print(f"closest, {name}: fp32 vs float64 {np.abs(d64 - d32).max():.3e}")
    for name, F in (("closed", c.F), ("open", c.F[c.open_keep]), ("triangle", c.F[:1]), ("flipped", c.F[:, ::-1])):
        T = c.V32[F].reshape(-1, 9).astype(np.float64)
        w64, w32 = brute_winding(c.wn_points.astype(np.float64), T), brute_winding(c.wn_points.astype(np.float64), T, np.float32)
        worst_w = max(worst_w, float(np.abs(w64 - w32).max()))
        sure = np.abs(np.abs(w64) - 0.5) > 10 * TOL_WN
        print(f"winding, {name}: fp32 vs float64 {np.abs(w64 - w32).max():.3e}, undecided share {1 - sure.mean():.5f}")
    print(f"FP32_GAP_DIST {worst_d:.3e}  FP32_GAP_WN {worst_w:.3e}; nearest grid point to the surface {brute_closest(c.grid.reshape(-1, 3), c.T)[0].min():.3e}")
