"""Meshes, query sets and float64 oracles of the mesh-preprocessing tests (tests/test_meshprep_gpu.py, test_meshprep_hard_host.py,
test_meshprep_hard_gpu.py).  NumPy only: nothing here needs a GPU.  `python tests/meshprep_cases.py` prints the
fp32-restatement figures the tolerances come from, per set (CPU only).

Tolerances.  The brute force run in float32 differs from float64, over the meshes and query sets of test_meshprep_gpu.py, by at most
    FP32_GAP_DIST = 1.3e-7 in the distance (measured 1.288e-7)   and   FP32_GAP_WN = 8.4e-7 in the winding number (8.345e-7);
the device is allowed 8x that (FMA contraction, device sqrt, division and atan2): TOL_DIST = 1.04e-6, TOL_WN = 6.72e-6.

Two float64 definitions of the distance to a triangle live here.  `pair_closest` restates Ericson's region test, the formulation
the kernel started from; it divides 0 / 0 on a face without area.  `tri_distance64` is independent of it: the minimum of the three
clamped segment distances and, where the projection falls inside, the plane distance; it is defined on every face and is the
oracle of the hard sets.  `boundary_distance64` keeps the segments only.  The sandwich the soups are held to,

    min(min_f tri_distance64, band) - TOL_DIST  <=  dist  <=  min(min_f boundary_distance64, band) + TOL_DIST,

has two float64 oracle values as its bounds.  The lower one says that the reported distance belongs to a point of the mesh; the
upper one that no edge was missed.  They differ by at most a sliver's height and by nothing on a face without area, so the check
is exact where a float32 region test is worst (the plane of a sliver is not resolved by fp32 products: its normal is a difference
of products whose true value lies below their rounding), and asks fp32 for nothing it cannot give where the interior projection
is ill-conditioned.
"""
from fractions import Fraction

import numpy as np

FP32_GAP_DIST, FP32_GAP_WN = 1.3e-7, 8.4e-7
TOL_DIST, TOL_WN = 8 * FP32_GAP_DIST, 8 * FP32_GAP_WN
R_MAJOR, R_MINOR = 0.55, 0.22
CAP_EPS = (1e-2, 1e-3, 1e-4, 1e-5, 1e-6, 1e-7, 0.0)
SLIVER_EPS = (1e-3, 1e-6)
SOUP_BANDS = (0.25, 0.05)
SOUP_SIGMAS = (0.003, 0.03, 0.2)
TILE_FACES, TILE_POINTS = (1, 255, 256, 257, 513), (1, 511, 512, 513)        # kWindTile = 256 faces; a block owns 512 points


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


def box_mesh(aabb):
    lo, hi = aabb[:3], aabb[3:]
    V = np.array([[(lo, hi)[(i >> k) & 1][k] for k in range(3)] for i in range(8)], dtype=np.float64)
    F = [[0, 2, 1], [1, 2, 3], [4, 5, 6], [5, 7, 6], [0, 1, 4], [1, 5, 4], [2, 6, 3], [3, 6, 7], [0, 4, 2], [2, 4, 6], [1, 3, 5], [3, 7, 5]]
    return V, np.asarray(F, dtype=np.int64)


def uv_sphere(radius, centre, n_lat=24, n_lon=48):
    """2 * n_lon * (n_lat - 1) outward-oriented faces: 2208 for 24 x 48."""
    th = np.arange(1, n_lat) * np.pi / n_lat
    ph = np.arange(n_lon) * 2 * np.pi / n_lon
    ring = np.stack([np.sin(th)[:, None] * np.cos(ph)[None], np.cos(th)[:, None] * np.ones(n_lon)[None], np.sin(th)[:, None] * np.sin(ph)[None]], -1)
    V = np.concatenate([[[0.0, 1.0, 0.0]], ring.reshape(-1, 3), [[0.0, -1.0, 0.0]]]) * radius + np.asarray(centre, dtype=np.float64)
    idx = lambda r, k: 1 + r * n_lon + k % n_lon                        # noqa: E731
    F = [[0, idx(0, k + 1), idx(0, k)] for k in range(n_lon)]
    for r in range(n_lat - 2):
        for k in range(n_lon):
            F += [[idx(r, k), idx(r, k + 1), idx(r + 1, k + 1)], [idx(r, k), idx(r + 1, k + 1), idx(r + 1, k)]]
    south = len(V) - 1
    F += [[south, idx(n_lat - 2, k), idx(n_lat - 2, k + 1)] for k in range(n_lon)]
    return V, np.asarray(F, dtype=np.int64)


# ------------------------------------------------------------------ the oracle (dtype float64) and its float32 restatement
def _dot(x, y):
    return (x * y).sum(-1)


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


def ericson32_plain(P, T):
    """The formulation k_mesh_closest started from, in float32: Ericson's region test alone.  On a face without area it may
    return NaN (0 / 0), which the kernel's `d2 < best` never took: the face was dropped."""
    return pair_closest(P, T, np.float32)


def _bary_dist2(P, a, b, c, b0, b1, b2):
    q = b0[..., None] * a + b1[..., None] * b + b2[..., None] * c - P
    return _dot(q, q)


def closest32(P, T, dtype=np.float32):
    """closest_on_triangle of s3d_meshsdf.hip restated line by line (NumPy rounds every product; the device contracts some into
    FMAs): Ericson's answer with its barycentrics clamped into the triangle, then the three clamped edge projections; the
    candidate with the smallest reconstructed squared distance wins, the earlier one on a tie, a NaN never.  Returns
    (distance, barycentrics [..., 3]) in `dtype`."""
    P, T = np.asarray(P, dtype=dtype), np.asarray(T, dtype=dtype)
    a, b, c = np.broadcast_arrays(T[..., 0:3], T[..., 3:6], T[..., 6:9])
    ab, ac, bcv, ap, bp, cp = b - a, c - a, c - b, P - a, P - b, P - c
    d1, d2, d3, d4, d5, d6 = _dot(ab, ap), _dot(ac, ap), _dot(ab, bp), _dot(ac, bp), _dot(ab, cp), _dot(ac, cp)
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    zero, one = np.zeros_like(d1), np.ones_like(d1)
    with np.errstate(divide="ignore", invalid="ignore"):
        vab, wac, wbc, den = d1 / (d1 - d3), d2 / (d2 - d6), (d4 - d3) / ((d4 - d3) + (d5 - d6)), va + vb + vc
        v = np.fmin(np.fmax(vb / den, zero), one)                      # (fmin / fmax drop a NaN, as fminf / fmaxf do)
        u = one - v
        w = np.fmin(np.fmax(vc / den, zero), u)
        conds = [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (vc <= 0) & (d1 >= 0) & (d3 <= 0), (d6 >= 0) & (d5 <= d6),
                 (vb <= 0) & (d2 >= 0) & (d6 <= 0), (va <= 0) & ((d4 - d3) >= 0) & ((d5 - d6) >= 0)]
        cands = [(np.select(conds, [one, zero, one - vab, zero, one - wac, zero], u - w),
                  np.select(conds, [zero, one, vab, zero, zero, one - wbc], v),
                  np.select(conds, [zero, zero, zero, one, wac, wbc], w))]
        for num, e, which in ((d1, ab, 0), (d2, ac, 1), (_dot(bcv, bp), bcv, 2)):
            l2 = _dot(e, e)
            t = np.where(l2 > 0, np.fmin(np.fmax(num / l2, zero), one), zero)
            cands.append(((one - t, t, zero), (one - t, zero, t), (zero, one - t, t))[which])
        best = np.full(d1.shape, np.inf, dtype=dtype)
        bary = np.zeros(d1.shape + (3,), dtype=dtype)
        for bc in cands:
            dd = _bary_dist2(P, a, b, c, *bc)
            win = dd < best                                             # False on a NaN
            best = np.where(win, dd, best)
            bary = np.where(win[..., None], np.stack(np.broadcast_arrays(*bc), -1), bary)
    return np.sqrt(best), bary


def _segment_distance(P, u, v):
    e, w = v - u, P - u
    l2 = _dot(e, e)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(l2 > 0, np.clip(_dot(w, e) / np.where(l2 > 0, l2, 1.0), 0.0, 1.0), 0.0)
    q = w - t[..., None] * e
    return np.sqrt(_dot(q, q))


def boundary_distance64(P, T):
    """Distance of points P [..., 3] to the boundary (the three edge segments) of triangles T [..., 9], float64, broadcast."""
    P, T = np.asarray(P, dtype=np.float64), np.asarray(T, dtype=np.float64)
    a, b, c = T[..., 0:3], T[..., 3:6], T[..., 6:9]
    return np.minimum(np.minimum(_segment_distance(P, a, b), _segment_distance(P, b, c)), _segment_distance(P, c, a))


def exact_normals(T):
    """ab x ac of triangles T [..., 9] in rational arithmetic, each component rounded once to float64.  A float64 cross product
    is not enough on a sliver: the products of coordinate differences of float32 values may need more than 53 bits, and their
    rounding, 1e-16 of |ab| |ac|, is 1e-10 of a normal of length 1e-6 |ab| |ac| — 7e-12 in the plane distance of a point 0.07 away."""
    flat = np.ascontiguousarray(np.asarray(T, dtype=np.float64).reshape(-1, 9))
    key = hash(flat.tobytes())                                          # (a brute force asks for the same faces once per chunk of points)
    if key not in _NORMALS:
        out = np.empty((len(flat), 3), dtype=np.float64)
        for i, t in enumerate(flat):
            a, b, c = ([Fraction(float(x)) for x in t[k:k + 3]] for k in (0, 3, 6))
            u, v = [b[k] - a[k] for k in range(3)], [c[k] - a[k] for k in range(3)]
            out[i] = [float(u[1] * v[2] - u[2] * v[1]), float(u[2] * v[0] - u[0] * v[2]), float(u[0] * v[1] - u[1] * v[0])]
        if len(_NORMALS) >= 64:
            _NORMALS.clear()
        _NORMALS[key] = out
    return _NORMALS[key].reshape(np.shape(T)[:-1] + (3,))


_NORMALS = {}


def tri_distance64(P, T):
    """Distance of points to triangles, float64, independent of pair_closest: min(three clamped segment distances, the plane
    distance where |ab x ac|^2 > 0 and the projection lies inside by the three edge functions).  Defined on collinear and
    coincident-vertex faces."""
    P, T = np.asarray(P, dtype=np.float64), np.asarray(T, dtype=np.float64)
    a, b, c = T[..., 0:3], T[..., 3:6], T[..., 6:9]
    n = exact_normals(T)
    n2 = _dot(n, n)
    ap, bp, cp = P - a, P - b, P - c
    # the edge functions (e x (p - v)) . n, written (p - v) . (n x e): one product per face, not one per pair
    inside = (n2 > 0) & (_dot(ap, np.cross(n, b - a)) >= 0) & (_dot(bp, np.cross(n, c - b)) >= 0) & (_dot(cp, np.cross(n, a - c)) >= 0)
    plane = np.abs(_dot(ap, n)) / np.sqrt(np.where(n2 > 0, n2, 1.0))
    return np.minimum(boundary_distance64(P, T), np.where(inside, plane, np.inf))


def brute_min(fn, P, T, chunk=256):
    """Per point: (min over the faces of fn(P, T), which returns the distance or (distance, ...); the first face at it).  A NaN
    counts as +inf: the kernel's comparison never takes one."""
    d, f = np.empty(len(P), dtype=np.float64), np.empty(len(P), dtype=np.int64)
    for s in range(0, len(P), chunk):
        dd = fn(P[s:s + chunk, None, :], T[None])
        dd = np.asarray(dd[0] if isinstance(dd, tuple) else dd, dtype=np.float64)
        dd = np.where(np.isnan(dd), np.inf, dd)
        f[s:s + chunk] = dd.argmin(1)
        d[s:s + chunk] = dd.min(1)
    return d, f


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


# ------------------------------------------------------------------ the hard sets: slivers, soups, thin bands
class HardSet:
    """A mesh whose vertices are rounded to float32 before anything reads them (T: the float64 image of the rounded corners,
    [F, 9]), its float32 queries and winding-number points, and a memo of oracle results."""

    def __init__(self, name, V, F, queries=None, wn_points=None, **extra):
        self.name = name
        self.V32 = np.asarray(V, dtype=np.float64).astype(np.float32)
        self.F = np.asarray(F, dtype=np.int64)
        self.T = self.V32[self.F].reshape(-1, 9).astype(np.float64)
        self.queries = None if queries is None else np.asarray(queries).astype(np.float32)
        self.wn_points = None if wn_points is None else np.asarray(wn_points).astype(np.float32)
        assert self.queries is None or len(self.queries) * len(self.F) <= 2 * 10 ** 7
        assert self.wn_points is None or len(self.wn_points) * len(self.F) <= 2 * 10 ** 7
        self.__dict__.update(extra)
        self._memo = {}

    def memo(self, key, fn):
        if key not in self._memo:
            self._memo[key] = fn()
        return self._memo[key]

    def area2(self):
        """|ab x ac|^2 per face: 0 exactly where the face has no area."""
        n = exact_normals(self.T)
        return _dot(n, n)

    def sampler(self):
        from sin3dm_amd.data.mesh_sampler import MeshSampler
        return MeshSampler(verts=self.V32.astype(np.float64), faces=self.F)

    # the oracle values, each computed once
    def lo(self):
        return self.memo("lo", lambda: brute_min(tri_distance64, self.queries.astype(np.float64), self.T)[0])

    def hi(self):
        return self.memo("hi", lambda: brute_min(boundary_distance64, self.queries.astype(np.float64), self.T)[0])

    def wn(self):
        return self.memo("wn", lambda: brute_winding(self.wn_points.astype(np.float64), self.T))


def _unit(rng, n):
    v = rng.standard_normal((n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _soup_queries(rng, V32, n_faces, n=4000):
    """n points: the centroid of face i mod n_faces + N(0, sigma), sigma going through SOUP_SIGMAS in blocks of n_faces points."""
    i = np.arange(n)
    centroid = V32.astype(np.float64).reshape(n_faces, 3, 3).mean(1)
    sigma = np.asarray(SOUP_SIGMAS)[(i // n_faces) % len(SOUP_SIGMAS)]
    return centroid[i % n_faces] + rng.standard_normal((n, 3)) * sigma[:, None]


def _soup(name, corners, rng):
    V32 = np.asarray(corners, dtype=np.float64).reshape(-1, 3).astype(np.float32)
    n = len(V32) // 3
    return HardSet(name, V32, np.arange(3 * n).reshape(n, 3), queries=_soup_queries(rng, V32, n))


def cap_soup(eps, n=600):
    """n isolated cap triangles: a long edge of length L in [0.02, 0.3], the apex at height eps * L over its interior.  The first
    100 lie along a coordinate axis with the apex over the midpoint, so with eps = 0 they are exactly collinear after rounding; the
    others with eps = 0 are collinear to a rounding of the apex.  The same triangles for every eps but for the apex's height."""
    rng = np.random.Generator(np.random.PCG64(2024))
    L, ctr, u, t = rng.uniform(0.02, 0.3, n), rng.uniform(-0.7, 0.7, (n, 3)), _unit(rng, n), rng.uniform(0.2, 0.8, n)
    u[:100], t[:100] = np.eye(3)[np.arange(100) % 3], 0.5
    h = _unit(rng, n)
    h -= _dot(h, u)[:, None] * u
    h /= np.linalg.norm(h, axis=1, keepdims=True)
    a = (ctr - 0.5 * L[:, None] * u).astype(np.float32).astype(np.float64)
    b = (ctr + 0.5 * L[:, None] * u).astype(np.float32).astype(np.float64)
    c = a + t[:, None] * (b - a) + (eps * L)[:, None] * h
    return _soup(f"cap_soup[{eps:g}]", np.stack([a, b, c], 1), rng)


def needle_soup(n=600, n_points=20):
    """n triangles with two of their vertices 1e-3 L, 1e-6 L and 0 apart (a third of the faces each; which two vertices rotates)
    and n_points faces whose three vertices are equal."""
    rng = np.random.Generator(np.random.PCG64(2025))
    L, x, u, w = rng.uniform(0.02, 0.3, n), rng.uniform(-0.7, 0.7, (n, 3)), _unit(rng, n), _unit(rng, n)
    sep = np.asarray([1e-3, 1e-6, 0.0])[np.arange(n) % 3]
    tri = np.stack([x, x + (sep * L)[:, None] * u, x + L[:, None] * w], 1)
    perm = np.asarray([[0, 1, 2], [2, 0, 1], [0, 2, 1]])[(np.arange(n) // 3) % 3]                # the close pair: ab, bc, ac
    tri = np.take_along_axis(tri, perm[:, :, None], 1)
    pts = rng.uniform(-0.7, 0.7, (n_points, 1, 3)) * np.ones((1, 3, 1))
    return _soup("needle_soup", np.concatenate([tri, pts]), rng)


def sliver_torus(eps):
    """The Case torus with a vertex m = midpoint of ab + eps |ab| towards c, in the face's plane, on every face (a, b, c): the
    sliver (a, b, m) at index f, then (b, c, m) and (c, a, m): 3 * 576 = 1728 faces, closed, the orientation kept."""
    c = case()
    V, F = c.V32.astype(np.float64), c.F
    A, B, Cc = V[F[:, 0]], V[F[:, 1]], V[F[:, 2]]
    e = B - A
    le = np.linalg.norm(e, axis=1, keepdims=True)
    g = (Cc - A) - _dot(Cc - A, e)[:, None] * e / le ** 2
    g /= np.linalg.norm(g, axis=1, keepdims=True)
    m = len(V) + np.arange(len(F))
    faces = np.concatenate([np.stack([F[:, 0], F[:, 1], m], 1), np.stack([F[:, 1], F[:, 2], m], 1), np.stack([F[:, 2], F[:, 0], m], 1)])
    hs = HardSet(f"sliver_torus[{eps:g}]", np.concatenate([V, A + 0.5 * e + eps * le * g]), faces, queries=c.queries[::3], wn_points=c.wn_points[::3],
                 n_sliver=len(F))
    return hs


def duplicated():
    c = case()
    return HardSet("duplicated", c.V32, np.concatenate([c.F, c.F]), queries=c.queries[::3], wn_points=c.wn_points[::3], n_unique=len(c.F))


THIN_BAND = 0.004


def thin_band():
    """3000 area-weighted surface samples of the Case torus + N(0, 0.003); with band 0.004 the cell edge is extent / 256 > band."""
    c = case()
    rng = np.random.Generator(np.random.PCG64(35))
    tri = c.V32[c.F].astype(np.float64)
    area = 0.5 * np.linalg.norm(np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]), axis=1)
    f = rng.choice(len(c.F), size=3000, p=area / area.sum())
    on = np.einsum("nk,nkd->nd", rng.dirichlet(np.ones(3), size=3000), tri[f])
    return HardSet("thin_band", c.V32, c.F, queries=on + 0.003 * rng.standard_normal(on.shape), band=THIN_BAND)


def dense_cell():
    """A sphere of radius 0.02 with 2208 faces (edge ~ 0.0026) inside one cell of the band-0.25 grid, and one triangle that spans
    the box and is listed in every cell."""
    rng = np.random.Generator(np.random.PCG64(32))
    centre = np.array([0.31, -0.12, 0.27])
    V, F = uv_sphere(0.02, centre)
    assert len(F) == 2208
    big = np.array([[-1.0, -0.9, -1.0], [1.0, -0.8, 0.9], [-0.2, 1.0, 0.3]])
    queries = np.concatenate([rng.uniform(-1, 1, (1500, 3)), centre + 0.03 * rng.standard_normal((1500, 3))])
    return HardSet("dense_cell", np.concatenate([V, big]), np.concatenate([F, [[len(V), len(V) + 1, len(V) + 2]]]), queries=queries)


FLAT_BANDS = (0.25, 0.01)
FLAT_Y = float(np.float32(0.1))
FLAT_REACH = 2 * np.sqrt(2.0) + 0.2              # no corner of the quad lies further from the foot of a point of [-1, 1]^3


def flat():
    """One planar quad (two faces), y = fl32(0.1) on all four vertices: the mesh has no extent along y."""
    rng = np.random.Generator(np.random.PCG64(33))
    cs, sn = np.cos(0.4), np.sin(0.4)
    xz = np.array([[-0.8, -0.5], [0.8, -0.5], [0.8, 0.5], [-0.8, 0.5]]) @ np.array([[cs, -sn], [sn, cs]]).T + [0.1, -0.05]
    V = np.stack([xz[:, 0], np.full(4, FLAT_Y), xz[:, 1]], 1)
    P = rng.uniform(-1, 1, (2000, 3))
    return HardSet("flat", V, [[0, 1, 2], [0, 2, 3]], queries=P, wn_points=P)


def tile_edges(n_faces, n_points):
    c = case()
    return HardSet(f"tile_edges[{n_faces},{n_points}]", c.V32, c.F[:n_faces], wn_points=c.wn_points[:n_points])


_BUILDERS = {**{f"cap_soup[{e:g}]": (lambda e=e: cap_soup(e)) for e in CAP_EPS}, "needle_soup": needle_soup,
             **{f"sliver_torus[{e:g}]": (lambda e=e: sliver_torus(e)) for e in SLIVER_EPS}, "duplicated": duplicated, "thin_band": thin_band,
             "dense_cell": dense_cell, "flat": flat,
             **{f"tile_edges[{n},{m}]": (lambda n=n, m=m: tile_edges(n, m)) for n in TILE_FACES for m in TILE_POINTS}}
SOUPS = tuple(f"cap_soup[{e:g}]" for e in CAP_EPS) + ("needle_soup",)
SLIVER_TORI = tuple(f"sliver_torus[{e:g}]" for e in SLIVER_EPS)
TILE_EDGES = tuple(f"tile_edges[{n},{m}]" for n in TILE_FACES for m in TILE_POINTS)
TIGHT = SLIVER_TORI + ("duplicated", "thin_band", "dense_cell", "flat")        # held to TOL_DIST against the float64 distance itself
_HARD = {}


def hard(name):
    if name not in _HARD:
        _HARD[name] = _BUILDERS[name]()
    return _HARD[name]


def check_sandwich(ms, hs, band):
    """The per-query assertions of the closest-point kernel on a soup; returns max |dist - lo| (reported, not gated)."""
    dist, face, bary = (t.cpu().numpy() for t in ms.closest(hs.queries, band))
    band32 = np.float32(band)
    P = hs.queries.astype(np.float64)
    lo, hi = np.minimum(hs.lo(), float(band32)), np.minimum(hs.hi(), float(band32))
    assert np.isfinite(dist).all() and np.isfinite(bary).all()
    hit = face >= 0
    below, above, off = float(np.max(lo - dist)), float(np.max(dist - hi)), float(np.abs(dist - lo).max())
    print(f"{hs.name}, band {band}: {len(P)} queries, {int(hit.sum())} within the band; below lo by {below:.3e}, above hi by {above:.3e} "
          f"(tol {TOL_DIST:.3e}); |dist - lo| max {off:.3e}; hi - lo max {np.max(hi - lo):.3e}")
    assert below <= TOL_DIST and above <= TOL_DIST
    assert (face >= -1).all() and (face < len(hs.F)).all()
    assert np.array_equal(face == -1, dist == band32) and (bary[~hit] == 0).all()
    bc = bary[hit].astype(np.float64)
    assert (bary[hit] >= 0).all() and np.abs(bc.sum(1) - 1).max() <= 4 * 2.0 ** -23
    tri = hs.T[face[hit]]
    recon = bc[:, 0:1] * tri[:, 0:3] + bc[:, 1:2] * tri[:, 3:6] + bc[:, 2:3] * tri[:, 6:9]
    gap = np.abs(np.linalg.norm(P[hit] - recon, axis=1) - dist[hit])
    print(f"   |p - sum bc v| vs distance: {gap.max():.3e}")
    assert gap.max() <= TOL_DIST                                     # the reported point lies on the reported face
    return off


def undecided(wn64):
    """Share of points whose inside / outside mask rounding may decide."""
    return float((np.abs(np.abs(wn64) - 0.5) <= 10 * TOL_WN).mean())


def _restatement_figures():
    """Per set: what the float32 restatements give against the float64 oracles (CPU)."""
    rows = {}
    for name in SOUPS:
        hs = hard(name)
        P = hs.queries.astype(np.float64)
        lo, hi = hs.lo(), hs.hi()
        new, old = brute_min(closest32, P, hs.T)[0], brute_min(ericson32_plain, P, hs.T)[0]
        rows[name] = dict(new_below=float(np.max(lo - new)), new_above=float(np.max(new - hi)), new_off=float(np.abs(new - lo).max()),
                          old_above=float(np.max(old - hi)), old_count=int((old - hi > TOL_DIST).sum()), old_off=float(np.abs(old - lo).max()),
                          width=float(np.max(hi - lo)))
    for name in TIGHT:
        hs = hard(name)
        P = hs.queries.astype(np.float64)
        rows[name] = dict(new_off=float(np.abs(brute_min(closest32, P, hs.T)[0] - hs.lo()).max()),
                          old_off=float(np.abs(brute_min(ericson32_plain, P, hs.T)[0] - hs.lo()).max()))
        if hs.wn_points is not None:
            rows[name].update(wn_gap=float(np.abs(brute_winding(hs.wn_points.astype(np.float64), hs.T, np.float32) - hs.wn()).max()),
                              undecided=undecided(hs.wn()))
    return rows


if __name__ == "__main__":                                  # the fp32 restatement's gap to float64 (CPU): the source of the tolerances
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    c = Case()
    Q = c.queries.astype(np.float64)
    worst_d = worst_w = 0.0
    for name, T in (("torus", c.T), ("box", c.box_T)):
        d64, _ = brute_closest(Q, T)
        d32, _ = brute_closest(Q, T, np.float32)
        worst_d = max(worst_d, float(np.abs(d64 - d32).max()))
        print(f"closest, {name}: fp32 vs float64 {np.abs(d64 - d32).max():.3e}; closest32 vs float64 {np.abs(brute_min(closest32, Q, T)[0] - d64).max():.3e}")
    for name, F in (("closed", c.F), ("open", c.F[c.open_keep]), ("triangle", c.F[:1]), ("flipped", c.F[:, ::-1])):
        T = c.V32[F].reshape(-1, 9).astype(np.float64)
        w64, w32 = brute_winding(c.wn_points.astype(np.float64), T), brute_winding(c.wn_points.astype(np.float64), T, np.float32)
        worst_w = max(worst_w, float(np.abs(w64 - w32).max()))
        sure = np.abs(np.abs(w64) - 0.5) > 10 * TOL_WN
        print(f"winding, {name}: fp32 vs float64 {np.abs(w64 - w32).max():.3e}, undecided share {1 - sure.mean():.5f}")
    print(f"FP32_GAP_DIST {worst_d:.3e}  FP32_GAP_WN {worst_w:.3e}; nearest grid point to the surface {brute_closest(c.grid.reshape(-1, 3), c.T)[0].min():.3e}")
    print("\nthe hard sets, float32 restatements against the float64 oracles (lo = tri_distance64, hi = boundary_distance64, no band)")
    for name, r in _restatement_figures().items():
        if name in SOUPS:
            print(f"  {name:<20s} closest32: below lo {r['new_below']:10.3e}  above hi {r['new_above']:10.3e}  |d - lo| {r['new_off']:.3e}   "
                  f"ericson32_plain: above hi {r['old_above']:.3e} ({r['old_count']} queries over {TOL_DIST:.2e})  |d - lo| {r['old_off']:.3e}   "
                  f"hi - lo {r['width']:.3e}")
        else:
            wn = f"   winding fp32 vs float64 {r['wn_gap']:.3e}, undecided share {r['undecided']:.5f}" if "wn_gap" in r else ""
            print(f"  {name:<20s} closest32 vs float64 {r['new_off']:.3e}   ericson32_plain {r['old_off']:.3e}{wn}")
    worst = 0.0
    for name in TILE_EDGES:
        hs = hard(name)
        worst = max(worst, float(np.abs(brute_winding(hs.wn_points.astype(np.float64), hs.T, np.float32) - hs.wn()).max()))
        assert undecided(hs.wn()) <= 0.01, name
    print(f"  tile_edges ({len(TILE_EDGES)} pairs)  winding fp32 vs float64 {worst:.3e}")
