"""Inputs, NumPy restatements and checks of the textured-export tests on the hard cases (tests/test_texmesh_hard_host.py,
tests/test_texmesh_hard_gpu.py).  NumPy only: nothing here needs a GPU.

The restatements are written from the text of DESIGN.md §15, one per kernel of s3d_tex.hip and stage of simplify_mesh, and each
takes `fault=`: the clean statement with one defect put in.  Every check is a function of "got" arrays, so the GPU file feeds it
what the device returned and the host file feeds it the restatement (which must pass) and the restatement with one fault (which
the check must report).  Exact comparisons carry no tolerance.  The two bounds are derived, with u = 2^-24 (fp32 unit round-off):

  means       |got - mean| <= 0.5 ulp32(mean) + (n + 1) 2^-53 max|v|     one conversion to fp32; n - 1 double additions and one
                                                                         double division, each relative 2^-53 of at most max|v|
  positions   |got - pos|  <= 8 u M_f, M_f = max |coordinate| of the face   b1, b2 one rounding each, b0 two, three products, two
                                                                         sums: with b0 + b1 + b2 = 1 they add up to at most 5 u M_f,
                                                                         fewer when the compiler contracts a product into a sum

`mean` is the exact mean (math.fsum) of the fp32 inputs, `pos` the float64 barycentric formula."""
import math

import numpy as np

from test_texmesh_host import rasterise

U32 = 2.0 ** -24
POS_BOUND = 8 * U32                 # positions, relative to the face's largest |coordinate|
EDGE_BOUND = 8 * U32                # corner0: squared edge lengths in fp32 (three products, two sums) against float64
R_LIMIT = 1 << 20                   # simplify_mesh's largest grid


def rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def ulp32(x):
    """spacing of float32 at |x| (x float64): 2^(e - 24) for |x| = m 2^e, m in [0.5, 1); the subnormal spacing below 2^-126"""
    x = np.abs(np.asarray(x, np.float64))
    _, e = np.frexp(x)
    return np.ldexp(1.0, np.where(x == 0, -149, np.maximum(e - 24, -149)))


# ================================================================== k_cluster_keys
def np_grid(extent, R):
    """cell side s = fp32(extent_max / R) and cells per axis min(R, max(1, ceil(extent_axis / s))), in float32"""
    ext = np.asarray(extent, np.float32)
    s = np.float32(ext.max() / np.float32(R))
    dims = [int(min(R, max(1, math.ceil(float(np.float32(e / s)))))) for e in ext]
    return s, dims


def np_keys(v, origin, s, dims, fault=None):
    """float32: IEEE subtract, correctly rounded divide, floor, clamp to [0, R_axis - 1], key (ix Ry + iy) Rz + iz"""
    v, origin, s = np.asarray(v, np.float32), np.asarray(origin, np.float32), np.float32(s)
    dims = np.asarray(dims, np.int64)
    d = v - origin
    assert d.dtype == np.float32
    with np.errstate(all="ignore"):
        if fault == "reciprocal":
            q = d * (np.float32(1) / s)
        elif fault == "float64":
            q = d.astype(np.float64) / np.float64(s)
        else:
            q = d / s
    i = np.maximum(np.floor(q).astype(np.int64), 0)
    if fault != "no_clamp":
        i = np.minimum(i, dims - 1)
    if fault == "swapped_dims":
        return (i[:, 0] * dims[2] + i[:, 1]) * dims[1] + i[:, 2]
    return (i[:, 0] * dims[1] + i[:, 1]) * dims[2] + i[:, 2]


KEY_FAULTS = ("reciprocal", "float64", "no_clamp", "swapped_dims")
BOX = (8.0, 5.0, 3.0)


def _face_lattice(seed, n, box=BOX):
    """the 9 x 6 x 4 cell corners of the box and n points with coordinates in multiples of 1/8, one of them (at least) an integer"""
    g = rng(seed)
    corners = np.stack(np.meshgrid(*[np.arange(int(b) + 1) for b in box], indexing="ij"), -1).reshape(-1, 3).astype(np.float64)
    p = np.stack([g.integers(0, int(b) * 8 + 1, n) for b in box], 1) / 8.0
    ax = g.integers(0, 3, n)
    p[np.arange(n), ax] = np.round(p[np.arange(n), ax])
    return np.concatenate([corners, p]).astype(np.float32)


def _with_neighbours(v):
    """v, v one ulp down, v one ulp up (every coordinate)"""
    v = np.asarray(v, np.float32)
    return np.concatenate([v, np.nextafter(v, np.float32(-np.inf)), np.nextafter(v, np.float32(np.inf))])


class KeyCase:
    """verts float32 [n,3] with the grid they are binned on: origin and extent come from `base` (the unmoved vertices)"""

    def __init__(self, name, base, verts, R, unmoved):
        self.name, self.R, self.unmoved = name, R, unmoved          # the first `unmoved` vertices are lattice points as they are
        base = np.asarray(base, np.float32)
        self.verts = np.ascontiguousarray(verts, np.float32)
        self.origin = base.min(0)
        self.extent = base.max(0) - self.origin
        self.s, self.dims = np_grid(self.extent, R)

    def keys(self, fault=None):
        return np_keys(self.verts, self.origin, self.s, self.dims, fault)


def _boundary_verts(seed, base, R):
    """vertices with one coordinate at fp32(k s) (k = 0 .. R_axis) from the origin, the others from the lattice"""
    g = rng(seed)
    origin = base.min(0)
    s, dims = np_grid(base.max(0) - origin, R)
    out = []
    for ax in range(3):
        k = np.arange(dims[ax] + 1, dtype=np.float32)
        for rep in range(3):
            p = base[g.integers(0, len(base), len(k))].copy()
            p[:, ax] = origin[ax] + k * s
            out.append(p)
    return np.concatenate(out).astype(np.float32)


KEY_CASES = ("lattice_R8", "box_R7", "box_R13", "sheet_R8", "offset_R8", "offset_R13")
_key_cases = {}


def key_case(name):
    if name not in _key_cases:
        lat = _face_lattice(1, 1000)
        if name == "lattice_R8":                                         # s = 1: every vertex on a cell face, the maxima on the clamp
            c = KeyCase(name, lat, _with_neighbours(lat), 8, len(lat))
        elif name in ("box_R7", "box_R13"):                              # s inexact: the boundaries k s are not representable
            R = int(name[5:])
            c = KeyCase(name, lat, np.concatenate([lat[:400], _with_neighbours(_boundary_verts(2, lat, R))]), R, 400)
        elif name == "sheet_R8":                                         # no extent along z: dims[2] = 1
            flat = lat.copy()
            flat[:, 2] = 0.375
            c = KeyCase(name, flat, _with_neighbours(flat), 8, len(flat))
        elif name in ("offset_R8", "offset_R13"):
            R = int(name[8:])
            off = (lat.astype(np.float64) + np.asarray([1000.0, -2000.0, 0.5])).astype(np.float32)
            c = KeyCase(name, off, np.concatenate([_with_neighbours(off[:700]), _with_neighbours(_boundary_verts(3, off, R))]), R, 700)
        else:
            raise KeyError(name)
        assert len(c.verts) <= 4096
        _key_cases[name] = c
    return _key_cases[name]


def check_keys(case, got):
    got = np.asarray(got)
    assert got.shape == (len(case.verts),) and got.dtype == np.int64
    want = case.keys()
    bad = np.flatnonzero(got != want)
    assert len(bad) == 0, (case.name, len(bad), case.verts[bad[:4]].tolist(), got[bad[:4]].tolist(), want[bad[:4]].tolist())


# ================================================================== k_cluster_means
def np_means(vals, order, seg, fault=None):
    """float32 [nc, C]: per (cluster, channel) the members order[seg[c] : seg[c + 1]] added in that order in double, divided by
    their number, converted once; an empty segment gives 0"""
    vals, order, seg = np.asarray(vals, np.float32), np.asarray(order, np.int64), np.asarray(seg, np.int64)
    out = np.zeros((len(seg) - 1, vals.shape[1]), np.float32)
    for c in range(len(seg) - 1):
        b, e = seg[c], seg[c + 1]
        if e <= b:
            continue
        m = vals[np.arange(b, e) if fault == "unsorted" else order[b:e]]
        if fault == "float32_accumulator":
            out[c] = np.add.accumulate(m, axis=0, dtype=np.float32)[-1] / np.float32(e - b)
        else:
            out[c] = (np.add.accumulate(m.astype(np.float64), axis=0)[-1] / float(e - b)).astype(np.float32)
    if fault == "one_ulp":
        out = np.nextafter(out, np.float32(np.inf))
    return out


MEAN_FAULTS = {"float32_accumulator": "one_cluster", "unsorted": "small_clusters", "one_ulp": "one_cluster"}      # fault -> the set that shows it
MEAN_CASES = [("one_cluster", 1), ("one_cluster", 5), ("small_clusters", 1), ("small_clusters", 5)]
_mean_cases = {}


class MeanCase:
    def __init__(self, name, vals, order, seg):
        self.name, self.vals, self.order, self.seg = name, np.ascontiguousarray(vals, np.float32), order.astype(np.int64), seg.astype(np.int64)
        self._exact = None

    def exact(self):
        """the exact mean of the fp32 members, rounded once to float64; NaN for an empty segment"""
        if self._exact is None:
            v64 = self.vals.astype(np.float64)
            out = np.full((len(self.seg) - 1, v64.shape[1]), np.nan)
            for c in range(len(self.seg) - 1):
                m = self.order[self.seg[c]:self.seg[c + 1]]
                for ch in range(v64.shape[1] if len(m) else 0):
                    out[c, ch] = math.fsum(v64[m, ch]) / len(m)          # fsum is exact: one rounding in the division
            self._exact = out
        return self._exact


def mean_case(name, C):
    """positions 1000 + 1e-3 noise in the first three columns, then C attribute channels of noise scaled 1, 1e3, 1e-3, 1, 1e3.
    one_cluster: 50 000 members in a shuffled order.  small_clusters: 3000 segments of 0 to 3 members (every tenth one empty)."""
    if (name, C) not in _mean_cases:
        g = rng(10 + C)
        n = 50000 if name == "one_cluster" else 6000
        scale = np.asarray([1.0, 1e3, 1e-3, 1.0, 1e3])[:C]
        vals = np.concatenate([1000.0 + 1e-3 * g.standard_normal((n, 3)), g.standard_normal((n, C)) * scale], 1)
        if name == "one_cluster":
            order, seg = g.permutation(n), np.asarray([0, n])
        else:
            size = g.integers(1, 4, 3000)
            size[::10] = 0
            seg = np.concatenate([[0], np.cumsum(size)])
            order = g.permutation(n)[:seg[-1]]
        _mean_cases[(name, C)] = MeanCase(f"{name}[C={C}]", vals, order, seg)
    return _mean_cases[(name, C)]


def check_means(case, got):
    """-> worst ratio of |got - mean| to 0.5 ulp32(mean) + (n + 1) 2^-53 max|v|; an empty segment is 0.0"""
    got = np.asarray(got)
    want = case.exact()
    assert got.shape == want.shape and got.dtype == np.float32
    n = np.diff(case.seg)
    empty = n == 0
    assert (got[empty] == 0).all(), (case.name, "empty segment")
    vmax = np.zeros_like(want)
    a = np.abs(case.vals.astype(np.float64))
    for c in np.flatnonzero(~empty):
        vmax[c] = a[case.order[case.seg[c]:case.seg[c + 1]]].max(0)
    bound = 0.5 * ulp32(want[~empty]) + (n[~empty, None] + 1) * 2.0 ** -53 * vmax[~empty]
    ratio = np.abs(got[~empty].astype(np.float64) - want[~empty]) / bound
    assert ratio.max() <= 1.0, (case.name, float(ratio.max()))
    return float(ratio.max())


# ================================================================== k_remap_faces, the keep-first dedupe, the whole of simplify_mesh
def np_faces(tris, vmap, fault=None):
    """remap, drop faces with two equal indices, keep the lowest-index face of every vertex set in its own winding, preserve the order"""
    m = np.asarray(vmap)[np.asarray(tris)].astype(np.int64)
    ok = (m[:, 0] != m[:, 1]) & (m[:, 1] != m[:, 2]) & (m[:, 0] != m[:, 2])
    if not ok.any():
        return m[:0]
    live = np.flatnonzero(ok)
    sets = np.sort(m[ok], 1)
    if fault == "keep_last":
        _, first = np.unique(sets[::-1], axis=0, return_index=True)
        first = len(sets) - 1 - first
    else:
        _, first = np.unique(sets, axis=0, return_index=True)
    out = m[live[np.sort(first)]]
    return np.sort(out, 1) if fault == "sorted_triple" else out


FACE_FAULTS = ("keep_last", "sorted_triple")


def np_simplify(v, t, R, fault=None):
    """simplify_mesh at a given R -> dict: origin, s, dims, keys, vmap (clusters in ascending key), tris (compacted), used (the
    cluster of every output vertex)"""
    v = np.asarray(v, np.float32)
    origin = v.min(0)
    s, dims = np_grid(v.max(0) - origin, R)
    keys = np_keys(v, origin, s, dims)
    vmap = np.unique(keys, return_inverse=True)[1].reshape(-1)
    f = np_faces(t, vmap, fault)
    used = np.unique(f)
    return {"origin": origin, "s": s, "dims": dims, "keys": keys, "vmap": vmap, "tris": np.searchsorted(used, f), "used": used}


def np_count(v, t, R):
    return len(np_simplify(v, t, R)["tris"])


def np_bisect(v, t, n_faces):
    """R of simplify_mesh: count(1) = 0; hi doubles while count(hi) <= n_faces, at most up to 2^21; then the bisection, unless
    hi has left the range, in which case lo = 2^20 stands"""
    lo, hi = 1, 2
    while hi <= R_LIMIT and np_count(v, t, hi) <= n_faces:
        lo, hi = hi, hi * 2
    while hi <= R_LIMIT and hi - lo > 1:
        mid = (lo + hi) // 2
        if np_count(v, t, mid) <= n_faces:
            lo = mid
        else:
            hi = mid
    return lo


def sheet(nx=12, ny=12):
    """(nx + 1)(ny + 1) vertices of a rippled sheet, spacing 1 by 0.75, and its 2 nx ny faces"""
    i, j = np.meshgrid(np.arange(nx + 1), np.arange(ny + 1), indexing="ij")
    v = np.stack([i * 1.0, j * 0.75, 0.3 * np.sin(0.9 * i + 0.4) * np.cos(0.7 * j)], -1).reshape(-1, 3).astype(np.float32)
    f = []
    for a in range(nx):
        for b in range(ny):
            p, q, r, s = a * (ny + 1) + b, (a + 1) * (ny + 1) + b, (a + 1) * (ny + 1) + b + 1, a * (ny + 1) + b + 1
            f += [[p, q, r], [r, s, p]]                                  # the second one is not in ascending order: its winding shows
    return v, np.asarray(f, np.int32)


class FaceCase:
    def __init__(self, name, v, t, n_faces, n_first, long_bisection=False):
        self.name, self.verts, self.tris, self.n_faces = name, v, np.ascontiguousarray(t, np.int32), n_faces
        self.n_first = n_first                       # None, or: face i repeats face i % n_first (i < n_first is the one to keep)
        self.attrs = (rng(7).standard_normal((len(v), 2)) * [1.0, 1e3]).astype(np.float32)      # averaged like the positions
        self.long_bisection = long_bisection


FACE_CASES = ("double_sided", "repeats", "repeats_long", "double_sided_long")
_face_cases = {}


def face_case(name):
    if name not in _face_cases:
        v, f = sheet()
        F = len(f)
        if name.startswith("double_sided"):                              # the copy of face i at i + F, reversed
            t = np.concatenate([f, f[:, ::-1]])
            c = FaceCase(name, v, t, 300 if name.endswith("long") else 100, F, name.endswith("long"))
        else:                                                            # (a,b,c) first, then (b,c,a) and (c,b,a) behind all of them
            t = np.concatenate([f, f[:, [1, 2, 0]], f[:, ::-1]])
            c = FaceCase(name, v, t, 288 if name.endswith("long") else 60, F, name.endswith("long"))
        _face_cases[name] = c
    return _face_cases[name]


def np_simplified(case, R, fault=None):
    """what simplify_mesh returns for the case at grid R, as check_simplified takes it"""
    st = np_simplify(case.verts, case.tris, R, fault)
    order = np.argsort(st["vmap"], kind="stable")
    seg = np.concatenate([[0], np.cumsum(np.bincount(st["vmap"]))])
    return (np_means(case.verts, order, seg)[st["used"]], st["tris"].astype(np.int32), st["vmap"], st["keys"], st["dims"], st["s"],
            np_means(case.attrs, order, seg)[st["used"]])


def check_simplified(case, R, got_verts, got_tris, got_vmap, got_keys, got_dims, got_s, got_attrs):
    """the output of simplify_mesh(case, attrs=case.attrs) at the device's R against the restatement at that R: keys, vmap and faces
    exactly, every kept face the first copy in its own winding, the means of vertices and attributes inside the derived bound ->
    worst ratio to it"""
    v, t = case.verts, case.tris
    st = np_simplify(v, t, R)
    assert list(got_dims) == st["dims"] and np.float32(got_s) == st["s"]
    assert np.array_equal(np.asarray(got_keys), st["keys"])
    assert np.array_equal(np.asarray(got_vmap).astype(np.int64), st["vmap"])
    got_tris = np.asarray(got_tris)
    assert got_tris.dtype == np.int32 and got_tris.shape == st["tris"].shape and np.array_equal(got_tris, st["tris"]), case.name
    assert len(got_tris) <= case.n_faces
    # said once more without the restatement's dedupe: every kept face is the row of the lowest-index input face with its vertex set
    m = st["vmap"][t].astype(np.int64)
    sets = [tuple(sorted(r)) for r in m.tolist()]
    lowest = {}
    for i, k in enumerate(sets):
        lowest.setdefault(k, i)
    kept = st["used"][got_tris]
    for row in kept.tolist():
        i = lowest[tuple(sorted(row))]
        assert m[i].tolist() == row, (case.name, i, m[i].tolist(), row)
        assert case.n_first is None or i < case.n_first
    # vertices: the means of the members in ascending vertex index
    order = np.argsort(st["vmap"], kind="stable")
    seg = np.concatenate([[0], np.cumsum(np.bincount(st["vmap"]))])
    vals = np.concatenate([v, case.attrs], 1)
    mc = MeanCase(case.name, vals, order, seg)
    got = np.concatenate([np.asarray(got_verts), np.asarray(got_attrs)], 1)
    assert got.shape == (len(st["used"]), vals.shape[1])
    full = np.array(np_means(vals, order, seg))
    full[st["used"]] = got                                                # dropped clusters: nothing to compare
    return check_means(mc, full)


def check_invariant(case, R):
    """count(R) <= n_faces < count(R + 1), recomputed in NumPy; where faces repeat so often that no grid up to 2^20 is over the
    budget, the documented outcome instead: R = 2^20, the finest grid, still inside the budget"""
    v, t = case.verts, case.tris
    assert np_count(v, t, R) <= case.n_faces
    if case.long_bisection:
        assert R == R_LIMIT
    else:
        assert 1 <= R < R_LIMIT and np_count(v, t, R + 1) > case.n_faces


# ================================================================== k_face_corner0
def np_edge2(v, t, dtype=np.float32):
    """squared lengths of v0v1, v1v2, v2v0 [F,3]"""
    p = np.asarray(v, dtype)[np.asarray(t)]
    d = np.stack([p[:, (j + 1) % 3] - p[:, j] for j in range(3)], 1)
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def np_corner0(v, t, fault=None, dtype=np.float32):
    """the vertex opposite the longest edge; of equal edges the first of v0v1, v1v2, v2v0"""
    d = np_edge2(v, t, dtype)
    e = 2 - np.argmax(d[:, ::-1], 1) if fault == "last_max" else np.argmax(d, 1)
    return ((e + (1 if fault == "plus_one" else 2)) % 3).astype(np.int32)


CORNER_FAULTS = ("last_max", "plus_one")


def tie_faces():
    """faces with small-integer coordinates (every squared length exact in fp32, contracted or not) -> verts, tris, name per face"""
    A, B, Cc = (0, 5, 0), (-1, 0, 0), (1, 0, 0)                        # AB = AC = sqrt(26) > BC = 2: the two longest tie
    P, Q, Rr = (0, 1, 0), (-3, 0, 0), (3, 0, 0)                        # PQ = PR = sqrt(10) < QR = 6: the two shortest tie
    shapes = {"equilateral": [(3, 0, 0), (0, 3, 0), (0, 0, 3)], "equilateral_far": [(7, 1, -2), (1, 7, -2), (1, 1, 4)],
              "long_pair_01": [B, A, Cc], "long_pair_12": [B, Cc, A], "long_pair_20": [A, B, Cc],
              "long_pair_01_reversed": [Cc, A, B], "long_pair_12_reversed": [Cc, B, A], "long_pair_20_reversed": [A, Cc, B],
              "short_pair_01": [Q, P, Rr], "short_pair_12": [Q, Rr, P], "short_pair_20": [P, Q, Rr],
              "point": [(2, 3, 4)] * 3, "v0_is_v1": [(1, 2, 3), (1, 2, 3), (4, 6, 3)], "v1_is_v2": [(4, 6, 3), (1, 2, 3), (1, 2, 3)],
              "v2_is_v0": [(1, 2, 3), (4, 6, 3), (1, 2, 3)]}
    verts, tris, names = [], [], []
    for shift, perm in (((0, 0, 0), (0, 1, 2)), ((1000, -2000, 16), (2, 0, 1)), ((-7, 300, 40000), (1, 2, 0))):
        for name, tri in shapes.items():
            tris.append([len(verts) + j for j in range(3)])
            verts += [[p[perm[k]] + shift[k] for k in range(3)] for p in tri]
            names.append(f"{name}{list(shift)}")
    return np.asarray(verts, np.float32), np.asarray(tris, np.int32), names


TIE_WANT = {"equilateral": 2, "equilateral_far": 2, "long_pair_01": 2, "long_pair_12": 0, "long_pair_20": 2, "long_pair_01_reversed": 2,
            "long_pair_12_reversed": 0, "long_pair_20_reversed": 2, "short_pair_01": 1, "short_pair_12": 2, "short_pair_20": 0,
            "point": 2, "v0_is_v1": 0, "v1_is_v2": 2, "v2_is_v0": 2}       # by hand, from the first-maximum rule


def check_corner0_ties(got):
    v, t, names = tie_faces()
    got = np.asarray(got)
    want = np_corner0(v, t)
    assert got.dtype == np.int32 and got.shape == want.shape
    bad = np.flatnonzero(got != want)
    assert len(bad) == 0, [(names[i], int(got[i]), int(want[i])) for i in bad]


CORNER_SEED = 5


def generic_faces(seed=CORNER_SEED, F=2000):
    """2000 faces of three different vertices each: 1500 over 3000 shared vertices of order 1, 500 over 750 vertices at offset 1000"""
    g = rng(seed)
    v = g.uniform(-1, 1, (3750, 3))
    v[3000:] = v[3000:] * 0.5 + np.asarray([1000.0, -1000.0, 1000.0])

    def faces(n, count):
        a, d1, d2 = g.integers(0, n, count), g.integers(1, n // 3, count), g.integers(1, n // 3, count)
        return np.stack([a, (a + d1) % n, (a + d1 + d2) % n], 1)
    t = np.concatenate([faces(3000, F - 500), 3000 + faces(750, 500)])
    return v.astype(np.float32), t.astype(np.int32)


def corner0_band(v, t):
    """float64: (restated corner0, the faces whose longest edge leads the next one by no more than EDGE_BOUND relative)"""
    d = np_edge2(v, t, np.float64)
    top = np.sort(d, 1)
    return np_corner0(v, t, dtype=np.float64), top[:, 2] - top[:, 1] <= EDGE_BOUND * top[:, 2]


def check_corner0_generic(v, t, got):
    """-> share of faces inside the band.  The chosen edge is within EDGE_BOUND of the float64 maximum; outside the band the
    choice is the float64 one"""
    got = np.asarray(got).astype(np.int64)
    assert got.shape == (len(t),) and got.min() >= 0 and got.max() <= 2
    d = np_edge2(v, t, np.float64)
    chosen = d[np.arange(len(t)), (got + 1) % 3]                          # corner r is opposite the edge from r + 1 to r + 2
    assert (chosen >= (1 - EDGE_BOUND) * d.max(1)).all()
    want, band = corner0_band(v, t)
    assert band.mean() <= 0.01
    assert np.array_equal(got[~band], want[~band])
    return float(band.mean())


# ================================================================== k_texel_positions
ATLAS_LAYOUTS = [(1, 8), (2, 8), (3, 19), (5, 37), (7, 128), (33, 100), (999, 512)]
TEXEL_FAULTS = ("k_past_F", "open_hypotenuse", "uv_swapped_upper", "r_minus_j", "plus_half")


def chart_frames(F, n, c):
    """origin [F,2] and corners [F,3,2] of every face's chart in texels, restated from the layout"""
    k = np.arange(F)
    cell = k // 2
    org = np.stack([(cell % n) * c, (cell // n) * c], 1)
    lower = np.asarray([[1, 1], [c - 4, 1], [1, c - 4]])
    upper = np.asarray([[c - 1, c - 1], [4, c - 1], [c - 1, 4]])
    return org, org[:, None, :] + np.where((k % 2 == 0)[:, None, None], lower[None], upper[None])


def atlas_nc(F, T):
    half = (F + 1) // 2
    n = max(1, math.isqrt(half))
    n += n * n < half
    return n, T // n


def np_texels(v, t, corner0, T, fault=None, dtype=np.float64):
    """face id int [T*T] (-1: uncovered) and position [T*T,3] of every texel, texel (x, y) at y T + x.  Face k in cell k // 2, the
    lower chart x, y >= 1, x + y <= c - 4 from the cell origin, the upper chart its mirror image; b1 = (u - .5) / L,
    b2 = (v - .5) / L, b0 = 1 - b1 - b2 with (u, v) = (x, y) in the lower and (c - 1 - x, c - 1 - y) in the upper chart;
    pos = b0 V0 + b1 V1 + b2 V2, V_j = vertex (corner0 + j) mod 3 of the face.  dtype float32 restates the kernel's arithmetic."""
    v, t = np.asarray(v, dtype), np.asarray(t)
    F = len(t)
    n, c = atlas_nc(F, T)
    L = c - 5
    y, x = np.meshgrid(np.arange(T), np.arange(T), indexing="ij")
    col, row = x // c, y // c
    lx, ly = x - col * c, y - row * c
    cell = row * n + col
    hyp_lo, hyp_up = (lx + ly < c - 4, lx + ly > c + 2) if fault == "open_hypotenuse" else (lx + ly <= c - 4, lx + ly >= c + 2)
    lower = (lx >= 1) & (ly >= 1) & hyp_lo
    upper = (lx <= c - 2) & (ly <= c - 2) & hyp_up & ~lower
    k = np.where(lower, 2 * cell, np.where(upper, 2 * cell + 1, -1))
    k[(col >= n) | (row >= n)] = -1
    past = k >= F
    if fault != "k_past_F":
        k[past] = -1
    uu, vv = np.where(lower, lx, c - 1 - lx), np.where(lower, ly, c - 1 - ly)
    if fault == "uv_swapped_upper":
        uu, vv = np.where(upper, vv, uu), np.where(upper, uu, vv)
    half = 0.5 if fault == "plus_half" else -0.5
    b1 = ((uu.astype(dtype) + dtype(half)) / dtype(L)).reshape(-1)
    b2 = ((vv.astype(dtype) + dtype(half)) / dtype(L)).reshape(-1)
    b0 = dtype(1) - b1 - b2
    k = k.reshape(-1)
    ok = (k >= 0) & (k < F)
    kk = np.where(ok, k, 0)
    r = np.asarray(corner0).astype(np.int64)[kk]
    sign = -1 if fault == "r_minus_j" else 1
    V = [v[t[kk, (r + sign * j) % 3]] for j in range(3)]
    pos = (b0[:, None] * V[0] + b1[:, None] * V[1]) + b2[:, None] * V[2]
    pos[~ok] = 0
    assert pos.dtype == dtype
    return k, pos


def texel_mesh(F, far, seed=21):
    """F faces over shared random vertices of order 1, or the same mesh scaled by 1e-2 at offset 1000"""
    g = rng(seed + F)
    nv = max(3, (F + 1) // 2 + 2)
    v = g.uniform(-1, 1, (nv, 3))
    t = np.stack([g.permutation(nv)[:3] for _ in range(F)]).astype(np.int32)
    if far:
        v = v * 1e-2 + np.asarray([1000.0, -1000.0, 1000.0])
    return v.astype(np.float32), t


def check_texels(v, t, corner0, T, got_fid, got_pos):
    """face ids against rasterise(F, T) exactly, uncovered positions 0, covered ones within POS_BOUND M_f of the float64 formula
    and inside the face's bounding box widened by that -> worst ratio to the bound"""
    F = len(t)
    got_fid, got_pos = np.asarray(got_fid), np.asarray(got_pos)
    assert got_fid.shape == (T * T,) and got_pos.shape == (T * T, 3) and got_pos.dtype == np.float32
    face, claims, n, c = rasterise(F, T)
    assert (n, c) == atlas_nc(F, T) and claims.max() <= 1
    bad = np.flatnonzero(got_fid != face.reshape(-1))
    assert len(bad) == 0, (F, T, len(bad), bad[:8].tolist(), got_fid[bad[:8]].tolist())
    cov = got_fid >= 0
    assert (got_pos[~cov] == 0).all()
    _, want = np_texels(v, t, corner0, T)
    p = np.asarray(v, np.float64)[np.asarray(t)]                          # [F,3,3]
    k = got_fid[cov]
    M = np.abs(p).max((1, 2))[k]
    bound = POS_BOUND * M[:, None]
    got = got_pos[cov].astype(np.float64)
    ratio = np.abs(got - want[cov]) / bound
    assert ratio.max() <= 1.0, (F, T, float(ratio.max()))
    assert (got >= p.min(1)[k] - bound).all() and (got <= p.max(1)[k] + bound).all()
    return float(ratio.max())


def np_uvs(corner0, F, T):
    """[3F,2] float32: vertex j of face k shows chart corner (j - corner0[k]) mod 3, in units of the texture"""
    n, c = atlas_nc(F, T)
    _, corners = chart_frames(F, n, c)
    which = (np.arange(3)[None, :] - np.asarray(corner0).astype(np.int64)[:, None]) % 3
    return (np.take_along_axis(corners, which[:, :, None], 1).reshape(-1, 2) / float(T)).astype(np.float32)


# ================================================================== k_tex_quantize
def np_quantize(cols, idx, T, fault=None):
    """uint8 [T*T, C]: zeros, then img[idx[i]] = uint8(clamp(fp32(col[i]) * fp32(255), 0, 255)), truncating; the clamp is
    fmax / fmin, so a NaN becomes 0; an index outside [0, T*T) is ignored"""
    cols, idx = np.asarray(cols, np.float32), np.asarray(idx, np.int64)
    with np.errstate(all="ignore"):
        x = cols * np.float32(255)
        assert x.dtype == np.float32
        if fault == "clamp_after_cast":                                   # int32 conversion (saturating, NaN -> 0), then the low byte
            i = np.trunc(np.clip(np.nan_to_num(x.astype(np.float64), nan=0.0), -2.0 ** 31, 2.0 ** 31 - 1)).astype(np.int64)
            q = (i & 255).astype(np.uint8)
        else:
            x = np.fmin(np.fmax(x, np.float32(0)), np.float32(255))
            q = (np.rint(x) if fault == "round" else np.trunc(x)).astype(np.int64).astype(np.uint8)
    img = np.zeros((T * T, cols.shape[1]), np.uint8)
    ok = (idx >= 0) & (idx < T * T)
    img[idx[ok]] = q[ok]
    return img


QUANT_FAULTS = ("round", "clamp_after_cast")
QUANT_T = 32


def quant_table():
    """fp32(k / 255) and its two neighbours for k = 0 .. 255, and the values outside [0, 1]; then NaN"""
    k = (np.arange(256) / 255.0).astype(np.float32)
    special = np.asarray([-0.0, -1e-3, 1.0, np.nextafter(np.float32(1), np.float32(2)), 2.0, np.inf, -np.inf, np.nan], np.float32)
    return np.concatenate([k, np.nextafter(k, np.float32(-np.inf)), np.nextafter(k, np.float32(np.inf)), special])


def quant_case(C, seed=31):
    """cols [N, C]: every channel holds the whole table (in an order of its own); idx: N distinct texels in a shuffled order with
    four indices outside [0, T^2) among them (their colours would be 255)"""
    g = rng(seed + C)
    tab = quant_table()
    N = len(tab) + 4
    assert N < QUANT_T * QUANT_T
    cols = np.stack([np.concatenate([tab[g.permutation(len(tab))], np.ones(4, np.float32)]) for _ in range(C)], 1)
    idx = g.permutation(QUANT_T * QUANT_T)[:N].astype(np.int64)
    idx[-4:] = [-1, QUANT_T * QUANT_T, 1 << 40, -(1 << 40)]
    return np.ascontiguousarray(cols, np.float32), idx


def check_quantize(cols, idx, T, got):
    got = np.asarray(got)
    want = np_quantize(cols, idx, T)
    assert got.dtype == np.uint8 and got.shape == want.shape
    bad = np.argwhere(got != want)
    where = {int(p): i for i, p in enumerate(idx)}
    assert len(bad) == 0, [(int(p), int(ch), float(cols[where[int(p)], ch]) if int(p) in where else None, int(got[p, ch]), int(want[p, ch]))
                           for p, ch in bad[:6]]
    hit = np.zeros(T * T, bool)
    hit[idx[(idx >= 0) & (idx < T * T)]] = True
    assert (got[~hit] == 0).all()


# ================================================================== k_tex_dilate
PREFILL = 0xAB
DILATE_T = 17
DILATE_FAULTS = ("four_neighbours", "covered_too", "cascade")


def np_dilate(q, covered, fault=None):
    """uint8 [T,T,C]: q where covered; elsewhere the maximum of q over the 3 x 3 neighbourhood, neighbours outside the image not
    taking part (a padded maximum).  fault="zero_border" lets them take part as 0: the same for a maximum of unsigned values."""
    q, covered = np.asarray(q, np.uint8), np.asarray(covered, bool)
    T = q.shape[0]
    if fault == "cascade":                                                # reads the output buffer, texel after texel
        out = np.full_like(q, PREFILL)
        for y in range(T):
            for x in range(T):
                if covered[y, x]:
                    out[y, x] = q[y, x]
                else:
                    out[y, x] = out[max(0, y - 1):y + 2, max(0, x - 1):x + 2].max((0, 1))
        return out
    offs = [(dy, dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if fault != "four_neighbours" or dy == 0 or dx == 0]
    pad = np.full((T + 2, T + 2, q.shape[2]), 0 if fault == "zero_border" else -1, np.int64)      # -1 never wins: the centre takes part
    pad[1:-1, 1:-1] = q
    dil = np.max([pad[1 + dy:T + 1 + dy, 1 + dx:T + 1 + dx] for dy, dx in offs], 0).astype(np.uint8)
    return dil if fault == "covered_too" else np.where(covered[:, :, None], q, dil)


def dilate_case(C, seed=41):
    """covered bool [T,T]: about 30 % at random, the four corners, a run along every border; q uint8 [T,T,C] random everywhere and
    never PREFILL, with covered zeros that have an uncovered 255 beside them"""
    g = rng(seed + C)
    T = DILATE_T
    cov = g.uniform(size=(T, T)) < 0.3
    cov[0, 2:7] = cov[-1, 9:15] = cov[3:9, 0] = cov[8:14, -1] = True
    cov[0, 0] = cov[0, -1] = cov[-1, 0] = cov[-1, -1] = True
    cov[1, 1] = cov[0, 8] = False
    q = g.integers(0, 256, (T, T, C)).astype(np.uint8)
    q[q == PREFILL] = PREFILL + 1
    ys, xs = np.nonzero(cov)
    for y, x in list(zip(ys, xs))[::3]:
        for dy, dx in ((0, 1), (1, 0), (0, -1), (-1, 0), (1, 1), (-1, -1)):
            if 0 <= y + dy < T and 0 <= x + dx < T and not cov[y + dy, x + dx]:
                q[y, x] = 0
                q[y + dy, x + dx] = 255
                break
    return q, cov


def check_dilate(q, covered, got):
    got = np.asarray(got)
    assert got.dtype == np.uint8 and got.shape == q.shape
    assert np.array_equal(got[covered], q[covered])                      # a copy, also where q is 0
    assert not (got == PREFILL).any()                                    # every element written, nothing read from the output buffer
    want = np_dilate(q, covered)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, [(b.tolist(), int(got[tuple(b)]), int(want[tuple(b)])) for b in bad[:6]]
