"""CPU-only: what the quadric decimation's GPU tests stand on — the pure-NumPy closed-manifold check on known good and bad meshes,
the NumPy restatement of one round (quadrics, cost and target, link condition, flip test, selection rule; float64 and integers)
on meshes whose answers are known by hand — and the S3D_DECIMATE parsing of the sampling CLI."""
import numpy as np
import pytest

NO_KEY = np.int64(0x7FFFFFFFFFFFFFFF)
DET_REL, REACH, TIE_REL, FLIP_COS = 1e-6, 2.0, 1e-10, 0.2               # the constants of s3d_qem.hip


# ------------------------------------------------------------------ meshes
def tetrahedron():
    v = np.asarray([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32)
    t = np.asarray([[0, 2, 1], [0, 1, 3], [1, 2, 3], [0, 3, 2]], np.int32)
    return v, t


def octahedron():
    v = np.asarray([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float32)
    t = np.asarray([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]], np.int32)
    return v, t


def two_tetrahedra():
    """two tetrahedra that share vertex 0 and nothing else: every edge has two faces, vertex 0 has two face fans"""
    v, t = tetrahedron()
    v2 = -v[1:]
    t2 = np.where(t == 0, 0, t + 3)[:, [0, 2, 1]]                       # mirrored through the origin: flip to keep it outward
    return np.concatenate([v, v2]), np.concatenate([t, t2]).astype(np.int32)


def grid_torus(n=12, m=8, R=1.0, r=0.4):
    """a closed genus-1 surface as an n x m quad grid, every quad cut in two"""
    i, j = np.meshgrid(np.arange(n), np.arange(m), indexing="ij")
    a, b = 2 * np.pi * i / n, 2 * np.pi * j / m
    v = np.stack([(R + r * np.cos(b)) * np.cos(a), (R + r * np.cos(b)) * np.sin(a), r * np.sin(b)], -1).reshape(-1, 3).astype(np.float32)
    idx = lambda p, q: (p % n) * m + (q % m)
    t = np.concatenate([np.stack([idx(i, j), idx(i + 1, j), idx(i + 1, j + 1)], -1).reshape(-1, 3),
                        np.stack([idx(i, j), idx(i + 1, j + 1), idx(i, j + 1)], -1).reshape(-1, 3)]).astype(np.int32)
    return v, t


# ------------------------------------------------------------------ the closed-manifold check
def mesh_edges(t, nv):
    """(eu, ev, count) of the undirected edges, ascending in eu * nv + ev"""
    t = np.asarray(t, np.int64)
    a, b = t.reshape(-1), t[:, [1, 2, 0]].reshape(-1)
    key, cnt = np.unique(np.minimum(a, b) * nv + np.maximum(a, b), return_counts=True)
    return key // nv, key % nv, cnt


def n_components(t, nv):
    """connected components among the vertices that faces reference"""
    eu, ev, _ = mesh_edges(t, nv)
    lab = np.arange(nv)
    while True:
        new = lab.copy()
        np.minimum.at(new, eu, lab[ev])
        np.minimum.at(new, ev, lab[eu])
        new = new[new]
        if np.array_equal(new, lab):
            break
        lab = new
    return len(np.unique(lab[np.unique(t)]))


def euler_characteristic(t, nv):
    return len(np.unique(t)) - len(mesh_edges(t, nv)[0]) + len(t)


def manifold_report(t, nv):
    """Pure NumPy.  dict of the counts that must all be 0 for a closed manifold: faces with a repeated index, undirected edges
    without exactly two faces, directed edges that appear more than once, vertices whose faces form more than one fan (two
    faces at a vertex belong to one fan when they share an edge at that vertex)."""
    t = np.asarray(t, np.int64)
    nf = len(t)
    rep = {"repeated_index": int(((t[:, 0] == t[:, 1]) | (t[:, 1] == t[:, 2]) | (t[:, 0] == t[:, 2])).sum())}
    a, b = t.reshape(-1), t[:, [1, 2, 0]].reshape(-1)                   # half-edge h = 3 f + k runs from corner k to corner k + 1
    _, _, cnt = mesh_edges(t, nv)
    rep["edges_not_two_faces"] = int((cnt != 2).sum())
    rep["directed_edge_repeated"] = int(len(a) - len(np.unique(a * nv + b)))
    rep["vertex_fans_extra"] = -1
    if rep["edges_not_two_faces"] == 0 and rep["repeated_index"] == 0:
        order = np.argsort(np.minimum(a, b) * nv + np.maximum(a, b), kind="stable")
        h0, h1 = order[0::2], order[1::2]                              # the two half-edges of every edge
        mate = np.empty(3 * nf, np.int64)
        mate[h0], mate[h1] = h1, h0
        # node = (face, corner); half-edge h touches corner h (its start) and corner next(h) (its end); the same vertex on the mate
        nxt = (np.arange(3 * nf) // 3) * 3 + (np.arange(3 * nf) + 1) % 3
        prv = (np.arange(3 * nf) // 3) * 3 + (np.arange(3 * nf) + 2) % 3
        h = np.arange(3 * nf)
        same_dir = a[mate] == a                                          # the mate runs the same way (inconsistent orientation)
        start_partner = np.where(same_dir, mate, nxt[mate])              # the mate's corner at this half-edge's start vertex
        # the half-edge that ENDS at corner h is prv(h); its mate's corner at that vertex
        hp = prv[h]
        end_partner = np.where(a[mate[hp]] == a[hp], nxt[mate[hp]], mate[hp])
        lab = np.arange(3 * nf)
        while True:
            new = np.minimum(lab, np.minimum(lab[start_partner], lab[end_partner]))
            if np.array_equal(new, lab):
                break
            lab = new
        fans = len(np.unique(a * (3 * nf) + lab))
        rep["vertex_fans_extra"] = int(fans - len(np.unique(a)))
    return rep


def is_closed_manifold(t, nv):
    r = manifold_report(t, nv)
    return all(x == 0 for x in r.values())


# ------------------------------------------------------------------ one round, restated in float64 and integers
def np_quadrics(v, t):
    """[nv,4,4] float64: the sum over the faces at a vertex of area * p p^T, p the unit plane (faces without area skipped)"""
    v = np.asarray(v, np.float64)
    a, b, c = v[t[:, 0]], v[t[:, 1]], v[t[:, 2]]
    n = np.cross(b - a, c - a)
    ln = np.linalg.norm(n, axis=1)
    ok = ln > 0
    p = np.zeros((len(t), 4))
    p[ok, :3] = n[ok] / ln[ok, None]
    p[:, 3] = -np.einsum("ij,ij->i", p[:, :3], a)
    K = (0.5 * ln)[:, None, None] * p[:, :, None] * p[:, None, :]
    Q = np.zeros((len(v), 4, 4))
    for k in range(3):
        np.add.at(Q, t[:, k], K)
    return Q


def np_eval(Q, x):
    return np.einsum("ni,nij,nj->n", x, Q[:, :3, :3], x) + 2 * np.einsum("ni,ni->n", Q[:, :3, 3], x) + Q[:, 3, 3]


def np_cost_target(v, Q, eu, ev):
    """(cost, target, solved) per edge in float64 by the rule of s3d_mesh_qem_edge_cost"""
    v = np.asarray(v, np.float64)
    q = Q[eu] + Q[ev]
    pu, pv = v[eu], v[ev]
    mid = 0.5 * (pu + pv)
    len2 = ((pv - pu) ** 2).sum(1)
    xx, xy, xz, xw, yy, yz, yw, zz, zw = (q[:, 0, 0], q[:, 0, 1], q[:, 0, 2], q[:, 0, 3], q[:, 1, 1], q[:, 1, 2], q[:, 1, 3], q[:, 2, 2],
                                          q[:, 2, 3])
    c00, c01, c02 = yy * zz - yz * yz, xz * yz - xy * zz, xy * yz - xz * yy
    c11, c12, c22 = xx * zz - xz * xz, xy * xz - xx * yz, xx * yy - xy * xy
    det = xx * c00 + xy * c01 + xz * c02
    tr = (xx + yy + zz) / 3.0
    good = np.abs(det) > DET_REL * tr ** 3
    d = np.where(good, det, 1.0)
    x = -np.stack([c00 * xw + c01 * yw + c02 * zw, c01 * xw + c11 * yw + c12 * zw, c02 * xw + c12 * yw + c22 * zw], 1) / d[:, None]
    solved = good & (((x - mid) ** 2).sum(1) <= REACH ** 2 * len2)
    best = np.where(solved[:, None], x, mid)
    c = np_eval(q, best)
    tol = TIE_REL * 3.0 * tr * (1.0 + (mid ** 2).sum(1))
    cu, cv = np_eval(q, pu), np_eval(q, pv)
    take_u = ~solved & (cu < c - tol)
    c, best = np.where(take_u, cu, c), np.where(take_u[:, None], pu, best)
    take_v = ~solved & (cv < c - tol)
    c, best = np.where(take_v, cv, c), np.where(take_v[:, None], pv, best)
    return np.maximum(c, 0.0), best, solved


def np_link(t, nv, eu, ev):
    """bool per edge, integers only: u and v have exactly two common neighbours w1 < w2, and the faces {u, w1, w2} and
    {v, w1, w2} do not both exist"""
    t = np.asarray(t, np.int64)
    au, av, _ = mesh_edges(t, nv)
    adj = [[] for _ in range(nv)]
    for x, y in zip(au.tolist(), av.tolist()):
        adj[x].append(y)
        adj[y].append(x)
    faces = {tuple(sorted(f)) for f in t.tolist()}
    out = np.zeros(len(eu), bool)
    for i, (u, v) in enumerate(zip(np.asarray(eu).tolist(), np.asarray(ev).tolist())):
        common = sorted(set(adj[u]) & set(adj[v]))
        if len(common) != 2:
            continue
        w1, w2 = common
        out[i] = not (tuple(sorted((u, w1, w2))) in faces and tuple(sorted((v, w1, w2))) in faces)
    return out


def np_flip(v, t, eu, ev, target):
    """(ok bool per edge, gap per edge): every face at u or v that does not hold both keeps, with that vertex at the target, a
    non-zero area and a cosine above FLIP_COS with its old normal; gap = the smallest |cosine - FLIP_COS| among those faces"""
    v = np.asarray(v, np.float64)
    t = np.asarray(t, np.int64)
    nf, ne = len(t), len(eu)
    corner_v = t.reshape(-1)
    order = np.argsort(corner_v, kind="stable")
    off = np.zeros(len(v) + 1, np.int64)
    off[1:] = np.cumsum(np.bincount(corner_v, minlength=len(v)))
    ok, gap = np.ones(ne, bool), np.full(ne, np.inf)
    for w, other in ((np.asarray(eu, np.int64), np.asarray(ev, np.int64)), (np.asarray(ev, np.int64), np.asarray(eu, np.int64))):
        deg = off[w + 1] - off[w]
        e = np.repeat(np.arange(ne), deg)
        j = np.arange(deg.sum()) - np.repeat(np.cumsum(deg) - deg, deg) + np.repeat(off[w], deg)
        f = order[j] // 3
        tri = t[f]
        use = ~(tri == other[e][:, None]).any(1)
        e, tri = e[use], tri[use]
        p = v[tri]
        n0 = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
        r = np.where((tri == w[e][:, None])[:, :, None], np.asarray(target, np.float64)[e][:, None, :], p)
        n1 = np.cross(r[:, 1] - r[:, 0], r[:, 2] - r[:, 0])
        l0, l1 = (n0 * n0).sum(1), (n1 * n1).sum(1)
        den = np.sqrt(l0 * l1)
        cos = np.where(den > 0, (n0 * n1).sum(1) / np.where(den > 0, den, 1.0), -1.0)
        good = (l1 > 0) & ((n0 * n1).sum(1) > FLIP_COS * den)
        np.logical_and.at(ok, e, good)
        np.minimum.at(gap, e, np.abs(cos - FLIP_COS))
    return ok, gap


def np_frozen(nv, eu, ev, cnt):
    fr = np.zeros(nv, bool)
    fr[eu[cnt != 2]] = True
    fr[ev[cnt != 2]] = True
    return fr


def np_select(nv, eu, ev, keys, valid):
    """the selection rule on given keys and validity: m1 = min key of the valid edges at a vertex, m2 = min of m1 over the
    vertex and its neighbours (along ALL edges), selected iff valid and key == m2[u] == m2[v]"""
    keys = np.asarray(keys, np.int64)
    m1 = np.full(nv, NO_KEY, np.int64)
    np.minimum.at(m1, eu[valid], keys[valid])
    np.minimum.at(m1, ev[valid], keys[valid])
    m2 = m1.copy()
    np.minimum.at(m2, eu, m1[ev])
    np.minimum.at(m2, ev, m1[eu])
    return valid & (keys == m2[eu]) & (keys == m2[ev])


def np_mix(i):
    """the 32-bit bijection that scatters the edge index in a key"""
    m = np.uint64(0xFFFFFFFF)
    i = np.asarray(i, np.uint64) & m
    i = (i * np.uint64(0x9E3779B1)) & m
    i ^= i >> np.uint64(16)
    i = (i * np.uint64(0x85EBCA6B)) & m
    i ^= i >> np.uint64(13)
    return i.astype(np.int64)


def np_keys(cost32):
    return (np.asarray(cost32, np.float32).view(np.uint32).astype(np.int64) << 32) | np_mix(np.arange(len(cost32)))


def np_round(v, t):
    """one whole round in NumPy: edges, cost, target, the four tests, keys from the fp32-rounded cost, the selected set"""
    nv = len(v)
    eu, ev, cnt = mesh_edges(t, nv)
    cost, target, _ = np_cost_target(v, np_quadrics(v, t), eu, ev)
    target32 = target.astype(np.float32)
    fr = np_frozen(nv, eu, ev, cnt)
    link = np_link(t, nv, eu, ev)
    flip, _ = np_flip(v, t, eu, ev, target32)
    valid = (cnt == 2) & ~fr[eu] & ~fr[ev] & link & flip
    keys = np_keys(cost.astype(np.float32))
    return {"eu": eu, "ev": ev, "cost": cost, "target": target32, "valid": valid, "keys": keys, "link": link, "flip": flip, "frozen": fr,
            "selected": np_select(nv, eu, ev, keys, valid)}


def np_decimate(v, t, n_faces, max_rounds=1000):
    """the rounds of simplify_mesh_quadric on the host (positions only): the algorithm's own claims — a closed manifold stays
    one, the budget is met to within one face — can be held without a device"""
    v, t = np.array(v, np.float32), np.array(t, np.int64)
    nv = len(v)
    Q = None
    rounds = 0
    while len(t) > n_faces and rounds < max_rounds:
        eu, ev, cnt = mesh_edges(t, nv)
        if Q is None:
            Q = np_quadrics(v, t)
        cost, target, _ = np_cost_target(v, Q, eu, ev)
        target32 = target.astype(np.float32)
        fr = np_frozen(nv, eu, ev, cnt)
        valid = (cnt == 2) & ~fr[eu] & ~fr[ev] & np_link(t, nv, eu, ev) & np_flip(v, t, eu, ev, target32)[0]
        keys = np_keys(cost.astype(np.float32))
        chosen = np.flatnonzero(np_select(nv, eu, ev, keys, valid))
        need = (len(t) - n_faces + 1) // 2
        chosen = chosen[np.argsort(keys[chosen])[:need]]
        if len(chosen) == 0:
            return v, t, rounds, True
        u, w = eu[chosen], ev[chosen]
        assert len(np.unique(np.concatenate([u, w]))) == 2 * len(chosen)
        v[u] = target32[chosen]
        Q[u] += Q[w]
        vmap = np.arange(nv)
        vmap[w] = u
        t = vmap[t]
        t = t[(t[:, 0] != t[:, 1]) & (t[:, 1] != t[:, 2]) & (t[:, 0] != t[:, 2])]
        rounds += 1
    return v, t, rounds, False


# ------------------------------------------------------------------ tests of the helpers
def test_manifold_check_on_known_meshes():
    for v, t in (tetrahedron(), octahedron(), grid_torus()):
        rep = manifold_report(t, len(v))
        assert all(x == 0 for x in rep.values()), rep
    v, t = tetrahedron()
    assert euler_characteristic(t, 4) == 2 and n_components(t, 4) == 1
    v, t = grid_torus()
    assert euler_characteristic(t, len(v)) == 0 and n_components(t, len(v)) == 1
    # a boundary: one face missing
    assert manifold_report(octahedron()[1][1:], 6)["edges_not_two_faces"] == 3
    # an inconsistently oriented face: a directed edge twice
    bad = octahedron()[1].copy()
    bad[0] = bad[0][[0, 2, 1]]
    rep = manifold_report(bad, 6)
    assert rep["edges_not_two_faces"] == 0 and rep["directed_edge_repeated"] == 3 and not is_closed_manifold(bad, 6)
    # a pinch: every edge has two faces, one vertex has two fans
    v, t = two_tetrahedra()
    rep = manifold_report(t, len(v))
    assert rep == {"repeated_index": 0, "edges_not_two_faces": 0, "directed_edge_repeated": 0, "vertex_fans_extra": 1}, rep
    assert n_components(t, len(v)) == 1 and euler_characteristic(t, len(v)) == 3
    # a repeated index; a face twice (three edges with three faces)
    assert manifold_report(np.asarray([[0, 0, 1]]), 2)["repeated_index"] == 1
    dup = np.concatenate([octahedron()[1], octahedron()[1][:1]])
    assert manifold_report(dup, 6)["edges_not_two_faces"] == 3
    # two components
    v, t = tetrahedron()
    assert n_components(np.concatenate([t, t + 4]), 8) == 2 and is_closed_manifold(np.concatenate([t, t + 4]), 8)


def test_round_restatement_on_meshes_known_by_hand():
    # the tetrahedron: every edge has its two common neighbours, and both faces over them exist -> no link, nothing valid
    v, t = tetrahedron()
    r = np_round(v, t)
    assert len(r["eu"]) == 6 and not r["link"].any() and not r["valid"].any() and not r["selected"].any()
    # the octahedron: every edge passes the link condition; the quadric of an edge is minimised inside, targets stay near
    v, t = octahedron()
    r = np_round(v, t)
    assert len(r["eu"]) == 12 and r["link"].all() and not r["frozen"].any()
    # the quadric of a vertex vanishes on the planes of its faces: the cost of staying put is 0 to rounding
    Q = np_quadrics(v, t)
    assert np.abs(np_eval(Q, v.astype(np.float64))).max() < 1e-14
    assert len(np.unique(np_mix(np.arange(1 << 16)))) == 1 << 16 and np_mix([0, 1, 2, 3]).tolist() == [0, 1678549374, 4256427940, 2630778099]
    # selected edges are pairwise non-adjacent: no endpoint shared, no edge between endpoints
    sel = np.flatnonzero(r["selected"])
    assert len(sel) >= 1 or not r["valid"].any()
    # the pinch: nothing can collapse
    v, t = two_tetrahedra()
    assert not np_round(v, t)["valid"].any()
    # a boundary freezes its vertices
    v, t = grid_torus()
    r = np_round(v, t[3:])
    assert r["frozen"].sum() > 0 and not r["valid"][r["frozen"][r["eu"]] | r["frozen"][r["ev"]]].any()


def test_selection_is_independent_and_rounds_keep_a_closed_manifold():
    v, t = grid_torus(24, 12)
    r = np_round(v, t)
    sel = np.flatnonzero(r["selected"])
    assert len(sel) > 1
    ends = np.concatenate([r["eu"][sel], r["ev"][sel]])
    assert len(np.unique(ends)) == 2 * len(sel)
    edge_set = set((r["eu"] * len(v) + r["ev"]).tolist())
    owner = np.concatenate([sel, sel])
    for i in range(len(ends)):
        for j in range(i + 1, len(ends)):
            if owner[i] != owner[j]:
                a, b = sorted((int(ends[i]), int(ends[j])))
                assert a * len(v) + b not in edge_set
    for budget in (200, 60, 24):
        v2, t2, rounds, stuck = np_decimate(v, t, budget)
        assert not stuck and budget - 2 < len(t2) <= budget, (budget, len(t2), stuck)
        assert is_closed_manifold(t2, len(v)) and euler_characteristic(t2, len(v)) == 0 and n_components(t2, len(v)) == 1
    v2, t2, rounds, stuck = np_decimate(*tetrahedron(), 2)
    assert stuck and len(t2) == 4 and rounds == 0
    v2, t2, rounds, stuck = np_decimate(*octahedron(), 4)
    assert not stuck and len(t2) == 4 and is_closed_manifold(t2, 6)


# ------------------------------------------------------------------ S3D_DECIMATE
def test_decimation_mode_from_the_environment(monkeypatch):
    from sin3dm_amd import sample
    monkeypatch.delenv("S3D_DECIMATE", raising=False)
    assert sample.decimation_mode() == "cluster"
    monkeypatch.setenv("S3D_DECIMATE", "")
    assert sample.decimation_mode() == "cluster"
    monkeypatch.setenv("S3D_DECIMATE", "cluster")
    assert sample.decimation_mode() == "cluster"
    monkeypatch.setenv("S3D_DECIMATE", "quadric")
    assert sample.decimation_mode() == "quadric"
    monkeypatch.setenv("S3D_DECIMATE", "open3d")
    with pytest.raises(ValueError) as e:
        sample.decimation_mode()
    assert "open3d" in str(e.value)
    assert sample.decimation_mode("quadric") == "quadric"                       # an explicit argument wins over the environment


def test_decode_passes_the_decimation_on(monkeypatch, tmp_path):
    """sample.decode hands decimation="quadric" to decode_texmesh only under S3D_DECIMATE=quadric; the default call is unchanged"""
    import os
    from types import SimpleNamespace
    import torch
    from sin3dm_amd import sample
    from sin3dm_amd.encoding import model
    from sin3dm_amd.utils import triplane_util
    calls = []

    class FakeAE:
        def __init__(self, *a, **k):
            pass

        def load_ckpt(self, name):
            pass

        def decode_texmesh(self, save_dir, fm, reso, **kw):
            calls.append(kw)
    monkeypatch.setattr(model, "ShapeAutoEncoder", FakeAE)
    monkeypatch.setattr(triplane_util, "load_triplane_data", lambda path, device=None, compose=True: [torch.zeros(2, 3, 3)] * 3)
    monkeypatch.setattr(sample.dist_util, "dev", lambda: torch.device("cpu"))
    args = SimpleNamespace(tag=str(tmp_path / "exp"), vox=False, reso=48, n_faces=500, texreso=256, file_format="obj", copy_mtl=False,
                           data_path=None)
    path = str(tmp_path / "exp" / "results" / "000" / "feat.npz")
    monkeypatch.setenv("S3D_MESH", "textured")
    monkeypatch.delenv("S3D_DECIMATE", raising=False)
    sample.decode(args, [path])
    monkeypatch.setenv("S3D_DECIMATE", "quadric")
    sample.decode(args, [path])
    assert "decimation" not in calls[0] and calls[1]["decimation"] == "quadric"
    assert {k: x for k, x in calls[1].items() if k != "decimation"} == calls[0]
    monkeypatch.setenv("S3D_DECIMATE", "foo")
    with pytest.raises(ValueError):
        sample.decode(args, [path])
    assert os.path.basename(path) == "feat.npz"


def test_decode_texmesh_rejects_an_unknown_decimation():
    from sin3dm_amd.encoding.model import ShapeAutoEncoder
    with pytest.raises(ValueError) as e:
        ShapeAutoEncoder.decode_texmesh(object(), "x", None, 8, decimation="open3d")
    assert "open3d" in str(e.value)
