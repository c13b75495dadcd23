"""GPU: EVERY round of the quadric decimation replayed in float64 (isosurface.simplify_mesh_quadric(..., return_round="all"),
s3d_qem.hip).  test_qem_gpu.py holds the first round against NumPy and the later ones by properties of the final
mesh; k_qem_apply, though, writes state that only later rounds read — the accumulated quadrics, the interpolated attributes, the
moved vertex, the parent map.  check_trace below follows the device's choices round by round (it never makes a tie decision of its
own) and holds each round's structure, quadrics, costs, targets, flags, selection and apply step against the NumPy restatement of
tests/test_qem_host.py; tests/test_qem_rounds_host.py runs the same checker on a NumPy float32 model of the rounds and on that
model with faults put in, so every check is known to be able to fail.  Each failure names its check in square brackets.

Bounds (u32 = 2^-24, u64 = 2^-53):
  quadrics of round 0   per vertex (n_w + 16) u64 * 3 A_w max(1, M^2): n_w faces at the vertex, A_w their area sum, M the largest
                        coordinate — every term is area * p_i p_j with |p_i p_j| <= 3 M^2, summed in double.
  quadrics afterwards   Q[u] + Q[v] is ONE IEEE addition per entry: bit for bit; every other row unchanged in bits.
  cost, target          TARGET_TOL, COST_TOL and the metrics of test_qem_gpu.test_one_round_against_numpy, from the device's own Q
                        and vertices of that round.  No edge is excluded: instead every decision of the target rule (determinant,
                        reach, endpoint against midpoint) must stand clear of its threshold by more than 1e-12 relative, 10^4
                        double round-offs.  If that ever fails the INPUT has to change, not the edge be masked.
  flip flag             exact where the restatement's cosine is more than 1e-4 from the margin; at most 0.5 % of a round's edges
                        may be that close.
  attributes            a64 = (1 - t) a_u + t a_v, t = clamp(<x - p_u, d> / |d|^2, 0, 1) in float64 from the stored fp32 target:
                        8 u32 max(|a_u|, |a_v|), and inside [min, max] of the two."""
import numpy as np
import pytest

import test_qem_host as H
from test_qem_gpu import COST_TOL, TARGET_TOL, _field

pytestmark = pytest.mark.gpu

U32, U64 = 2.0 ** -24, 2.0 ** -53
CLEAR = 1e-12                                # the decisions of the target rule stand clear of their thresholds by more than this
FLIP_CLEAR, FLIP_SHARE = 1e-4, 0.005
QEM_TWO_FACES, QEM_NOT_FROZEN, QEM_LINK, QEM_NO_FLIP, QEM_VALID = 1, 2, 4, 8, 15
ATTR_SCALE = np.asarray([1.0, 1e3, 1e-3])
_Q10 = ((0, 0), (0, 1), (0, 2), (0, 3), (1, 1), (1, 2), (1, 3), (2, 2), (2, 3), (3, 3))      # xx xy xz xw yy yz yw zz zw ww

# name -> (field, grid, faces removed, divisor of the face count, faces expected)
MESHES = {"box20": ("box", 20, (), 10, 2048), "torus20": ("torus", 20, (), 10, 1424), "box28": ("box", 28, (), 25, 4080),
          "torus20_open": ("torus", 20, (5, 6, 7, 700, 701, 1400), 10, 1418)}


def field_of(name):
    kind, n = MESHES[name][:2]
    return _field(kind, n)


def finish_mesh(name, v, t):
    """(verts, tris, attrs, n_faces) of a MESHES entry from the largest component of its iso-surface"""
    _, _, removed, divisor, faces = MESHES[name]
    keep = np.ones(len(t), bool)
    keep[list(removed)] = False
    assert len(t) == faces + len(removed), (name, len(t))
    t = np.ascontiguousarray(t[keep])
    return v, t, vertex_attrs(len(v)), len(t) // divisor


def vertex_attrs(nv, seed=7):
    """three channels of per-vertex noise scaled 1, 1e3 and 1e-3"""
    return (np.random.Generator(np.random.PCG64(seed)).uniform(-1, 1, (nv, 3)) * ATTR_SCALE).astype(np.float32)


def q10_to_44(Q):
    out = np.zeros((len(Q), 4, 4))
    for c, (i, j) in enumerate(_Q10):
        out[:, i, j] = out[:, j, i] = Q[:, c]
    return out


def q44_to_10(Q):
    return np.ascontiguousarray(np.stack([Q[:, i, j] for i, j in _Q10], 1))


def _fail(tag, r, msg):
    raise AssertionError(f"[{tag}] round {r}: {msg}")


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view({4: np.uint32, 8: np.uint64}[x.dtype.itemsize]) if x.dtype.kind == "f" else x


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def decision_margins(v, Q, eu, ev):
    """How far the float64 restatement's three decisions of the target rule (np_cost_target, s3d_mesh_qem_edge_cost) stand from
    their thresholds, relative: (determinant, reach, endpoint against midpoint), the smallest over the edges each applies to."""
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
    thr = H.DET_REL * tr ** 3
    m_det = np.abs(np.abs(det) - thr) / np.maximum(np.maximum(np.abs(det), thr), 1e-300)
    good = np.abs(det) > thr
    d = np.where(good, det, 1.0)
    x = -np.stack([c00 * xw + c01 * yw + c02 * zw, c01 * xw + c11 * yw + c12 * zw, c02 * xw + c12 * yw + c22 * zw], 1) / d[:, None]
    r2, lim = ((x - mid) ** 2).sum(1), H.REACH ** 2 * len2
    m_reach = np.abs(r2 - lim) / np.maximum(np.maximum(r2, lim), 1e-300)
    solved = good & (r2 <= lim)
    c = H.np_eval(q, np.where(solved[:, None], x, mid))
    size = 3.0 * tr * (1.0 + (mid ** 2).sum(1))
    tol = H.TIE_REL * size
    cu, cv = H.np_eval(q, pu), H.np_eval(q, pv)
    m_u = np.abs(cu - (c - tol)) / size
    c2 = np.where(cu < c - tol, cu, c)
    m_v = np.abs(cv - (c2 - tol)) / size
    m_tie = np.minimum(m_u, m_v)
    return (float(m_det.min()), float(m_reach[good].min()) if good.any() else np.inf,
            float(m_tie[~solved].min()) if (~solved).any() else np.inf)


def check_round0_quadrics(st):
    """[quadrics-0] the device's initial quadrics against np_quadrics, per vertex within the bound in the module docstring"""
    v, t = st["verts"], st["tris"].astype(np.int64)
    ref = q44_to_10(H.np_quadrics(v, t))
    p = v.astype(np.float64)[t]
    area = 0.5 * np.linalg.norm(np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]), axis=1)
    n_w, A_w = np.zeros(len(v)), np.zeros(len(v))
    for k in range(3):
        np.add.at(n_w, t[:, k], 1.0)
        np.add.at(A_w, t[:, k], area)
    M = float(np.abs(v).max())
    bound = (n_w + 16.0) * U64 * 3.0 * A_w * max(1.0, M * M)
    err = np.abs(st["Q"] - ref).max(1)
    ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
    if ratio.max() > 1.0:
        w = int(np.argmax(ratio))
        _fail("quadrics-0", 0, f"vertex {w}: {st['Q'][w].tolist()} against {ref[w].tolist()}, {ratio.max():.3f} of the bound")
    return float(ratio.max())


def check_trace(trace, out, n_faces, has_attrs=True):
    """trace: the entries of info["trace"] as NumPy arrays; out: the returned verts, tris, attrs, vmap.  Raises AssertionError
    "[check] round r: ..." at the first thing that is off; returns the figures of the run."""
    nv = len(trace[0]["verts"])
    fig = {"rounds": 0, "quadrics0": check_round0_quadrics(trace[0]), "target_gap": 0.0, "cost_gap": 0.0, "flip_share": 0.0,
           "det_margin": np.inf, "reach_margin": np.inf, "tie_margin": np.inf, "frozen": 0, "collapses": 0}
    for r, (E, N) in enumerate(zip(trace[:-1], trace[1:])):
        v, t, Q = E["verts"], E["tris"].astype(np.int64), E["Q"]
        nf = len(t)
        # 1. structure
        eu, ev, cnt = H.mesh_edges(t, nv)
        if not (np.array_equal(E["eu"], eu) and np.array_equal(E["ev"], ev) and np.array_equal(E["edge_faces"], cnt)):
            _fail("structure", r, "eu / ev / edge_faces are not the edges of this round's faces")
        fr = H.np_frozen(nv, eu, ev, cnt)
        if not np.array_equal(E["frozen"].astype(bool), fr):
            _fail("frozen", r, f"{int((E['frozen'].astype(bool) != fr).sum())} frozen marks differ")
        flags = E["flags"]
        if not np.array_equal((flags & QEM_TWO_FACES) != 0, cnt == 2):
            _fail("frozen", r, "QEM_TWO_FACES is not `the edge has two faces`")
        if not np.array_equal((flags & QEM_NOT_FROZEN) != 0, ~fr[eu] & ~fr[ev]):
            _fail("frozen", r, "QEM_NOT_FROZEN is not `neither endpoint is frozen`")
        fig["frozen"] = max(fig["frozen"], int(fr.sum()))
        # 4. cost and target from the device's own quadrics and vertices
        Q4 = q10_to_44(Q)
        cost, target, solved = H.np_cost_target(v, Q4, eu, ev)
        m_det, m_reach, m_tie = decision_margins(v, Q4, eu, ev)
        if min(m_det, m_reach, m_tie) <= CLEAR:
            _fail("decision-margin", r, f"a decision of the target rule lies within {CLEAR} of its threshold (determinant {m_det:.3e}, "
                  f"reach {m_reach:.3e}, endpoint {m_tie:.3e}): change the input mesh")
        fig["det_margin"], fig["reach_margin"] = min(fig["det_margin"], m_det), min(fig["reach_margin"], m_reach)
        fig["tie_margin"] = min(fig["tie_margin"], m_tie)
        scale = float(np.abs(v).max())
        tgt_gap = float(np.abs(E["target"].astype(np.float64) - target).max() / scale)
        qe = Q4[eu] + Q4[ev]
        magnitude = (qe[:, 0, 0] + qe[:, 1, 1] + qe[:, 2, 2]) * (1.0 + (target ** 2).sum(1))
        cost_gap = float((np.abs(E["cost"].astype(np.float64) - cost) / (cost + 1e-7 * magnitude)).max())
        fig["target_gap"], fig["cost_gap"] = max(fig["target_gap"], tgt_gap), max(fig["cost_gap"], cost_gap)
        if tgt_gap > TARGET_TOL:
            _fail("target", r, f"gap {tgt_gap:.3e} of the largest coordinate, bound {TARGET_TOL:.3e}")
        if cost_gap > COST_TOL:
            _fail("cost", r, f"gap {cost_gap:.3e} relative, bound {COST_TOL:.3e}")
        # 5. flags
        link = H.np_link(t, nv, eu, ev)
        if not np.array_equal((flags & QEM_LINK) != 0, link):
            _fail("link", r, f"{int((((flags & QEM_LINK) != 0) != link).sum())} link flags differ")
        flip, gap = H.np_flip(v, t, eu, ev, E["target"])
        clear = gap > FLIP_CLEAR
        share = 1.0 - float(clear.mean())
        fig["flip_share"] = max(fig["flip_share"], share)
        if share > FLIP_SHARE:
            _fail("flip", r, f"{share * 100:.3f} % of the edges lie within {FLIP_CLEAR} of the flip margin, cap {FLIP_SHARE * 100} %")
        if not np.array_equal(((flags & QEM_NO_FLIP) != 0)[clear], flip[clear]):
            _fail("flip", r, f"{int((((flags & QEM_NO_FLIP) != 0)[clear] != flip[clear]).sum())} flip flags differ clear of the margin")
        # 6. selection, from the device's own costs and flags
        valid = flags == QEM_VALID
        if not np.array_equal(E["keys"], H.np_keys(E["cost"])):
            _fail("keys", r, "keys are not (bits of the fp32 cost << 32) | mix(edge index)")
        sel = H.np_select(nv, eu, ev, E["keys"], valid)
        if not np.array_equal(E["selected"].astype(bool), sel):
            _fail("selection", r, f"{int((E['selected'].astype(bool) != sel).sum())} edges selected differently")
        need = (nf - n_faces + 1) // 2
        want = np.flatnonzero(sel)[np.argsort(E["keys"][sel])[:need]] if sel.sum() > need else np.flatnonzero(sel)
        chosen = E["chosen"].astype(np.int64)
        if not np.array_equal(chosen, want):
            _fail("selection", r, f"chosen is not the selected set cut to the cheapest {need}")
        u, w = eu[chosen], ev[chosen]
        if len(np.unique(np.concatenate([u, w]))) != 2 * len(chosen):
            _fail("selection", r, "two chosen edges share an endpoint")
        fig["collapses"] += len(chosen)
        # 3. quadrics: one IEEE addition per entry for the collapsed, nothing for the rest
        Qn = Q.copy()
        Qn[u] = Q[u] + Q[w]
        if not _same(N["Q"][u], Qn[u]):
            k = int(np.flatnonzero((_bits(N["Q"][u]) != _bits(Qn[u])).any(1))[0])
            _fail("quadric-sum", r, f"the quadric of vertex {u[k]} after the collapse of ({u[k]}, {w[k]}) is not Q_u + Q_v in bits: "
                  f"{N['Q'][u[k]].tolist()} against {Qn[u[k]].tolist()}")
        if not _same(N["Q"], Qn):
            _fail("quadric-untouched", r, f"{int((_bits(N['Q']) != _bits(Qn)).any(1).sum())} quadrics of vertices that were not collapsed changed")
        # 7. apply
        vn = v.copy()
        vn[u] = E["target"][chosen]
        if not _same(N["verts"][u], vn[u]):
            k = int(np.flatnonzero((_bits(N["verts"][u]) != _bits(vn[u])).any(1))[0])
            _fail("apply-target", r, f"vertex {u[k]} is at {N['verts'][u[k]].tolist()}, the target of its edge is {vn[u[k]].tolist()}")
        if not _same(N["verts"], vn):
            _fail("apply-verts-untouched", r, f"{int((_bits(N['verts']) != _bits(vn)).any(1).sum())} vertices that were not collapsed moved")
        pn = E["parent"].copy()
        pn[w] = u
        if not np.array_equal(N["parent"], pn):
            _fail("apply-parent", r, f"parent differs from `v -> u for the chosen, the rest unchanged` at {np.flatnonzero(N['parent'] != pn)[:8].tolist()}")
        if has_attrs:
            a, an = E["attrs"], N["attrs"]
            p64, x64 = v.astype(np.float64), E["target"].astype(np.float64)[chosen]
            d = p64[w] - p64[u]
            len2 = (d * d).sum(1)
            tt = np.where(len2 > 0, np.clip(((x64 - p64[u]) * d).sum(1) / np.where(len2 > 0, len2, 1.0), 0.0, 1.0), 0.0)
            au, av = a[u].astype(np.float64), a[w].astype(np.float64)
            ref = (1.0 - tt)[:, None] * au + tt[:, None] * av
            bound = 8.0 * U32 * np.maximum(np.abs(au), np.abs(av))
            err = np.abs(an[u].astype(np.float64) - ref)
            if (err > bound).any():
                k = int(np.argmax((err - bound).max(1)))
                _fail("apply-attrs", r, f"attributes of vertex {u[k]} after the collapse of ({u[k]}, {w[k]}) at t = {tt[k]:.6f}: "
                      f"{an[u[k]].tolist()} against {ref[k].tolist()} (a_u {a[u[k]].tolist()}, a_v {a[w[k]].tolist()})")
            if not ((an[u] >= np.minimum(a[u], a[w])) & (an[u] <= np.maximum(a[u], a[w]))).all():
                _fail("apply-attrs", r, "an interpolated attribute lies outside [min, max] of the two it came from")
            rest = np.ones(nv, bool)
            rest[u] = False
            if not _same(an[rest], a[rest]):
                _fail("apply-attrs-untouched", r, "attribute rows of vertices that were not collapsed changed")
        m = np.arange(nv)
        m[w] = u
        tn = m[t]
        tn = tn[(tn[:, 0] != tn[:, 1]) & (tn[:, 1] != tn[:, 2]) & (tn[:, 0] != tn[:, 2])]
        if not np.array_equal(N["tris"].astype(np.int64), tn):
            _fail("apply-faces", r, "the faces are not the remap and drop of the round's faces, in order")
        if len(chosen) and len(tn) != nf - 2 * len(chosen):
            _fail("apply-faces", r, f"{len(chosen)} collapses took {nf - len(tn)} faces away")
        fig["rounds"] += int(len(chosen) > 0)
    # 8. the end: compaction of the last state, the parent chain followed to its root
    L = trace[-1]
    t = L["tris"].astype(np.int64)
    root = L["parent"].astype(np.int64)
    for _ in range(nv + 1):
        nxt = root[root]
        if np.array_equal(nxt, root):
            break
        root = nxt
    used = np.zeros(nv, bool)
    used[t.reshape(-1)] = True
    remap = np.cumsum(used) - 1
    r = len(trace) - 1
    if not _same(out["verts"], L["verts"][used]):
        _fail("end", r, "the returned vertices are not the referenced ones of the last state")
    if not np.array_equal(out["tris"].astype(np.int64), remap[t]):
        _fail("end", r, "the returned faces are not the last state's, renumbered")
    if has_attrs and not _same(out["attrs"], L["attrs"][used]):
        _fail("end", r, "the returned attributes are not the referenced rows of the last state")
    if not np.array_equal(out["vmap"].astype(np.int64), np.where(used[root], remap[root], -1)):
        _fail("end", r, "vmap is not the root of the parent chain, renumbered")
    return fig


def format_figures(name, faces, n_faces, fig):
    return (f"{name}: {faces} faces -> budget {n_faces} in {fig['rounds']} rounds, {fig['collapses']} collapses; quadrics of round 0 "
            f"{fig['quadrics0']:.3f} of the bound; worst target gap {fig['target_gap']:.3e} (bound {TARGET_TOL:.3e}), cost gap "
            f"{fig['cost_gap']:.3e} (bound {COST_TOL:.3e}); largest share of edges within {FLIP_CLEAR} of the flip margin "
            f"{fig['flip_share'] * 100:.3f} % (cap {FLIP_SHARE * 100} %); margins of the target rule: determinant {fig['det_margin']:.2e}, "
            f"reach {fig['reach_margin']:.2e}, endpoint {fig['tie_margin']:.2e}; frozen vertices {fig['frozen']}")


# ------------------------------------------------------------------ the device runs
def _to_np(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else x


def device_trace(v, t, attrs, n_faces):
    import torch
    from sin3dm_amd.encoding.isosurface import simplify_mesh_quadric
    vd, td = torch.from_numpy(v).cuda(), torch.from_numpy(np.ascontiguousarray(t, np.int32)).cuda()
    ad = torch.from_numpy(attrs).cuda() if attrs is not None else None
    v2, t2, info = simplify_mesh_quadric(vd, td, n_faces, attrs=ad, return_round="all")
    trace = [{k: _to_np(x) for k, x in e.items() if x is not None} for e in info["trace"]]
    out = {"verts": _to_np(v2), "tris": _to_np(t2), "attrs": _to_np(info["attrs"]) if ad is not None else None, "vmap": _to_np(info["vmap"])}
    # the trace changes no arithmetic: the plain call returns the same bits
    v3, t3, info3 = simplify_mesh_quadric(vd, td, n_faces, attrs=ad)
    assert torch.equal(v3, v2) and torch.equal(t3, t2) and torch.equal(info3["vmap"], info["vmap"]) and "trace" not in info3
    assert ad is None or torch.equal(info3["attrs"], info["attrs"])
    assert info3["per_round"] == info["per_round"] and info3["stuck"] == info["stuck"]
    return trace, out, info


@pytest.mark.parametrize("name", list(MESHES))
def test_every_round_against_float64(name):
    import torch
    from sin3dm_amd.encoding.isosurface import largest_component, marching_cubes
    v, t, _ = marching_cubes(torch.from_numpy(field_of(name)).cuda(), 0.0, 1.0)
    v, t, _ = largest_component(v, t)
    v, t, attrs, n_faces = finish_mesh(name, v.cpu().numpy(), t.cpu().numpy())
    trace, out, info = device_trace(v, t, attrs, n_faces)
    fig = check_trace(trace, out, n_faces)
    print(format_figures(name, len(t), n_faces, fig))
    assert not info["stuck"] and n_faces - 2 < len(out["tris"]) <= n_faces
    assert fig["rounds"] == info["rounds"] == len(trace) - 1 and fig["rounds"] > 10            # the later rounds are what this is about
    assert [len(e["chosen"]) for e in trace[:-1]] == [c for c, _ in info["per_round"]]
    if name == "torus20_open":
        assert fig["frozen"] >= 9                                  # the boundary loops freeze their vertices: the flags are not trivial
        assert any(((e["flags"] & QEM_TWO_FACES) == 0).any() for e in trace[:-1])
    else:
        assert fig["frozen"] == 0
    if name == "box28":                                            # the last round is cut to the budget
        last = trace[-2]
        assert len(last["chosen"]) < int(last["selected"].sum())


def test_octahedron_every_round():
    v, t = H.octahedron()
    trace, out, info = device_trace(v, t, vertex_attrs(6), 4)
    fig = check_trace(trace, out, 4)
    print(format_figures("octahedron", 8, 4, fig))
    assert fig["rounds"] == info["rounds"] == 2 and len(out["tris"]) == 4 and not info["stuck"]
