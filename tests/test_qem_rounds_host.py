"""CPU-only: the round-by-round checker of tests/test_qem_rounds_gpu.py must pass on a correct run and must be able to fail.
A NumPy float32 model of the rounds of simplify_mesh_quadric (the restatement of test_qem_host.py, with the outputs rounded where
the device rounds them) writes a trace in the device's format; check_trace passes on it, and reports each fault put into it by
the check meant for that fault."""
import copy

import numpy as np
import pytest

import test_qem_host as H
import test_qem_rounds_gpu as G


def model_trace(v, t, attrs, n_faces, max_rounds=1000):
    """(trace, out): the rounds on the host, every stored quantity in the device's type"""
    v, t = np.array(v, np.float32), np.array(t, np.int32)
    at = np.array(attrs, np.float32)
    nv = len(v)
    Q = G.q44_to_10(H.np_quadrics(v, t.astype(np.int64)))
    parent = np.arange(nv, dtype=np.int32)
    trace = []

    def state():
        return {"verts": v.copy(), "tris": t.copy(), "Q": Q.copy(), "attrs": at.copy(), "parent": parent.copy()}
    while len(t) > n_faces and len(trace) < max_rounds:
        tl = t.astype(np.int64)
        eu, ev, cnt = H.mesh_edges(tl, nv)
        cost, target, _ = H.np_cost_target(v, G.q10_to_44(Q), eu, ev)
        cost32, target32 = cost.astype(np.float32), target.astype(np.float32)
        fr = H.np_frozen(nv, eu, ev, cnt)
        link, flip = H.np_link(tl, nv, eu, ev), H.np_flip(v, tl, eu, ev, target32)[0]
        flags = ((cnt == 2) * G.QEM_TWO_FACES + (~fr[eu] & ~fr[ev]) * G.QEM_NOT_FROZEN + link * G.QEM_LINK + flip * G.QEM_NO_FLIP).astype(np.int32)
        keys = H.np_keys(cost32)
        sel = H.np_select(nv, eu, ev, keys, flags == G.QEM_VALID)
        chosen = np.flatnonzero(sel)
        need = (len(t) - n_faces + 1) // 2
        if len(chosen) > need:
            chosen = chosen[np.argsort(keys[chosen])[:need]]
        trace.append(dict(state(), eu=eu.astype(np.int32), ev=ev.astype(np.int32), edge_faces=cnt.astype(np.int32), cost=cost32,
                          target=target32, flags=flags, frozen=fr, keys=keys, selected=sel, chosen=chosen))
        if len(chosen) == 0:
            break
        u, w = eu[chosen], ev[chosen]
        p = v.astype(np.float64)
        d = p[w] - p[u]
        tt = np.clip(((target32[chosen].astype(np.float64) - p[u]) * d).sum(1) / (d * d).sum(1), 0.0, 1.0).astype(np.float32)[:, None]
        au, av = at[u], at[w]
        at[u] = np.minimum(np.maximum((np.float32(1) - tt) * au + tt * av, np.minimum(au, av)), np.maximum(au, av))
        v[u] = target32[chosen]
        Q[u] = Q[u] + Q[w]
        parent[w] = u
        m = parent[t]
        t = np.ascontiguousarray(m[(m[:, 0] != m[:, 1]) & (m[:, 1] != m[:, 2]) & (m[:, 0] != m[:, 2])])
    trace.append(state())
    root = parent.astype(np.int64)
    while not np.array_equal(root[root], root):
        root = root[root]
    used = np.zeros(nv, bool)
    used[t.reshape(-1)] = True
    remap = np.cumsum(used) - 1
    out = {"verts": v[used], "tris": remap[t].astype(np.int32), "attrs": at[used], "vmap": np.where(used[root], remap[root], -1).astype(np.int32)}
    return trace, out


@pytest.fixture(scope="module")
def host_meshes(oracle):
    """the meshes of the GPU test from the C restatement of the iso-surface, their model traces computed once"""
    out = {}
    for name in G.MESHES:
        v, t = oracle.marching_cubes(G.field_of(name), 0.0, 1.0)
        lab = oracle.mesh_components(t, len(v))
        roots, counts = np.unique(lab[t[:, 0]], return_counts=True)
        best = roots[np.argmax(counts)]
        keep_v = lab == best
        remap = np.cumsum(keep_v) - 1
        v, t = v[keep_v], remap[t[lab[t[:, 0]] == best]].astype(np.int32)
        v, t, attrs, n_faces = G.finish_mesh(name, v, t)
        out[name] = (v, t, attrs, n_faces) + model_trace(v, t, attrs, n_faces)
    return out


@pytest.mark.parametrize("name", list(G.MESHES))
def test_checker_passes_on_the_model(host_meshes, name):
    v, t, attrs, n_faces, trace, out = host_meshes[name]
    fig = G.check_trace(trace, out, n_faces)
    print(G.format_figures(name, len(t), n_faces, fig))
    assert n_faces - 2 < len(out["tris"]) <= n_faces and fig["rounds"] == len(trace) - 1 > 10
    assert fig["quadrics0"] == 0.0                                   # the model's quadrics ARE np_quadrics
    assert (fig["frozen"] >= 9) == (name == "torus20_open")
    # the margins this file's docstring and DESIGN.md quote: far from the 1e-12 the checker asks for
    assert fig["det_margin"] > 1e-4 and fig["reach_margin"] > 1e-3 and fig["tie_margin"] > 0.99e-10
    assert fig["flip_share"] <= 0.001


def test_checker_passes_on_the_octahedron():
    v, t = H.octahedron()
    trace, out = model_trace(v, t, G.vertex_attrs(6), 4)
    fig = G.check_trace(trace, out, 4)
    assert fig["rounds"] == 2 and len(out["tris"]) == 4


# ------------------------------------------------------------------ faults
def _pick(trace, want):
    """(round, k): the first collapse k of a round >= 3 for which want(E, u, v, k) holds"""
    for r in range(3, len(trace) - 1):
        E = trace[r]
        for k, e in enumerate(E["chosen"]):
            if want(E, int(E["eu"][e]), int(E["ev"][e]), k):
                return r, k
    raise AssertionError("no collapse of the trace fits the fault")


def _t_of(E, u, v, k):
    p = E["verts"].astype(np.float64)
    d = p[v] - p[u]
    return float(np.clip(((E["target"][E["chosen"][k]].astype(np.float64) - p[u]) * d).sum() / (d * d).sum(), 0.0, 1.0))


def _fault_without_qv(trace):
    r, k = _pick(trace, lambda E, u, v, k: np.abs(E["Q"][v]).max() > 0)
    E = trace[r]
    trace[r + 1]["Q"][E["eu"][E["chosen"][k]]] = E["Q"][E["eu"][E["chosen"][k]]]


def _fault_qv_twice(trace):
    r, k = _pick(trace, lambda E, u, v, k: np.abs(E["Q"][v]).max() > 0)
    E = trace[r]
    u, v = E["eu"][E["chosen"][k]], E["ev"][E["chosen"][k]]
    trace[r + 1]["Q"][u] = E["Q"][u] + E["Q"][v] + E["Q"][v]


def _fault_one_minus_t(trace):
    r, k = _pick(trace, lambda E, u, v, k: abs(_t_of(E, u, v, k) - 0.5) > 0.2)
    E = trace[r]
    u, v = E["eu"][E["chosen"][k]], E["ev"][E["chosen"][k]]
    t = np.float32(_t_of(E, u, v, k))
    trace[r + 1]["attrs"][u] = t * E["attrs"][u] + (np.float32(1) - t) * E["attrs"][v]


def _fault_midpoint(trace):
    def off_mid(E, u, v, k):
        mid = (0.5 * (E["verts"][u].astype(np.float64) + E["verts"][v])).astype(np.float32)
        return not np.array_equal(mid, E["target"][E["chosen"][k]])
    r, k = _pick(trace, off_mid)
    E = trace[r]
    u, v = E["eu"][E["chosen"][k]], E["ev"][E["chosen"][k]]
    trace[r + 1]["verts"][u] = (0.5 * (E["verts"][u].astype(np.float64) + E["verts"][v])).astype(np.float32)


def _fault_parent_left(trace):
    r, k = _pick(trace, lambda E, u, v, k: True)
    v = trace[r]["ev"][trace[r]["chosen"][k]]
    trace[r + 1]["parent"][v] = v


def _fault_untouched_ulp(trace):
    r, _ = _pick(trace, lambda E, u, v, k: True)
    E = trace[r]
    rest = np.setdiff1d(np.unique(E["tris"]), E["eu"][E["chosen"]])
    w = rest[len(rest) // 2]
    x = trace[r + 1]["verts"][w, 1]
    trace[r + 1]["verts"][w, 1] = np.nextafter(x, np.float32(np.inf))


FAULTS = {"one collapse without its Q_v": (_fault_without_qv, "quadric-sum"),
          "one collapse with Q_v twice": (_fault_qv_twice, "quadric-sum"),
          "1 - t for t in one attribute row": (_fault_one_minus_t, "apply-attrs"),
          "one vertex moved to the midpoint instead of the target": (_fault_midpoint, "apply-target"),
          "one parent entry left alone": (_fault_parent_left, "apply-parent"),
          "one untouched vertex row perturbed by 1 ulp": (_fault_untouched_ulp, "apply-verts-untouched")}


@pytest.mark.parametrize("fault", list(FAULTS))
def test_checker_reports_the_fault(host_meshes, fault):
    v, t, attrs, n_faces, trace, out = host_meshes["torus20"]
    bad = copy.deepcopy(trace)
    inject, tag = FAULTS[fault]
    inject(bad)
    with pytest.raises(AssertionError, match=rf"^\[{tag}\] round \d+"):
        G.check_trace(bad, out, n_faces)
