"""GPU: quadric-error decimation (isosurface.simplify_mesh_quadric, s3d_qem.hip) — the properties it promises on
closed, open and pinched meshes, one round against the NumPy restatement of tests/test_qem_host.py, and its distance from the
input surface next to the vertex clustering's.  Parity with open3d's simplify_quadric_decimation is not claimed and not tested."""
import numpy as np
import pytest
import torch

import test_qem_host as H

pytestmark = pytest.mark.gpu

# float64 restatement vs the device's fp32-rounded outputs on the two iso-surfaces below, measured on an MI355X:
# target 5.23e-8 of the largest coordinate (box; torus 4.27e-8), cost 5.81e-8 relative (box; torus 5.52e-8) — both just under
# half an fp32 ulp, 5.96e-8, the rounding of the outputs.  The bounds are ten times the larger figure.
TARGET_TOL, COST_TOL = 5.23e-7, 5.81e-7
# RMS distance of the input vertices from the decimated surface of the box at a fiftieth of its faces, measured on an MI355X
# (profiles/qem.txt): vertex clustering CLUSTER_RMS, quadric QUADRIC_RMS, in grid cells.  The gate keeps half of that margin.
CLUSTER_RMS, QUADRIC_RMS = 1.19070, 0.00525


def _field(kind, n=None):
    """box: a box with a box-shaped hole through it along z (sharp edges, genus 1), on a 44^3 grid; torus: a torus with bumps
    (smooth, genus 1), on a 48^3 grid (or on n^3).  The offsets keep the surface off the grid points."""
    n = n or {"box": 44, "torus": 48}[kind]
    ax = np.linspace(-1, 1, n)
    x, y, z = np.meshgrid(ax + 0.0131, ax * 0.95 - 0.0072, ax * 1.05 + 0.0057, indexing="ij")
    if kind == "box":
        box = np.maximum(np.maximum(np.abs(x) - 0.71, np.abs(y) - 0.62), np.abs(z) - 0.53)
        hole = np.maximum(np.abs(x) - 0.31, np.abs(y) - 0.27)
        return np.maximum(box, -hole).astype(np.float32)
    f = np.sqrt((np.sqrt(x * x + y * y) - 0.6) ** 2 + z * z) - 0.24 + 0.03 * np.sin(7 * x) * np.sin(5 * y + 1) * np.sin(6 * z + 2)
    return f.astype(np.float32)


@pytest.fixture(scope="module")
def meshes():
    """the two iso-surfaces, with two attribute channels, built once"""
    from sin3dm_amd.encoding.isosurface import largest_component, marching_cubes
    out = {}
    for kind in ("box", "torus"):
        v, t, _ = marching_cubes(torch.from_numpy(_field(kind)).cuda(), 0.0, 1.0)
        v, t, _ = largest_component(v, t)
        attrs = torch.sin(v * 0.37 + 1.0)[:, :2].contiguous()
        vn, tn = v.cpu().numpy(), t.cpu().numpy()
        assert H.is_closed_manifold(tn, len(vn)) and H.euler_characteristic(tn, len(vn)) == 0, kind      # closed, genus 1
        out[kind] = (v.contiguous(), t.contiguous(), attrs)
    return out


def _check_output(v2, t2, info, n_in):
    """no repeated index, no unreferenced vertex, vmap points at output vertices"""
    t2n = t2.cpu().numpy()
    assert t2.dtype == torch.int32 and v2.dtype == torch.float32
    assert ((t2n[:, 0] != t2n[:, 1]) & (t2n[:, 1] != t2n[:, 2]) & (t2n[:, 0] != t2n[:, 2])).all()
    assert np.array_equal(np.unique(t2n), np.arange(len(v2)))
    vmap = info["vmap"].cpu().numpy()
    assert vmap.shape == (n_in,) and vmap.min() >= 0 and vmap.max() == len(v2) - 1
    return t2n, vmap


# ------------------------------------------------------------------ properties
@pytest.mark.parametrize("divisor", [4, 50])
@pytest.mark.parametrize("kind", ["box", "torus"])
def test_closed_manifold_stays_closed_manifold(meshes, kind, divisor):
    from sin3dm_amd.encoding.isosurface import simplify_mesh_quadric
    v, t, attrs = meshes[kind]
    n_faces = t.shape[0] // divisor
    v_in, t_in, a_in = v.clone(), t.clone(), attrs.clone()
    v2, t2, info = simplify_mesh_quadric(v, t, n_faces, attrs=attrs)
    assert torch.equal(v, v_in) and torch.equal(t, t_in) and torch.equal(attrs, a_in)          # the input is left alone
    t2n, vmap = _check_output(v2, t2, info, len(v))
    print(f"{kind}: {t.shape[0]} faces -> {len(t2n)} (budget {n_faces}) in {info['rounds']} rounds, stuck {info['stuck']}; "
          f"collapses per round {[c for c, _ in info['per_round']]}")
    assert info["stuck"] is False and n_faces - 2 < len(t2n) <= n_faces
    assert info["rounds"] == len(info["per_round"]) and info["per_round"][-1][1] == len(t2n)
    faces = t.shape[0]
    for c, f in info["per_round"]:
        assert c >= 1 and f == faces - 2 * c                                                     # a collapse takes two faces
        faces = f
    rep = H.manifold_report(t2n, len(v2))
    assert all(x == 0 for x in rep.values()), rep
    assert H.n_components(t2n, len(v2)) == 1 and H.euler_characteristic(t2n, len(v2)) == 0
    # the surviving faces keep their order: face k of the output is the k-th input face that vmap leaves with three vertices
    m = vmap[t.cpu().numpy()]
    alive = (m[:, 0] != m[:, 1]) & (m[:, 1] != m[:, 2]) & (m[:, 0] != m[:, 2])
    assert np.array_equal(m[alive], t2n)
    # attributes: inside the range of the input vertices merged into the vertex
    a_out, a_np = info["attrs"].cpu().numpy(), attrs.cpu().numpy()
    assert a_out.shape == (len(v2), 2)
    lo, hi = np.full(a_out.shape, np.inf), np.full(a_out.shape, -np.inf)
    np.minimum.at(lo, vmap, a_np)
    np.maximum.at(hi, vmap, a_np)
    assert (a_out >= lo).all() and (a_out <= hi).all()
    # same input, same bits
    v3, t3, info3 = simplify_mesh_quadric(v, t, n_faces, attrs=attrs)
    assert torch.equal(v3, v2) and torch.equal(t3, t2) and torch.equal(info3["vmap"], info["vmap"])
    assert torch.equal(info3["attrs"], info["attrs"]) and info3["per_round"] == info["per_round"]


def test_boundary_vertices_do_not_move(meshes):
    from sin3dm_amd.encoding.isosurface import simplify_mesh_quadric
    v, t, _ = meshes["torus"]
    keep = torch.ones(t.shape[0], dtype=torch.bool, device=t.device)
    assert t.shape[0] > 4000
    keep[[5, 6, 7, 1000, 1001, 4000]] = False                                    # a few faces deleted: boundary loops
    t_open = t[keep].contiguous()
    tn, vn = t_open.cpu().numpy(), v.cpu().numpy()
    eu, ev, cnt = H.mesh_edges(tn, len(vn))
    bverts = np.unique(np.concatenate([eu[cnt == 1], ev[cnt == 1]]))
    assert len(bverts) >= 9 and (cnt <= 2).all()
    n_faces = t_open.shape[0] // 10
    v2, t2, info = simplify_mesh_quadric(v, t_open, n_faces)
    t2n = t2.cpu().numpy()
    vmap = info["vmap"].cpu().numpy()
    referenced = np.unique(tn)
    assert (vmap[referenced] >= 0).all() and not info["stuck"] and n_faces - 2 < len(t2n) <= n_faces
    assert len(np.unique(vmap[bverts])) == len(bverts)                            # no two boundary vertices were merged
    assert np.array_equal(v2.cpu().numpy()[vmap[bverts]], vn[bverts])            # ... and each sits where it sat
    eu2, ev2, cnt2 = H.mesh_edges(t2n, len(v2))
    assert (cnt2 <= 2).all() and (cnt2 == 1).sum() == (cnt == 1).sum()          # nothing non-manifold, and the same boundary edges
    bu, bv = vmap[eu[cnt == 1]], vmap[ev[cnt == 1]]
    assert np.array_equal(np.sort(np.minimum(bu, bv) * len(v2) + np.maximum(bu, bv)), eu2[cnt2 == 1] * len(v2) + ev2[cnt2 == 1])


def test_pinch_and_tiny_meshes():
    from sin3dm_amd.encoding.isosurface import simplify_mesh_quadric
    dev = torch.device("cuda")
    # a pinch: nothing may collapse, everything comes back where it was
    vn, tn = H.two_tetrahedra()
    v, t = torch.from_numpy(vn).to(dev), torch.from_numpy(tn).to(dev)
    v2, t2, info = simplify_mesh_quadric(v, t, 4)
    assert info["stuck"] is True and info["rounds"] == 0 and torch.equal(v2, v) and torch.equal(t2, t)
    assert np.array_equal(info["vmap"].cpu().numpy(), np.arange(7))
    # a tetrahedron: stuck
    vn, tn = H.tetrahedron()
    v, t = torch.from_numpy(vn).to(dev), torch.from_numpy(tn).to(dev)
    v2, t2, info = simplify_mesh_quadric(v, t, 2)
    assert info["stuck"] is True and torch.equal(v2, v) and torch.equal(t2, t)
    # already inside the budget: returned as it is
    v2, t2, info = simplify_mesh_quadric(v, t, 4)
    assert v2 is v and t2 is t and info["stuck"] is False and info["rounds"] == 0 and info["per_round"] == []
    assert np.array_equal(info["vmap"].cpu().numpy(), np.arange(4))
    # an octahedron: one collapse per round (any two of its edges have neighbouring ends), down to a tetrahedron
    vn, tn = H.octahedron()
    v, t = torch.from_numpy(vn).to(dev), torch.from_numpy(tn).to(dev)
    for budget, rounds in ((7, 1), (6, 1), (4, 2)):
        v2, t2, info = simplify_mesh_quadric(v, t, budget)
        t2n, vmap = _check_output(v2, t2, info, 6)
        assert len(t2n) == 2 * (budget // 2) and info["rounds"] == rounds and not info["stuck"]
        assert [c for c, _ in info["per_round"]] == [1] * rounds
        assert H.is_closed_manifold(t2n, len(v2)) and H.euler_characteristic(t2n, len(v2)) == 2
    with pytest.raises(ValueError):
        simplify_mesh_quadric(v, t, -1)


# ------------------------------------------------------------------ one round against the restatement
@pytest.mark.parametrize("kind", ["box", "torus"])
def test_one_round_against_numpy(meshes, kind):
    from sin3dm_amd.encoding import isosurface as iso
    v, t, _ = meshes[kind]
    vn, tn = v.cpu().numpy(), t.cpu().numpy().astype(np.int64)
    nv = len(vn)
    _, _, info = iso.simplify_mesh_quadric(v, t, t.shape[0] // 2, max_rounds=1, return_round=True)
    rd = {k: x.cpu().numpy() for k, x in info["round"].items()}
    eu, ev, cnt = H.mesh_edges(tn, nv)
    assert np.array_equal(rd["eu"], eu) and np.array_equal(rd["ev"], ev) and np.array_equal(rd["edge_faces"], cnt)
    assert np.array_equal(rd["verts"], vn) and np.array_equal(rd["tris"], tn)
    # cost and target: float64 evaluation of the same formulas
    Q = H.np_quadrics(vn, tn)
    cost, target, solved = H.np_cost_target(vn, Q, eu, ev)
    scale = float(np.abs(vn).max())
    tgt_gap = float(np.abs(rd["target"].astype(np.float64) - target).max() / scale)
    qe = Q[eu] + Q[ev]
    magnitude = (qe[:, 0, 0] + qe[:, 1, 1] + qe[:, 2, 2]) * (1.0 + (target ** 2).sum(1))          # the size of the terms that cancel
    cost_gap = float((np.abs(rd["cost"].astype(np.float64) - cost) / (cost + 1e-7 * magnitude)).max())
    print(f"{kind}: {len(eu)} edges, {int(solved.sum())} solved; target gap {tgt_gap:.3e} of the largest coordinate {scale:.1f}, "
          f"cost gap {cost_gap:.3e} relative (floor 1e-7 of the cancelling terms)")
    assert tgt_gap <= TARGET_TOL and cost_gap <= COST_TOL
    assert solved.any() and (~solved).any()                                # both branches of the rule are exercised
    assert (solved.mean() > 0.5) if kind == "torus" else ((~solved).mean() > 0.5)
    # integer tests: exactly
    flags = rd["flags"]
    assert np.array_equal((flags & iso.QEM_TWO_FACES) != 0, cnt == 2) and (cnt == 2).all()
    assert not rd["frozen"].any() and ((flags & iso.QEM_NOT_FROZEN) != 0).all()
    link = H.np_link(tn, nv, eu, ev)
    assert np.array_equal((flags & iso.QEM_LINK) != 0, link)
    print(f"  link condition holds on {int(link.sum())} of {len(eu)} edges")
    # the flip test on the device's own fp32 targets, compared where the restatement's cosine is clear of the margin
    flip, gap = H.np_flip(vn, tn, eu, ev, rd["target"])
    clear = gap > 1e-4
    share = 1.0 - clear.mean()
    print(f"  flip test passes on {int(flip.sum())} edges; {share * 100:.3f} % of the edges lie within 1e-4 of the margin")
    assert share <= 0.01
    assert np.array_equal(((flags & iso.QEM_NO_FLIP) != 0)[clear], flip[clear])
    assert 0 < flip.sum()
    # keys and the selected set: the rule applied to the device's own costs and flags
    valid = flags == iso.QEM_VALID
    assert np.array_equal(rd["keys"], H.np_keys(rd["cost"]))
    sel = H.np_select(nv, eu, ev, rd["keys"], valid)
    assert np.array_equal(rd["selected"], sel) and sel.sum() > 0
    ends = np.concatenate([eu[sel], ev[sel]])
    assert len(np.unique(ends)) == len(ends)                               # independent: no shared endpoint ...
    mark = np.zeros(nv, np.int64)
    mark[eu[sel]] = mark[ev[sel]] = np.arange(1, sel.sum() + 1)
    both = (mark[eu] > 0) & (mark[ev] > 0)
    assert (mark[eu][both] == mark[ev][both]).all()                        # ... and no edge between two of them
    # the cut to the budget: the cheapest ceil((faces - n_faces) / 2) keys
    need = (len(tn) - len(tn) // 2 + 1) // 2
    want = np.flatnonzero(sel)[np.argsort(rd["keys"][sel])[:need]] if sel.sum() > need else np.flatnonzero(sel)
    assert np.array_equal(rd["chosen"], want)
    print(f"  {int(valid.sum())} valid edges, {int(sel.sum())} selected, {len(want)} collapsed")


# ------------------------------------------------------------------ quality next to the vertex clustering
def _rms_to_surface(points, v2, t2):
    from sin3dm_amd.data.mesh_sampler import MeshSampler
    ms = MeshSampler(verts=v2.cpu().numpy(), faces=t2.cpu().numpy())
    dist, face, _ = ms.closest(points, band=8.0)
    assert int((face < 0).sum()) == 0                                      # every input vertex found the surface inside the band
    return float(torch.sqrt((dist.double() ** 2).mean()))


def test_quadric_is_closer_to_the_surface_than_clustering(meshes):
    """At the same budget (a fiftieth of the faces of the box with its hole) the input vertices lie closer, in RMS by the exact
    closest-point kernel, to the quadric result than to the clustering's: below it by at least half the margin measured."""
    from sin3dm_amd.encoding.isosurface import simplify_mesh, simplify_mesh_quadric
    v, t, _ = meshes["box"]
    n_faces = t.shape[0] // 50
    vq, tq, iq = simplify_mesh_quadric(v, t, n_faces)
    vc, tc, ic = simplify_mesh(v, t, n_faces)
    rq, rc = _rms_to_surface(v, vq, tq), _rms_to_surface(v, vc, tc)
    print(f"box, {t.shape[0]} faces, budget {n_faces}: clustering {tc.shape[0]} faces RMS {rc:.5f}, quadric {tq.shape[0]} faces RMS {rq:.5f} "
          f"(grid cells), ratio {rq / rc:.4f}")
    assert rq < rc
    assert rq / rc <= 1.0 - 0.5 * (1.0 - QUADRIC_RMS / CLUSTER_RMS)


# ------------------------------------------------------------------ the export
def test_sample_cli_quadric(tmp_path, monkeypatch):
    """S3D_MESH=textured S3D_DECIMATE=quadric: the CLI writes a valid textured OBJ whose mesh is inside the budget; without
    S3D_DECIMATE decode writes what S3D_DECIMATE=cluster writes, byte for byte, and that is another mesh"""
    import os
    import shutil
    from test_cli_gpu import make_experiment
    from test_texmesh_gpu import _check_textured_obj
    from sin3dm_amd import sample
    from sin3dm_amd.utils import parser_util as pu
    tag = make_experiment(str(tmp_path))
    argv = ["--tag", tag, "--n_samples", "1", "--use_ddim", "True", "--timestep_respacing", "5", "--reso", "48", "--n_faces", "2000",
            "--texreso", "512"]
    monkeypatch.setenv("S3D_MESH", "textured")
    monkeypatch.setenv("S3D_DECIMATE", "quadric")
    paths = sample.main(argv + ["--output", "quadric"])
    folder = os.path.dirname(paths[0])
    lo, hi = np.asarray([-0.72, -1.0, -0.72]), np.asarray([0.72, 1.0, 0.72])
    pv, pvt, pf, png = _check_textured_obj(folder, 512, lo, hi, 48, 2000)
    tris = pf[:, :, 0] - 1
    assert 0 < len(tris) <= 2000 and png.max() > 0
    assert H.manifold_report(tris, len(pv))["repeated_index"] == 0 and np.array_equal(np.unique(tris), np.arange(len(pv)))
    args = pu.sample_args(argv)
    files = {}
    for name in ("", "cluster"):
        monkeypatch.setenv("S3D_DECIMATE", name)
        out = os.path.join(tag, "again", name or "unset")
        os.makedirs(out)
        shutil.copy(paths[0], os.path.join(out, "feat.npz"))
        sample.decode(args, [os.path.join(out, "feat.npz")])
        files[name] = {f: open(os.path.join(out, f), "rb").read() for f in ("object.obj", "object.mtl", "object.png")}
    assert files[""] == files["cluster"]
    assert files[""]["object.obj"] != open(os.path.join(folder, "object.obj"), "rb").read()
    monkeypatch.setenv("S3D_DECIMATE", "open3d")
    with pytest.raises(ValueError):
        sample.decode(args, [paths[0]])
