"""GPU: the device's marching cubes, vertex attributes and connected components on the inputs of tests/isosurface_cases.py.
Every case is checked three ways: against the C restatement exactly (vertex bits, triangles — shared table, shared formulas),
against the table-free float64 reference with the derived bounds of isosurface_cases.py (positions, attributes, the border
fallback bit for bit), and, where the grid is small enough, by oracle/mc_independent.check_mesh with the edge of every vertex
taken from the vertex ORDER.  tests/test_isosurface_hard_host.py shows on the CPU that each of these checks can fail."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

import isosurface_cases as IC
from conftest import REPO

pytestmark = pytest.mark.gpu


def _independent():
    sys.path.insert(0, os.path.join(REPO, "oracle"))
    import mc_independent
    return mc_independent


def _device_mesh(c):
    from sin3dm_amd.encoding.isosurface import marching_cubes
    v, t, a = marching_cubes(torch.tensor(c.grid, device="cuda"), c.iso, c.pad, n_attr=c.n_attr)
    return v.cpu().numpy(), t.cpu().numpy(), (a.cpu().numpy() if a is not None else None)


# ------------------------------------------------------------------ A. marching cubes
@pytest.mark.parametrize("name", [c.name for c in IC.cases()])
def test_device_against_restatement_and_float64(oracle, name):
    c = IC.case(name)
    cut = IC.cut_of(c)
    v, t, a = _device_mesh(c)
    assert len(v) == len(cut.keys)                                              # vertex n is edge n
    v_ref, t_ref = oracle.marching_cubes(c.grid, c.iso, c.pad)
    assert np.array_equal(t, t_ref) and t.dtype == np.int32
    assert np.array_equal(v.view(np.uint32), v_ref.view(np.uint32))
    ratio = IC.check_positions(cut, v)
    aratio = 0.0
    if c.n_attr:
        assert a.shape == (len(v), c.n_attr)
        aratio = IC.check_attributes(c.grid, cut, a, c.n_attr)
    else:
        assert a is None
    print(f"{name}: {len(v)} vertices, {len(t)} triangles; position {ratio:.3f} of its bound, "
          f"{f'attributes {aratio:.3f} of theirs' if c.n_attr else 'no attributes'}, {int((~(cut.a_in & cut.b_in)).sum())} edges into the border")
    if c.small:
        val = c.grid[..., 0] if c.grid.ndim == 4 else c.grid
        stats = _independent().check_mesh(val, v, t, float(np.float32(c.iso)), c.pad, keys=IC.key_list(cut))
        assert stats["triangles"] == len(t)
    if name == "thin_open":
        assert len(v) > 0 and len(t) == 0
    if name == "one_voxel":
        assert (len(v), len(t)) == (6, 8)


def test_attributes_do_not_change_the_mesh():
    from sin3dm_amd.encoding.isosurface import marching_cubes
    c = IC.case("pbr_stride_8")
    g = torch.tensor(c.grid, device="cuda")
    v0, t0, _ = marching_cubes(g[..., 0].contiguous(), c.iso, c.pad)
    v3, t3, a3 = marching_cubes(g, c.iso, c.pad, n_attr=3)
    v8, t8, a8 = marching_cubes(g, c.iso, c.pad, n_attr=8)
    assert torch.equal(v3, v0) and torch.equal(t3, t0) and torch.equal(v8, v0) and torch.equal(t8, t0)
    assert torch.equal(a8[:, :3], a3)                                           # the first channels do not depend on how many are asked for


def test_one_handle_across_sizes():
    """long -> 1 x 1 x 1 -> long on ONE handle: the workspace grown by the first run, barely used by the second, gives the first
    run's bits again"""
    from sin3dm_amd.encoding import isosurface as iso
    big, tiny = IC.case("long"), IC.case("one_voxel")
    v1, t1, _ = _device_mesh(big)
    handle = dict(iso._handles)
    v2, t2, _ = _device_mesh(tiny)
    v3, t3, _ = _device_mesh(big)
    assert {k: h.value for k, h in iso._handles.items()} == {k: h.value for k, h in handle.items()} and len(handle) == 1
    assert (len(v2), len(t2)) == (6, 8)
    assert np.array_equal(v3.view(np.uint32), v1.view(np.uint32)) and np.array_equal(t3, t1)


def test_too_many_attributes_are_refused():
    from sin3dm_amd.encoding.isosurface import marching_cubes
    g = torch.tensor(IC.case("border_sphere_pad").grid, device="cuda")
    assert g.shape[-1] == 4
    with pytest.raises(AssertionError, match="attributes requested"):
        marching_cubes(g, 0.0, 1.0, n_attr=4)


def test_count_refuses_a_grid_whose_edges_do_not_fit_an_int():
    """3 * 902^3 = 2.2e9 edges: below 2^32, above the signed 32-bit item count the scans take.  The refusal comes before the table
    upload, any allocation and any launch — the grid behind the pointer is ONE float."""
    from sin3dm_amd import _lib
    lib = _lib.load()
    assert 2 ** 31 <= 3 * 902 ** 3 < 2 ** 32
    g = torch.zeros(1, device="cuda")
    h = C.c_void_p()
    _lib.check(lib.s3d_mc_create(C.byref(h)))
    try:
        nv, nt = C.c_int64(-7), C.c_int64(-7)
        rc = lib.s3d_mc_count(h, _lib.ptr(g), 900, 900, 900, 1, 0.0, 1, 1.0, C.byref(nv), C.byref(nt), _lib.stream_ptr())
        assert rc == _lib.ERR_UNSUPPORTED and "too large" in _lib.last_error()
        assert (nv.value, nt.value) == (-7, -7)
        with pytest.raises(NotImplementedError):
            _lib.check(rc)
        # the largest cube that is accepted by the rule: 3 * (892 + 2)^3 < 2^31 (not run: it would need the 20 GB)
        assert 3 * 894 ** 3 < 2 ** 31 <= 3 * 895 ** 3
    finally:
        lib.s3d_mc_destroy(h)
    torch.cuda.synchronize()


# ------------------------------------------------------------------ B. components
def _labels(tris, nv):
    from sin3dm_amd.encoding.isosurface import mesh_components
    t = torch.from_numpy(np.ascontiguousarray(tris, np.int32)).reshape(-1, 3).cuda()
    return mesh_components(t, nv).cpu().numpy()


def _blob(oracle):
    """one closed blob (the sphere of case level_sphere), 560 vertices"""
    c = IC.case("level_sphere")
    v, t = oracle.marching_cubes(c.grid, c.iso, c.pad)
    assert len(np.unique(oracle.mesh_components(t, len(v)))) == 1
    return v, t


@pytest.mark.parametrize("name", ["pbr_stride_3", "ties_one", "level_noise", "long"])
def test_components_of_the_noise_meshes(oracle, name):
    c = IC.case(name)
    v, t = oracle.marching_cubes(c.grid, c.iso, c.pad)
    ref = oracle.mesh_components(t, len(v))
    assert len(np.unique(ref)) > 3                                              # many small components next to a large one
    assert np.array_equal(_labels(t, len(v)), ref)


def test_components_edge_cases(oracle):
    v, t = _blob(oracle)
    nv = len(v)
    # unreferenced vertices label themselves
    assert np.array_equal(_labels(t, nv + 7), oracle.mesh_components(t, nv + 7))
    assert np.array_equal(_labels(t, nv + 7)[nv:], np.arange(nv, nv + 7))
    # two blobs that share one vertex are one component
    t2 = t + nv
    t2[t2 == nv + 17] = 5
    both = np.concatenate([t2, t]).astype(np.int32)
    lab = _labels(both, 2 * nv)
    assert np.array_equal(lab, oracle.mesh_components(both, 2 * nv))
    assert lab[nv + 17] == nv + 17 and (np.delete(lab, nv + 17) == 0).all()
    # no triangles
    assert np.array_equal(_labels(np.zeros((0, 3), np.int32), 9), np.arange(9))
    # the 5000-triangle strip with its vertex indices permuted: the minimum no longer travels in index order, and the 4096-iteration
    # cap must not be what ends the loop
    strip, n = IC.strip_permuted()
    lab = _labels(strip, n)
    assert np.array_equal(lab, oracle.mesh_components(strip, n)) and (lab == 0).all()


def test_largest_component_ties_and_attributes(oracle):
    from sin3dm_amd.encoding.isosurface import largest_component
    v, t = _blob(oracle)
    nv = len(v)
    # two disjoint copies with equal face counts, the copy with the LARGER indices first in the face list: the smaller root is kept
    vv = np.concatenate([v, v + np.float32(20.0)])
    tt = np.concatenate([t + nv, t]).astype(np.int32)
    attrs = (np.random.Generator(np.random.PCG64(121)).uniform(-1, 1, (2 * nv, 3)) * np.asarray(IC.ATTR_SCALE)).astype(np.float32)
    v2, t2, a2 = largest_component(torch.from_numpy(vv).cuda(), torch.from_numpy(tt).cuda(), torch.from_numpy(attrs).cuda())
    assert np.array_equal(v2.cpu().numpy(), v) and np.array_equal(t2.cpu().numpy(), t)
    assert np.array_equal(a2.cpu().numpy().view(np.uint32), attrs[:nv].view(np.uint32))
    # a noise mesh: the kept vertices and attribute rows are those of the restatement's largest component, exactly
    c = IC.case("ties_one")
    v, t = oracle.marching_cubes(c.grid, c.iso, c.pad)
    ref = oracle.mesh_components(t, len(v))
    roots, counts = np.unique(ref[t[:, 0]], return_counts=True)
    keep_v = ref == roots[np.argmax(counts)]
    attrs = (np.random.Generator(np.random.PCG64(122)).uniform(-1, 1, (len(v), 3)) * np.asarray(IC.ATTR_SCALE)).astype(np.float32)
    v2, t2, a2 = largest_component(torch.from_numpy(v).cuda(), torch.from_numpy(t).cuda(), torch.from_numpy(attrs).cuda())
    assert np.array_equal(v2.cpu().numpy(), v[keep_v]) and len(t2) == int(counts.max())
    assert np.array_equal(a2.cpu().numpy().view(np.uint32), attrs[keep_v].view(np.uint32))
    assert np.array_equal(t2.cpu().numpy(), (np.cumsum(keep_v) - 1)[t[keep_v[t[:, 0]]]])
