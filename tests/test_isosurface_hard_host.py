"""CPU-only: the float64 references of tests/isosurface_cases.py against the C restatement of marching cubes, on the inputs where
marching cubes is delicate — values equal to the level, t rounded to 1, levels other than 0, a border value other than 1,
one-voxel-thick grids, attributes on edges into the virtual border — and the proof that each check can fail.  The C restatement
has no attributes: those are checked on a NumPy float32 model of the kernel's formula.  The device runs the same checks in
tests/test_isosurface_hard_gpu.py."""
import os
import sys

import numpy as np
import pytest

import isosurface_cases as IC
from conftest import REPO


def _independent():
    sys.path.insert(0, os.path.join(REPO, "oracle"))
    import mc_independent
    return mc_independent


def _value(c):
    return c.grid[..., 0] if c.grid.ndim == 4 else c.grid


@pytest.mark.parametrize("name", [c.name for c in IC.cases()])
def test_restatement_against_float64(oracle, name):
    c = IC.case(name)
    cut = IC.cut_of(c)
    v, t = oracle.marching_cubes(c.grid, c.iso, c.pad)
    assert len(v) == len(cut.keys)                                              # vertex n is edge n
    ratio = IC.check_positions(cut, v)
    mv, ma = IC.model_vertices(c.grid, cut, c.iso, c.pad, c.n_attr)
    assert np.array_equal(mv.view(np.uint32), v.view(np.uint32))                # the float32 model IS the restatement's formula
    aratio = IC.check_attributes(c.grid, cut, ma, c.n_attr) if c.n_attr else 0.0
    print(f"{name}: {len(v)} vertices, {len(t)} triangles; position {ratio:.3f} of its bound, attributes (model) {aratio:.3f}")
    assert len(t) == 0 or (t.min() >= 0 and t.max() < len(v))
    if c.small:
        stats = _independent().check_mesh(_value(c), v, t, float(np.float32(c.iso)), c.pad, keys=IC.key_list(cut))
        assert stats["triangles"] == len(t)


def test_the_cases_are_what_they_are_for(oracle):
    count = {c.name: (len(IC.cut_of(c).keys), len(oracle.marching_cubes(c.grid, c.iso, c.pad)[1])) for c in IC.cases()}
    assert count["border_sphere_pad"][0] == 728 and count["border_sphere_open"][0] == 544
    sphere = IC.case("border_sphere_pad")
    cut = IC.cut_of(sphere)
    border = ~(cut.a_in & cut.b_in)
    faces = {(int(a), int(k[1 + a] == 0)) for k, a in zip(cut.keys[border], cut.axis[border])}
    assert len(faces) == 6 and border.sum() == 184                              # the sphere leaves through all six faces
    assert ((~cut.a_in) & border).any() and ((~cut.b_in) & border).any()        # both directions of the fallback
    assert int((IC.ties_half_grid() == 0).sum()) == 114 and int((IC.ties_one_grid() == 0).sum()) > 100
    v, t = oracle.marching_cubes(IC.t_to_one_grid(), 0.0, 1.0)
    assert len(v) == 24 and len(np.unique(v, axis=0)) == 8                      # vertices rounded onto lattice points ...
    p = v.astype(np.float64)[t]
    assert (np.linalg.norm(np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]), axis=1) == 0).any()         # ... and zero-area faces
    assert count["thin_open"][0] > 0 and count["thin_open"][1] == 0             # vertices and no triangle
    assert count["one_voxel"] == (6, 8)
    assert all(not (cu.a_in & cu.b_in).any() for cu in [IC.cut_of(IC.case("full"))])                     # only border edges
    cut = IC.cut_of(IC.case("long"))
    assert cut.pos.max() > 256 and (3 * 302 * 7 * 6) % 256 != 0 and len(cut.keys) > 256
    assert float(np.float32(0.3)) != 0.3                                             # a level that float32 does not hold


@pytest.mark.parametrize("name", ["ties_half_pad", "t_to_one"])
def test_position_keys_are_blind_where_order_keys_are_not(oracle, name):
    """what check_mesh(keys=...) is for: read off the positions, two vertices land on one grid edge"""
    c = IC.case(name)
    v, t = oracle.marching_cubes(c.grid, c.iso, c.pad)
    with pytest.raises(AssertionError, match="two mesh vertices on one grid edge"):
        _independent().check_mesh(_value(c), v, t, c.iso, c.pad)
    _independent().check_mesh(_value(c), v, t, c.iso, c.pad, keys=IC.key_list(IC.cut_of(c)))


# ------------------------------------------------------------------ the checks can fail
def _model(name, **kw):
    c = IC.case(name)
    cut = IC.cut_of(c)
    v, a = IC.model_vertices(c.grid, cut, c.iso, c.pad, c.n_attr, **kw)
    return c, cut, v, a


def _inner_vertex(c, cut):
    """an interior edge whose two ends differ in every channel and whose mu is away from 1/2"""
    Aa, Ab = IC._ends(c.grid, cut, c.n_attr)
    ok = cut.a_in & cut.b_in & (np.abs(cut.mu - 0.5) > 0.2) & (np.abs(Aa - Ab) > 0.2 * np.maximum(np.abs(Aa), np.abs(Ab))).all(1)
    return int(np.flatnonzero(ok)[0]), Aa, Ab


def test_fault_attribute_ends_swapped():
    c, cut, v, a = _model("border_sphere_pad")
    n, Aa, Ab = _inner_vertex(c, cut)
    t = np.float32(cut.mu[n])
    a[n] = Ab[n] + t * (Aa[n] - Ab[n])
    with pytest.raises(AssertionError, match=rf"vertex {n} on edge .* of the bound"):
        IC.check_attributes(c.grid, cut, a, c.n_attr)


def test_fault_border_vertex_takes_the_mean_of_both_ends():
    """the end in the border read from the clamped voxel next to the inside end instead: not the inside end's bits"""
    c, cut, v, a = _model("border_sphere_pad")
    n = int(np.flatnonzero(~cut.b_in)[0])                                       # the upper end lies in the border
    inside = cut.a[n]
    other = inside.copy()
    other[cut.axis[n]] -= 1                                                     # what a wrapped or clamped read would fetch
    a[n] = (c.grid[tuple(inside)][1:4] + c.grid[tuple(other)][1:4]) * np.float32(0.5)
    with pytest.raises(AssertionError, match="border vertices do not carry the inside end's attributes bit for bit"):
        IC.check_attributes(c.grid, cut, a, c.n_attr)


@pytest.mark.parametrize("name", ["pbr_stride_3", "border_sphere_pad"])
def test_fault_attribute_channel_off_by_one(name):
    c = IC.case(name)
    cut = IC.cut_of(c)
    shifted = np.concatenate([c.grid[..., :1], c.grid[..., 2:], c.grid[..., 1:2]], -1)      # channel k + 1 where channel k belongs
    _, a = IC.model_vertices(shifted, cut, c.iso, c.pad, c.n_attr)
    with pytest.raises(AssertionError):
        IC.check_attributes(c.grid, cut, a, c.n_attr)
    one = IC.model_vertices(c.grid, cut, c.iso, c.pad, c.n_attr)[1]
    one[:, 0] = a[:, 0]                                                         # ... in a single channel
    with pytest.raises(AssertionError):
        IC.check_attributes(c.grid, cut, one, c.n_attr)


@pytest.mark.parametrize("name", ["long", "level_noise", "ties_one"])
def test_fault_vertex_moved_by_four_ulp(name):
    c, cut, v, _ = _model(name)
    n = int(np.argmax(np.where(np.arange(3)[None] == cut.axis[:, None], cut.pos, -np.inf).max(1)))       # the largest interpolated coordinate
    k = int(cut.axis[n])
    assert cut.pos[n, k] >= 2.0                     # 4 ulp of a coordinate in [2, 4) are 16 u, its bound at most 8 u (and so on upwards)
    x = v[n, k]
    for _ in range(4):
        x = np.nextafter(x, np.float32(np.inf) if v[n, k] >= cut.pos[n, k] else np.float32(-np.inf))
    v[n, k] = x
    with pytest.raises(AssertionError, match=rf"vertex {n} on edge"):
        IC.check_positions(cut, v)


def test_fault_level_used_as_a_double():
    c = IC.case("level_sphere")
    cut = IC.cut_of(c)
    v, _ = IC.model_vertices(c.grid, cut, 0.3, c.pad, iso_double=True)
    with pytest.raises(AssertionError, match="of the bound"):
        IC.check_positions(cut, v)


# ------------------------------------------------------------------ components: the restatement against plain label propagation
def _np_labels(t, nv):
    lab = np.arange(nv)
    t = np.asarray(t, np.int64).reshape(-1, 3)
    while len(t):
        new = lab.copy()
        m = np.minimum(np.minimum(lab[t[:, 0]], lab[t[:, 1]]), lab[t[:, 2]])
        for k in range(3):
            np.minimum.at(new, t[:, k], m)
        new = new[new]
        if np.array_equal(new, lab):
            break
        lab = new
    return lab


def test_restatement_components_on_the_hard_meshes(oracle):
    for name in ("pbr_stride_3", "ties_one", "level_noise"):
        c = IC.case(name)
        v, t = oracle.marching_cubes(c.grid, c.iso, c.pad)
        lab = oracle.mesh_components(t, len(v))
        assert np.array_equal(lab, _np_labels(t, len(v)))
        assert len(np.unique(lab)) > 3                                          # many small components next to a large one
    t, nv = IC.strip_permuted(200)
    assert np.array_equal(oracle.mesh_components(t, nv), np.zeros(nv, np.int32))
    assert np.array_equal(oracle.mesh_components(np.zeros((0, 3), np.int32), 5), np.arange(5))
