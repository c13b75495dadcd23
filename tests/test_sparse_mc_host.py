"""CPU-only: the NumPy restatement of the narrow-band extraction rule (tests/sparse_mc_cases.py) against the dense
definition — the C restatement of marching cubes, the table-free edge keys of isosurface_cases.py and the C connected components —
for both guarantees: (a) every brick active gives the dense mesh, (b) a closed growth gives whole components, those of the seed
bricks.  Then the proof that the checkers can fail: five faults a device implementation could have, each caught.  The device runs
the same checkers in tests/test_sparse_mc_gpu.py."""
import numpy as np
import pytest

import isosurface_cases as IC
import sparse_mc_cases as SC

_dense = {}


def dense_of(oracle, c):
    if c.name not in _dense:
        v, t = oracle.marching_cubes(c.grid, c.iso, c.pad)
        attrs = None
        if c.n_attr:
            cut = IC.expected_cut_edges(SC.value_of(c), c.iso, c.pad)
            mv, attrs = IC.model_vertices(c.grid, cut, c.iso, c.pad, c.n_attr)
            assert np.array_equal(mv.view(np.uint32), v.view(np.uint32))
        _dense[c.name] = SC.dense_mesh(c, v, t, attrs, oracle.mesh_components)
    return _dense[c.name]


@pytest.mark.parametrize("name,B", SC.case_blocks())
def test_all_active_is_the_dense_mesh(oracle, name, B):
    c = SC.case(name)
    d = dense_of(oracle, c)
    r = SC.rule(SC.value_of(c), c.iso, c.pad, B, all_active=True)
    assert r.ext.all() and r.closed and r.rounds == 0
    assert r.n_samples == int(np.prod(r.nb)) * B ** 3
    SC.check_all_active(d, SC.select_cells(d, r.ext))


@pytest.mark.parametrize("name,B", SC.case_blocks())
def test_grown_band_is_the_components_of_the_seed_bricks(oracle, name, B):
    c = SC.case(name)
    d = dense_of(oracle, c)
    r = SC.rule(SC.value_of(c), c.iso, c.pad, B)
    got = SC.select_cells(d, r.ext)
    SC.check_closed_result(d, r, got)
    SC.check_seed_components(d, r, got)
    print(f"{name} B={B}: {int(r.seed.sum())} seeds, {int(r.active.sum())} of {r.active.size} bricks after {r.rounds} rounds, "
          f"{len(got[1])} of {len(d.tris)} triangles")
    assert r.rounds <= 3
    # whenever the largest component touches a seed brick, largest_component sees no difference
    lv, lt = SC.largest_component_np(d.verts, d.tris, d.labels)
    if len(d.tris) and r.ext0[tuple(d.tri_cell[d.labels[d.tris[:, 0]] == np.bincount(d.labels[d.tris[:, 0]]).argmax()].T)].any():
        gv, gt = SC.largest_component_np(got[0], got[1], components=oracle.mesh_components)
        assert np.array_equal(gv.view(np.uint32), lv.view(np.uint32)) and np.array_equal(gt, lt)
    elif (name, B) not in SC.NO_SEEDS:
        pytest.fail(f"{name} B={B}: the largest component meets no seed brick; the case shows nothing")
    assert r.seed.any() == ((name, B) not in SC.NO_SEEDS)


def test_the_cases_are_what_they_are_for(oracle):
    # the pole is invisible to the lattice and followed by the growth; the speck is invisible and left out
    c = SC.case("pole_speck")
    d = dense_of(oracle, c)
    val = SC.value_of(c)
    for B in c.blocks:
        axes, _ = SC.lattice_axes(val.shape, B)
        seen = [set(np.clip(np.floor(a), 0, n - 1).astype(int)) for a, n in zip(axes, val.shape)]
        assert SC.SPECK[0] not in seen[0] and 31 not in seen[0]                                   # neither on a lattice line
        r = SC.rule(val, c.iso, c.pad, B)
        assert r.rounds >= 1
        grown = SC.select_cells(d, r.ext)
        seeds_only = SC.select_cells(d, r.ext0)
        assert len(seeds_only[1]) < len(grown[1])                                                   # growth added triangles
        top = grown[0][:, 2].max()
        assert top > 25.0 and np.abs(grown[0][grown[0][:, 2] > 22.0][:, :2] - [31, 18]).max() <= 1.0   # the pole's top is there
        assert not (np.abs(grown[0] - np.asarray(SC.SPECK)).max(1) <= 1.0).any()                    # the speck is not
        assert (np.abs(d.verts - np.asarray(SC.SPECK)).max(1) <= 1.0).sum() == 6                    # ... though the dense mesh has it
        assert len(np.unique(d.labels)) == 2
    # all negative: the only surface is the pad shell, only border bricks seed
    c = SC.case("all_negative")
    r = SC.rule(SC.value_of(c), c.iso, c.pad, 4)
    inner = r.seed[1:-1, 1:-1, 1:-1]
    assert r.seed.any() and not inner.any() and r.seed[0].all() and r.seed[:, :, -1].all()
    assert len(dense_of(oracle, c).tris) > 0
    # empty: nothing
    c = SC.case("empty")
    r = SC.rule(SC.value_of(c), c.iso, c.pad, 4)
    assert not r.seed.any() and len(dense_of(oracle, c).tris) == 0 and r.n_samples == int(np.prod([n + 1 for n in r.nb]))
    # thinner than a brick, partial last bricks, a brick size on which P is a multiple
    assert SC.rule(SC.value_of(SC.case("all_negative_thin")), 0.0, 1.0, 8).nb == (1, 6, 1)
    assert any((d + 2) % B for cc in SC.cases() for B in cc.blocks for d in SC.value_of(cc).shape)
    assert any((d + 2) % B == 0 for cc in SC.cases() for B in cc.blocks for d in SC.value_of(cc).shape)
    assert {B for cc in SC.cases() for B in cc.blocks} == {4, 8, 16}
    dims = {SC.value_of(cc).shape for cc in SC.cases()}
    assert {(40, 36, 28), (37, 33, 29), (5, 40, 3), (21, 19, 18)} <= dims
    # the band is a small part of the grid already at these sizes
    c = SC.case("torus_40")
    r = SC.rule(SC.value_of(c), c.iso, c.pad, 4)
    assert r.active.sum() < 0.5 * r.active.size


def test_dilation_and_round_limit(oracle):
    c = SC.case("pole_speck")
    d = dense_of(oracle, c)
    val = SC.value_of(c)
    r0, r1 = SC.rule(val, c.iso, c.pad, 8), SC.rule(val, c.iso, c.pad, 8, dilate=1)
    assert r1.active.sum() > r0.active.sum() and r1.closed and (r1.active >= r0.seed).all()
    SC.check_closed_result(d, r1, SC.select_cells(d, r1.ext))
    cut = SC.rule(val, c.iso, c.pad, 8, max_rounds=0)
    assert not cut.closed and cut.rounds == 0 and (cut.active == cut.seed).all()


def test_mesh_sparse_switch(monkeypatch):
    from sin3dm_amd import sample
    monkeypatch.delenv("S3D_MESH_SPARSE", raising=False)
    assert sample.mesh_sparse() == 0 and sample.mesh_sparse("16") == 16
    monkeypatch.setenv("S3D_MESH_SPARSE", "8")
    assert sample.mesh_sparse() == 8
    for bad in ("5", "eight", "-4"):
        with pytest.raises(ValueError):
            sample.mesh_sparse(bad)


def test_host_fused_multiply_add_is_exact():
    """the decoder adapter's point tables: q * b + c with one rounding.  Against float64 where the sum is exact there, against the
    two-rounding float32 result where the two are known to differ, and on a tie between two float32 neighbours."""
    from sin3dm_amd.encoding.model import _fma_f32
    q = ((np.float32(0.5) + np.arange(40, dtype=np.float32)) / np.float32(40)).astype(np.float32)
    b, c = np.float32(0.8) - np.float32(-0.8), np.float32(-0.8)
    got = _fma_f32(q, b, c)
    assert got.dtype == np.float32
    exact = q.astype(np.float64) * np.float64(b) + np.float64(c)                 # 24 x 24 bits and a float32: exact in float64 here
    assert np.array_equal(got, exact.astype(np.float32))
    plain = ((q * b).astype(np.float32) + c).astype(np.float32)
    assert (got != plain).sum() >= 10 and got[16] != plain[16] and np.abs(got.astype(np.float64) - plain).max() < 1e-7
    one, ulp = np.float32(1.0), np.float32(2.0 ** -23)
    tie = _fma_f32(np.asarray([one + ulp], np.float32), 0.5, 0.0)[0]             # (1 + u) / 2: halfway between 0.5 and 0.5 + u / 2 ... exact
    assert tie == np.float32(0.5) + np.float32(2.0 ** -24)
    half_ulp = _fma_f32(np.asarray([ulp], np.float32), 0.5, 1.0)[0]              # 1 + u / 2: a tie, to even = 1
    assert half_ulp == one and _fma_f32(np.asarray([3 * ulp], np.float32), 0.5, 1.0)[0] == one + 2 * ulp


# ------------------------------------------------------------------ the checkers can fail
def test_fault_growth_switched_off(oracle):
    c = SC.case("pole_speck")
    d = dense_of(oracle, c)
    val = SC.value_of(c)
    good, bad = SC.rule(val, c.iso, c.pad, 8), SC.rule(val, c.iso, c.pad, 8, fault="no_growth")
    got = SC.select_cells(d, bad.ext)
    with pytest.raises(AssertionError, match="components of the seed bricks"):
        SC.check_seed_components(d, good, got)
    with pytest.raises(AssertionError):
        SC.check_closed_result(d, bad, got)                     # even on its own terms: a component is only partly there


def test_fault_pad_vertices_unknown(oracle):
    c = SC.case("all_negative")
    d = dense_of(oracle, c)
    bad = SC.rule(SC.value_of(c), c.iso, c.pad, 4, all_active=True, fault="pad_unknown")
    with pytest.raises(AssertionError, match="all bricks active"):
        SC.check_all_active(d, SC.select_cells(d, bad.ext))


def test_fault_lattice_outside_the_box_not_padded(oracle):
    c = SC.case("all_negative")
    d = dense_of(oracle, c)
    val = SC.value_of(c)
    good, bad = SC.rule(val, c.iso, c.pad, 4), SC.rule(val, c.iso, c.pad, 4, fault="lattice_unpadded")
    assert not bad.seed.any()
    with pytest.raises(AssertionError, match="components of the seed bricks"):
        SC.check_seed_components(d, good, SC.select_cells(d, bad.ext))


def test_fault_brick_major_order(oracle):
    c = SC.case("torus_40")
    d = dense_of(oracle, c)
    brick = d.tri_cell // 8
    order = np.lexsort((np.arange(len(d.tris)), brick[:, 2], brick[:, 1], brick[:, 0]))
    assert not np.array_equal(order, np.arange(len(order)))
    with pytest.raises(AssertionError, match="triangles differ"):
        SC.check_all_active(d, (d.verts, d.tris[order], d.attrs))
    vb = d.keys[:, 1:] // 8
    vorder = np.lexsort((np.arange(len(d.verts)), vb[:, 2], vb[:, 1], vb[:, 0]))
    inv = np.empty_like(vorder)
    inv[vorder] = np.arange(len(vorder))
    with pytest.raises(AssertionError, match="differ"):
        SC.check_all_active(d, (d.verts[vorder], inv[d.tris].astype(np.int32), d.attrs))


def test_fault_partial_last_brick_read_past_the_grid(oracle):
    """the last brick of an axis holds vertices beyond P; an implementation that reads them (here: as the row-major neighbours a
    flat index reaches) extracts cells that do not exist"""
    c = SC.case("border_sphere")
    d = dense_of(oracle, c)
    val = SC.value_of(c)
    B = 4
    pv = np.pad(val, 1, mode="constant", constant_values=np.float32(c.pad))
    ext = [(-p) % B for p in pv.shape]
    assert any(ext)
    wrapped = np.pad(pv, [(0, e) for e in ext], mode="wrap")
    v, t = oracle.marching_cubes(wrapped, c.iso, None)
    with pytest.raises(AssertionError, match="all bricks active"):
        SC.check_all_active(d, (v - np.float32(1.0), t, None))
