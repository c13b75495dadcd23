"""CPU-only: the oracles and the float32 restatements of the hard mesh-preprocessing sets (tests/meshprep_cases.py: slivers, soups,
duplicated faces, a thin band, a dense cell, a flat mesh, tile edges), before any device sees them:

  * the two float64 definitions of the distance agree where both are defined;
  * the kernel's formulation, restated in float32 (`closest32`), stays inside the sandwich on every soup, and the formulation it
    replaced (`ericson32_plain`) does not: the check sees the defect it was written for;
  * on the sets held to the tight tolerance the float32 restatement leaves the device a factor of four;
  * the inside / outside mask of the winding-number sets is decided by the oracle alone.

`python tests/meshprep_cases.py` prints all the figures."""
import numpy as np
import pytest

import meshprep_cases as M
from meshprep_cases import TOL_DIST, TOL_WN, hard

ZERO_AREA = ("cap_soup[1e-06]", "cap_soup[1e-07]", "cap_soup[0]", "needle_soup")      # sets with a face of no area after rounding to fp32


def _restated(name, fn):
    hs = hard(name)
    return hs.memo(fn.__name__, lambda: M.brute_min(fn, hs.queries.astype(np.float64), hs.T)[0])


@pytest.mark.parametrize("name", M.SOUPS + M.TIGHT)
def test_the_two_float64_oracles_agree(name):
    """tri_distance64 (segments + plane, the normal in rational arithmetic) against pair_closest (Ericson in float64), per query
    as the minimum over the faces, to 1e-12, on every set whose faces all have an area; the boundary is never nearer than the
    triangle.  (Face by face, float64 Ericson itself is off by up to 4.2e-12 on faces of sliver_torus[1e-06] that are not the
    nearest: its barycentrics divide by a sum of differences of products that keeps 1e-10 of its value.)"""
    hs = hard(name)
    lo, hi = hs.lo(), hs.hi()
    assert (hi >= lo).all() and np.isfinite(hi).all()
    assert ((hs.area2() == 0).any()) == (name in ZERO_AREA)
    if name in ZERO_AREA:
        return
    d64, _ = M.brute_closest(hs.queries.astype(np.float64), hs.T)
    print(f"{name}: tri_distance64 vs pair_closest {np.abs(lo - d64).max():.3e}")
    assert np.abs(lo - d64).max() <= 1e-12


def test_segment_and_plane_distance_on_faces_without_area():
    """tri_distance64 by hand on a collinear face, a face with two equal vertices and a point face."""
    T = np.array([[0, 0, 0, 2, 0, 0, 1, 0, 0],            # collinear: the segment x in [0, 2]
                  [0, 0, 0, 0, 0, 0, 0, 3, 0],            # a = b: the segment y in [0, 3]
                  [1, 1, 1, 1, 1, 1, 1, 1, 1],            # a point
                  [0, 0, 0, 2, 0, 0, 0, 2, 0]], dtype=np.float64)        # a right triangle in z = 0
    P = np.array([[1, 1, 0], [3, 0, 4], [0.5, 0.5, 2]], dtype=np.float64)
    want = np.array([[1, 1, 1, 0],                                                    # (1, 1, 0) lies on the hypotenuse
                     [np.sqrt(17), 5, np.sqrt(14), np.sqrt(17)],                      # beyond b = (2, 0, 0)
                     [np.sqrt(4.25), np.sqrt(4.25), np.sqrt(1.5), 2]])                # above the interior: the plane is nearer
    got = M.tri_distance64(P[:, None, :], T[None])
    assert np.abs(got - want).max() <= 2e-15, got
    edges = M.boundary_distance64(P[:, None, :], T[None])
    assert np.array_equal(edges[:, :3], got[:, :3]) and np.array_equal(edges[:2, 3], got[:2, 3]) and abs(edges[2, 3] - np.sqrt(4.25)) <= 2e-15


@pytest.mark.parametrize("name", M.SOUPS)
def test_closest32_stays_in_the_sandwich(name):
    hs = hard(name)
    lo, hi, d = hs.lo(), hs.hi(), _restated(name, M.closest32)
    print(f"{name}: closest32 below lo by {np.max(lo - d):.3e}, above hi by {np.max(d - hi):.3e}, |d - lo| {np.abs(d - lo).max():.3e}, "
          f"hi - lo {np.max(hi - lo):.3e}")
    assert np.isfinite(d).all()
    assert np.max(lo - d) <= TOL_DIST and np.max(d - hi) <= TOL_DIST


@pytest.mark.parametrize("name", ["cap_soup[1e-05]", "cap_soup[0]", "needle_soup"])
def test_plain_ericson_in_float32_leaves_the_sandwich(name):
    """The formulation the kernel had: the wrong Voronoi region (or 0 / 0) on faces whose plane fp32 does not resolve.  Always on
    the far side."""
    hs = hard(name)
    lo, hi, d = hs.lo(), hs.hi(), _restated(name, M.ericson32_plain)
    print(f"{name}: ericson32_plain above hi by {np.max(d - hi):.3e} ({int((d - hi > TOL_DIST).sum())} queries over {TOL_DIST:.2e}), below lo by {np.max(lo - d):.3e}")
    assert (d - hi > 1e-4).sum() >= 1
    assert np.max(lo - d) <= TOL_DIST


@pytest.mark.parametrize("name", M.TIGHT)
def test_headroom_on_the_tight_sets(name):
    """The float32 restatement's gap to float64 is at most a quarter of the device tolerances."""
    hs = hard(name)
    gap = np.abs(_restated(name, M.closest32) - hs.lo()).max()
    print(f"{name}: closest32 vs float64 {gap:.3e} (TOL_DIST / 4 = {TOL_DIST / 4:.3e})")
    assert gap <= TOL_DIST / 4
    if hs.wn_points is not None:
        gap = np.abs(M.brute_winding(hs.wn_points.astype(np.float64), hs.T, np.float32) - hs.wn()).max()
        print(f"{name}: winding number fp32 vs float64 {gap:.3e} (TOL_WN / 4 = {TOL_WN / 4:.3e})")
        assert gap <= TOL_WN / 4


def test_headroom_on_the_tile_edges():
    for name in M.TILE_EDGES:
        hs = hard(name)
        assert np.abs(M.brute_winding(hs.wn_points.astype(np.float64), hs.T, np.float32) - hs.wn()).max() <= TOL_WN / 4, name


def test_the_sign_mask_is_decided_by_the_oracle():
    for name, most in [(n, 0.0) for n in M.SLIVER_TORI + ("duplicated",)] + [(n, 0.01) for n in M.TILE_EDGES + ("flat",)]:
        assert M.undecided(hard(name).wn()) <= most, name
    dup, c = hard("duplicated"), M.case()
    single = M.brute_winding(dup.wn_points.astype(np.float64), c.T)
    assert np.abs(dup.wn() - 2 * single).max() <= 1e-12 and (np.abs(np.abs(single) - 0.5) > 0.49).all()
    flat = hard("flat")
    height = np.abs(flat.wn_points[:, 1].astype(np.float64) - M.FLAT_Y)
    assert (np.abs(flat.wn()) <= 0.5 * (1 - height / np.hypot(height, M.FLAT_REACH)) + 1e-12).all()       # the cone that holds the quad


def test_the_sets_are_what_they_say():
    for e in M.CAP_EPS:
        hs = hard(f"cap_soup[{e:g}]")
        assert len(hs.F) == 600 and len(hs.queries) == 4000
    assert (hard("cap_soup[0]").area2()[:100] == 0).all() and (hard("cap_soup[0.01]").area2() > 0).all()
    nd = hard("needle_soup")
    assert len(nd.F) == 620 and (nd.T[600:, 0:3] == nd.T[600:, 3:6]).all() and (nd.T[600:, 0:3] == nd.T[600:, 6:9]).all()
    for e in M.SLIVER_EPS:
        hs = hard(f"sliver_torus[{e:g}]")
        assert len(hs.F) == 1728 and hs.n_sliver == 576
        edges = np.concatenate([hs.F[:, [0, 1]], hs.F[:, [1, 2]], hs.F[:, [2, 0]]])
        assert len({(a, b) for a, b in edges}) == len(edges) and {(b, a) for a, b in edges} == {(a, b) for a, b in edges}      # closed, oriented
    from sin3dm_amd.data.mesh_sampler import cell_grid
    tb = hard("thin_band")
    _, cell, dims = cell_grid(tb.V32.astype(np.float64).min(0), tb.V32.astype(np.float64).max(0), M.THIN_BAND)
    inside = tb.lo() < M.THIN_BAND
    print(f"thin_band: cell {cell:.5f} on {dims}; {int(inside.sum())} of {len(inside)} queries inside the band, nearest to it "
          f"{np.abs(tb.lo() - float(np.float32(M.THIN_BAND))).min():.3e}")
    assert cell > M.THIN_BAND and 1000 < inside.sum() < 2900
    assert np.abs(tb.lo() - float(np.float32(M.THIN_BAND))).min() > TOL_DIST
    dc = hard("dense_cell")
    assert len(dc.F) == 2209
    tri = dc.T[:2208].reshape(-1, 3, 3)
    edge = np.linalg.norm(tri - tri[:, [1, 2, 0]], axis=2)                        # ring edges 0.0026, a band's diagonal 0.0037
    assert 0.0003 < edge.min() and edge.max() < 0.0038 and (np.linalg.norm(tri - [0.31, -0.12, 0.27], axis=2) < 0.0201).all()
    fl = hard("flat")
    assert (fl.V32[:, 1] == np.float32(0.1)).all()
    reach = np.linalg.norm(fl.wn_points[:, None, [0, 2]].astype(np.float64) - fl.V32[None, :, [0, 2]], axis=2).max()
    assert reach <= M.FLAT_REACH
