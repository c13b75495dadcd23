"""GPU tests of the mesh preprocessing (MeshSampler -> s3d_meshsdf.hip) on the inputs the torus of test_meshprep_gpu.py does not
have: needle and cap slivers, faces without area, triangle soups, duplicated faces, a band thinner than the cell, thousands of
faces in one cell, a mesh without extent along an axis, and face / point counts around the winding-number kernel's tile and block
(tests/meshprep_cases.py builds the sets and their float64 oracles).

The sets with well-defined planes are held to the project's tolerances against the float64 distance itself (TOL_DIST = 1.04e-6,
TOL_WN = 6.72e-6: 8 x the float32 restatement's gap on the torus; test_meshprep_hard_host.py shows that the restatement uses at
most a quarter of them on these sets).  The soups are held to the sandwich

    min(min_f tri_distance64, band) - TOL_DIST  <=  dist  <=  min(min_f boundary_distance64, band) + TOL_DIST

whose two bounds are float64 oracle values that coincide on faces without area and differ by at most a sliver's height."""
import numpy as np
import pytest

import meshprep_cases as M
from meshprep_cases import TOL_DIST, TOL_WN, hard

pytestmark = pytest.mark.gpu


def check_winding(hs, max_excluded):
    wn_or = hs.wn()
    sure = np.abs(np.abs(wn_or) - 0.5) > 10 * TOL_WN
    assert 1 - sure.mean() <= max_excluded, (hs.name, 1 - sure.mean())          # the oracle alone: the mask is decided (almost) everywhere
    wn = hs.sampler().winding_number(hs.wn_points).cpu().numpy()
    err = np.abs(wn - wn_or).max()
    print(f"{hs.name}: {len(hs.F)} faces, {len(wn)} points, winding number error max {err:.3e} (tol {TOL_WN:.3e}), range [{wn_or.min():.3f}, {wn_or.max():.3f}]")
    assert wn.shape == wn_or.shape and err <= TOL_WN
    assert np.array_equal((np.abs(wn) >= 0.5)[sure], (np.abs(wn_or) >= 0.5)[sure])
    return wn


# ------------------------------------------------------------------ soups: the sandwich
@pytest.mark.parametrize("band", M.SOUP_BANDS)
@pytest.mark.parametrize("name", M.SOUPS)
def test_soup_distance_in_the_sandwich(name, band):
    """600 isolated cap triangles (apex eps L over the long edge; eps = 0: collinear) or 620 needles and point faces; 4000 queries
    0.003 to 0.2 from a face.  Measured on the MI355X (profiles/meshprep_hard.txt): outside the sandwich by at most 8.0e-8 on
    every set; with Ericson's region test alone, up to 0.106 (caps) and 0.178 (needles) above it and 1.3e-2 below it."""
    hs = hard(name)
    M.check_sandwich(hs.sampler(), hs, band)


# ------------------------------------------------------------------ sets held to the float64 distance itself
@pytest.mark.parametrize("eps", M.SLIVER_EPS)
def test_sliver_torus(eps):
    """The closed torus with an in-plane sliver on every face: distance (bands 0.25 and 0.05), winding number and its mask."""
    hs = hard(f"sliver_torus[{eps:g}]")
    ms = hs.sampler()
    for band in (M.case().band, 0.05):
        _, face, _ = M.check_closest(ms, hs.T, hs.queries, hs.lo(), band)
        assert (face >= 0).sum() > 150
    wn = check_winding(hs, 0.0)
    assert 0 < (np.abs(wn) >= 0.5).sum() < len(wn)


@pytest.mark.parametrize("eps", M.SLIVER_EPS)
def test_sliver_torus_surface_samples(eps):
    """20 000 samples lie on their faces; the share on the 576 slivers is their float64 area share within 5 sigma."""
    import torch
    hs = hard(f"sliver_torus[{eps:g}]")
    n = 20000
    g = torch.Generator(device="cuda")
    g.manual_seed(4321)
    pts, face, bary = (t.cpu().numpy() for t in hs.sampler().sample_surf(n, g))
    assert pts.shape == (n, 3) and face.min() >= 0 and face.max() < len(hs.F) and (bary >= 0).all()
    d = M.tri_distance64(pts.astype(np.float64), hs.T[face])
    area = 0.5 * np.sqrt(hs.area2())
    p = area[:hs.n_sliver].sum() / area.sum()
    got, sigma = (face < hs.n_sliver).mean(), np.sqrt(p * (1 - p) / n)
    print(f"{hs.name}: samples off their face by {d.max():.3e}; share on the slivers {got:.3e}, area share {p:.3e}, sigma {sigma:.3e}")
    assert d.max() <= TOL_DIST
    assert abs(got - p) <= 5 * sigma


def test_duplicated_faces():
    """Every face twice, the copy at f + F: the same distance, the lower index reported (the tie rule of k_mesh_closest), twice
    the winding number."""
    hs = hard("duplicated")
    ms = hs.sampler()
    for band in (M.case().band, 0.05):
        _, face, _ = M.check_closest(ms, hs.T, hs.queries, hs.lo(), band)
        assert (face >= 0).sum() > 150 and (face[face >= 0] < hs.n_unique).all()
    wn = check_winding(hs, 0.0)
    assert np.abs(hs.wn()).max() > 1.99 and (np.abs(wn) >= 0.5).sum() == (np.abs(wn) >= 1.5).sum() > 0


def test_band_thinner_than_the_cell():
    """Band 0.004 on the torus: cell = extent / 256 = 0.0076 > band, 252 x 140 x 256 cells."""
    hs = hard("thin_band")
    ms = hs.sampler()
    _, cell, dims = ms._binned(hs.band)[:3]
    print(f"thin_band: cell {cell:.5f} > band {hs.band} on {list(dims)} cells")
    assert cell > hs.band and max(dims) == 256
    _, face, _ = M.check_closest(ms, hs.T, hs.queries, hs.lo(), hs.band)
    assert (face >= 0).sum() > 1000 and (face < 0).sum() > 100


def test_thousands_of_faces_in_one_cell():
    """A 2208-face sphere of radius 0.02 inside one cell of the band-0.25 grid and one triangle listed in every cell."""
    hs = hard("dense_cell")
    ms = hs.sampler()
    _, face, _ = M.check_closest(ms, hs.T, hs.queries, hs.lo(), 0.25)
    n_pairs, seg = ms._binned(0.25)[5], ms._binned(0.25)[3].cpu().numpy()
    print(f"dense_cell: {n_pairs} pairs, longest segment {np.diff(seg).max()}, shortest {np.diff(seg).min()}")
    assert np.diff(seg).max() >= 2209 and np.diff(seg).min() >= 1
    assert (face == 2208).sum() > 100 and ((face >= 0) & (face < 2208)).sum() > 1000


def test_flat_mesh():
    """One planar quad, y = fl32(0.1) on every vertex.  A point sees it under less than the cone 2 pi (1 - h / sqrt(h^2 + R^2)), h its
    height over the plane and R = 3.03 the reach of the quad from any foot point, so |wn| >= 0.5 - TOL_WN needs h <= 2 TOL_WN R / sqrt(1 - 4 TOL_WN^2)."""
    hs = hard("flat")
    ms = hs.sampler()
    for band in M.FLAT_BANDS:
        _, face, _ = M.check_closest(ms, hs.T, hs.queries, hs.lo(), band)
        assert (face >= 0).sum() > 3
    wn = check_winding(hs, 0.01)
    height = np.abs(hs.wn_points[:, 1].astype(np.float64) - M.FLAT_Y)
    assert (height[np.abs(wn) >= 0.5] <= 2 * TOL_WN * M.FLAT_REACH / np.sqrt(1 - 4 * TOL_WN ** 2)).all()


@pytest.mark.parametrize("n_points", M.TILE_POINTS)
@pytest.mark.parametrize("n_faces", M.TILE_FACES)
def test_winding_number_at_the_tile_edges(n_faces, n_points):
    """Face counts around the 256-triangle LDS tile, point counts around the 512 points of a block."""
    check_winding(hard(f"tile_edges[{n_faces},{n_points}]"), 0.01)
