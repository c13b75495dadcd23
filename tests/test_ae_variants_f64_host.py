"""The CPU half of tests/test_hip_ae_variants_f64.py (cases, batches, metrics and bounds in tests/ae_f64_cases.py): every batch
draw converges and clears the kinks, the texture bands hold the rows they are said to hold, every bound follows the rule from
the float32 gap written beside it, the float32 restatement stays inside every bound — and injected faults, run in float32
through the same restatement, leave them: the ones tests/ae_pbr_cases.py and tests/ae_variants_cases.py already carry, and five
that only show at small planes, single-row bands, single points, off-centre boxes and rows on the band's edge."""
import numpy as np
import pytest

import ae_f64_cases as A
import ae_pbr_cases as P

CASES = list(A.CASES)


@pytest.fixture(scope="module", autouse=True)
def _threads():
    import torch
    n = torch.get_num_threads()
    torch.set_num_threads(min(16, n))
    yield
    torch.set_num_threads(n)


def test_the_grid_is_the_one_asked_for():
    assert len(A.SHAPES) == 17 and len(A.MODES) == 18 and len(A.BAND) == 4 and set(A.BOUNDS) == set(A.CASES)
    assert sorted(c["tc"] for c in A.SHAPES.values() if c["net"] == "skip") == [1, 2, 5, 8, 8, 8, 8]
    assert {(c["net"], c["enc"]) for c in A.MODES.values()} == {("geo", "skip"), ("geo", "pbr"), ("skip", "skip"), ("pbr", "pbr")}
    for c in A.CASES.values():                                   # what the constructors take
        geo, tex, up, hid, layers = c["cfg"]
        assert up % 32 == 0 and hid % 32 == 0 and layers == 4 and geo % 4 == 0 and tex % 4 == 0 and geo + tex <= 12
        assert c["net"] != "pbr" or c["tc"] == 8
    # one case has widths the inference decoder has no tile pair for; every other case compares the two forward paths
    assert [(k, A.CASES[k]["cfg"][2:4]) for k in A.CASES if not A.decoder_built(k)] == [("pbr-7x4x9-N1000-faces-off", (64, 128))]


@pytest.mark.parametrize("case", CASES)
def test_batch_converges_clear_of_every_kink(case):
    c = A.CASES[case]
    pts, sdf, tex = A.batch(case)                                # raises if its 40 rounds do not suffice
    assert tuple(pts.shape) == (c["N"], 3) and tuple(sdf.shape) == (c["N"], 1)
    assert (tex is None) == (c["net"] == "geo") and (tex is None or tuple(tex.shape) == (c["N"], c["tc"]))
    assert A.kink_distance(case) >= A.KINK
    if c["band_rows"] is not None:
        assert np.array_equal(sdf.numpy()[:len(c["band_rows"]), 0], c["band_rows"])


@pytest.mark.parametrize("case", [k for k, c in A.CASES.items() if c["net"] != "geo"])
def test_band_populations(case):
    c = A.CASES[case]
    s = np.abs(A.batch(case)[1].numpy()[:, 0])
    b, n = A.band(case), int((s < A.band(case)).sum())
    if c["loss"].get("one_row"):
        assert n == 1
    elif c["loss"].get("all_band"):
        assert n == c["N"]
    elif c["band_rows"] is not None:
        f = np.float32
        pinned = s[:8]
        assert list(pinned[:3] < b) == [True, False, False] and list(pinned[4:7] < b) == [True, False, False]
        assert pinned[0] == np.nextafter(b, f(0)) and pinned[1] == b and pinned[2] == np.nextafter(b, f(1))
        # the product of the two rounded factors falls on the other side of the band at the two settings
        assert (pinned[3] < b) == (c["loss"]["thr"] == 0.03) and pinned[3] in (pinned[0], pinned[2])
        assert 8 < n < c["N"]
    elif case in A.MODES:
        assert 0.1 * c["N"] < n < c["N"]
    else:
        assert n >= 1                                            # an empty band is NaN by definition: no case has one


def test_the_bounds_follow_the_rule():
    """the shared bound wherever ten times the gap written beside it is below it, otherwise ten times the gap, two digits, up"""
    for case, row in A.BOUNDS.items():
        assert tuple(row) == A.quantities(case)
        for q, (bound, gap) in row.items():
            assert bound == A.bound_for(q, gap), (case, q, bound, gap)
            if 10 * gap < A.SHARED[q]:
                assert bound == A.SHARED[q]
            else:
                assert 10 * gap <= bound <= 1.1 * 10 * gap, (case, q, bound, gap)


def _over(case, err):
    return {q: err[q] / A.BOUNDS[case][q][0] for q in A.quantities(case)}


@pytest.mark.parametrize("case", CASES)
def test_float32_restatement_stays_inside_every_bound(case):
    over = _over(case, A.float32_gap(case))
    print(case, " ".join(f"{q} {v:.2f}" for q, v in over.items()))
    assert max(over.values()) < 1, over
    # the analytically zero gradients are zero in float64, and nothing else is
    grad_r = A.reference(case)[3]
    gmax = max(float(v.norm()) for v in grad_r.values())
    zero = A.ZERO_GRAD[A.CASES[case]["net"]]
    assert set(zero) <= set(grad_r)
    for k, v in grad_r.items():
        assert (float(v.norm()) < 1e-12 * gmax) == (k in zero), (k, float(v.norm()), gmax)


def _fault_leaves(case, fault, where=None):
    over = _over(case, A.float32_gap(case, fault))
    print(case, fault, " ".join(f"{q} {v:.1f}x" for q, v in over.items()))
    assert max(over.values()) > 10, (case, fault, over)
    if where == "forward":
        assert over["pred"] > 10, over
    elif where == "backward":
        assert over["pred"] < 1 and over["encode"] < 1 and max(over["grad"], over["zero"]) > 10, over
    elif where == "loss":
        assert over["pred"] < 1 and over["loss"] > 10, over
    return over


@pytest.mark.parametrize("fault", P.FAULTS)
def test_each_fault_of_the_pbr_cases_stays_caught(fault):
    for case in ("pbr-3x3x3-N63-cell", "pbr-7x4x9-N1000-faces-off"):
        _fault_leaves(case, fault, "forward" if fault in ("residual_f0", "norm0_on_input", "sigmoid") else None)


def test_one_mean_over_eight_columns_stays_caught():
    for case in ("skip8-7x4x9-N65-faces-off", "skip8-band-holds-one"):
        _fault_leaves(case, "one_mean", "loss")


@pytest.mark.parametrize("case", ["pbr-1x6x5-N1-uniform", "pbr-2x33x3-N64-lattice-unit", "pbr-3x3x3-N63-cell"])
def test_a_3x3_convolution_that_pads_one_row_short_leaves_the_bounds(case):
    """forward values right, every gradient of the 3x3 blocks from a convolution whose lower halo row reads as zero: planes one
    pixel high are not touched by it (1x6x5 has one plane of 6 x 5), planes two and three pixels high are"""
    _fault_leaves(case, "conv3_short_row", "backward")


@pytest.mark.parametrize("case", ["skip8-band-holds-one", "pbr-band-holds-one", "skip8-2x33x3-N1-uniform", "pbr-1x6x5-N1-uniform"])
def test_a_group_mean_divided_by_eight_columns_leaves_the_bounds(case):
    _fault_leaves(case, "mean_cnt8", "loss")


@pytest.mark.parametrize("case, fault", [("pbr-1x6x5-N1-uniform", "normal_point_grad"), ("pbr-3x3x3-N63-cell", "normal_point_grad"),
                                         ("skip8-2x33x3-N1-uniform", "chain2_drop"), ("skip5-7x4x9-N257-uniform", "chain2_drop")])
def test_dropped_chain_2_point_gradients_leave_the_bounds(case, fault):
    """one head's gradient never reaches the gathered texture feature, at fewer points than one 64-row tile"""
    _fault_leaves(case, fault, "backward")


@pytest.mark.parametrize("case", ["geo-7x4x9-N63-faces-off", "skip8-7x4x9-N65-faces-off", "pbr-7x4x9-N1000-faces-off"])
def test_an_aabb_treated_as_centred_leaves_the_bounds(case):
    _fault_leaves(case, "aabb_centred", "forward")


@pytest.mark.parametrize("case", list(A.BAND))
def test_a_band_taken_with_le_leaves_the_bounds(case):
    """the two pinned rows with |sdf| exactly at the band enter every group mean"""
    _fault_leaves(case, "band_le", "loss")
