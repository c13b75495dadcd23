"""The float64-reference harness of the decoder tests (tests/decoder_f64_cases.py) on the CPU alone.

1. The float32 restatement stays under fixed caps on every case and stage.  The GPU test (tests/test_hip_decoder_f64.py) holds
   the device to a multiple of the float32 restatement's own error, so a case whose float32 evaluation drifts or is
   ill-conditioned would loosen it silently; the caps are the ceiling of that yardstick.  They are conditions on the inputs: a
   case that breaks one gets other inputs, never a wider cap.
2. The per-plane and per-column metrics see faults that relerr < 1e-4 over the whole array (test_pbr_gpu.py, test_hip_parity.py)
   cannot: each injected fault lifts its metric above 4 times the clean value while the old gate stays below 1e-4.
3. A wrong sampler in the gather (zero padding, align_corners=True) shows at full size, more than 100 times the cap, and is
   located: see test_a_wrong_sampler_shows_at_full_size_and_is_located for what that means for each sampler.
4. The designed rows put a low clamp, a high clamp and a texel centre on the row and on the column coordinate of every plane."""
import numpy as np
import pytest

import decoder_f64_cases as Dc

FACTOR = 4.0                     # every injected fault must push its metric above 4x the clean value
OLD_GATE = 1e-4


@pytest.mark.parametrize("case", list(Dc.CASES))
def test_float32_restatement_stays_under_the_caps(case, record_property):
    y = Dc.yardstick(case)
    record_property("errors", {k: v for k, v in y.items() if isinstance(v, float)})
    print(case, y)
    msg = f"reference ill-conditioned: choose other inputs ({case}: {y})"
    assert 0 < y["plane"] <= Dc.CAPS["plane"], msg
    assert 0 < y["point"] <= Dc.CAPS["point"], msg
    if Dc.CASES[case]["grid"]:
        assert 0 < y["grid"] <= Dc.CAPS["grid"], msg


@pytest.mark.parametrize("case", list(Dc.CASES))
def test_inputs_are_what_the_metrics_assume(case):
    """Both evaluations take the same float32 values; no output column is small; the one-point set is row 0 of the larger one."""
    c = Dc.CASES[case]
    r32, r64 = Dc.restated(case, False), Dc.restated(case, True)
    for n in c["n"]:
        assert r32["out"][n].dtype == np.float32 and r64["out"][n].dtype == np.float64
        assert r64["out"][n].shape == (n, {"skip": 4, "skip8": 9, "pbr": 9, "geo": 1}[c["kind"]])
        assert np.array_equal(Dc.points(case, n)[0], Dc.points(case, max(c["n"]))[0])
    assert all(f.dtype == np.float32 for fs in r32["feats"].values() for f in fs)
    assert all(f.shape[0] == c["up"] for fs in r64["feats"].values() for f in fs)
    assert sorted(r64["feats"]) == {"pbr": ["geo", "tex", "tex0"], "geo": ["geo"]}.get(c["kind"], ["geo", "tex"])
    assert Dc.column_scale(case).min() >= Dc.COLUMN_FLOOR, Dc.column_scale(case)
    if c["grid"]:
        dims = Dc.GRID_DIMS[case]
        assert len(set(dims)) == 3 and np.prod(dims) % 128 and r64["grid"].shape[0] == np.prod(dims)
        assert np.abs(r64["grid"]).max(axis=0).min() >= Dc.COLUMN_FLOOR
        mat = r64["grid"][:, 1:]
        if c["kind"] == "pbr":                                          # (the skip net's sigmoid columns never reach the clamp)
            assert mat.min() == 0 and mat.max() == 1                   # the clamp of the material columns acts, both ways


@pytest.mark.parametrize("case", list(Dc.CASES))
def test_designed_rows_reach_every_border_condition(case, record_property):
    n = max(Dc.CASES[case]["n"])
    rows = Dc.designed_rows(n)
    assert set(rows) >= {i for i in (0, 31, 32, 63, 64, 127, 128) if i < n} | {n - 1}
    cond = Dc.input_conditions(case, n)
    record_property("conditions", {f"{p}.{w}": v for (p, w), v in cond.items()})
    assert sorted(cond) == sorted((p, w) for p in ("xy", "xz", "yz") for w in ("row", "col"))
    for key, counts in cond.items():
        for what, (among_all, among_designed) in counts.items():
            assert among_designed >= 1 and among_all >= among_designed, (case, key, what, counts)
    if n >= 97:                                                         # eight designed rows and more: every axis takes every value
        sizes = Dc.CASES[case]["hwd"]
        lo, hi = Dc.AABB32[:3].astype(np.float64), Dc.AABB32[3:].astype(np.float64)
        x = 2 * (Dc.points(case, n)[rows].astype(np.float64) - lo) / (hi - lo) - 1
        for a in range(3):
            for v in range(len(Dc.VALUES)):
                assert np.abs(x[:, a] - Dc._value(v, sizes[a])).min() < 1e-6, (case, a, Dc.VALUES[v])
    # rows in both blocks' first and last lanes of a wave, and in the tail block where there is one
    assert {r % 32 for r in rows} >= ({0, 31} if n >= 32 else {0})
    assert n <= 128 or any(r >= 128 * ((n - 1) // 128) for r in rows)


# ---------------------------------------------------------------------------------------------- faults the old gate cannot see
@pytest.mark.parametrize("case", list(Dc.CASES))
def test_sdf_column_scaled_by_2e_5(case):
    n = max(Dc.CASES[case]["n"])
    y32, y64 = Dc.restated(case, False)["out"][n], Dc.restated(case, True)["out"][n]
    clean = Dc.point_error(case, n, y32, y64)[3]
    y = y32.copy()
    y[:, 0] *= np.float32(1 + 2e-5)
    e, j, where, E = Dc.point_error(case, n, y, y64)
    assert j == 0 and E[0] > FACTOR * clean[0] and e > FACTOR * clean.max(), (E, clean)
    assert np.array_equal(E[1:], clean[1:])
    assert Dc.old_gate(y, y64) < OLD_GATE


def test_tail_block_rows_of_lane_half_1_offset():
    """Columns 5..8 of case B (rows 4..7 of the texture head's output tile: lane half 1) on the two live points of block 1."""
    n = 130
    y32, y64 = Dc.restated("B", False)["out"][n], Dc.restated("B", True)["out"][n]
    assert [Dc.half_of_column("skip8", j) for j in range(9)] == [0, 0, 0, 0, 0, 1, 1, 1, 1]
    clean = Dc.point_error("B", n, y32, y64)[3]
    y = y32.copy()
    y[128:, 5:] += (1e-5 * np.abs(y64[:, 5:]).max(axis=0)).astype(np.float32)
    e, j, where, E = Dc.point_error("B", n, y, y64)
    assert (E[5:] > FACTOR * clean[5:]).all() and e > FACTOR * clean.max(), (E, clean)
    assert j >= 5 and where["block"] == 1 and where["half"] == 1 and where["lane"] >= 32, where
    assert Dc.old_gate(y, y64) < OLD_GATE


def test_one_border_point_moved_in_a_colour_column():
    n = 257
    y32, y64 = Dc.restated("A", False)["out"][n], Dc.restated("A", True)["out"][n]
    clean = Dc.point_error("A", n, y32, y64)[3]
    row = 64                                                            # designed: outside every plane
    assert row in Dc.designed_rows(n) and (np.abs(Dc.points("A", n)[row]) > Dc.AABB32[3:]).all()
    y = y32.copy()
    y[row, 2] += np.float32(2e-5)
    e, j, where, E = Dc.point_error("A", n, y, y64)
    assert j == 2 and e > FACTOR * clean.max(), (E, clean)
    assert where == dict(point=64, block=0, wave=2, lane=0, half=0, designed=True), where
    assert Dc.old_gate(y, y64) < OLD_GATE


def test_one_channel_quad_of_one_plane_scaled():
    r32, r64 = Dc.restated("D", False)["feats"], Dc.restated("D", True)["feats"]
    clean = Dc.plane_errors(r32, r64)
    feats = {g: [f.copy() for f in fs] for g, fs in r32.items()}
    feats["tex"][1][92:96] *= np.float32(1 + 2e-5)                      # plane xz, the last quad of the 24
    E = Dc.plane_errors(feats, r64)
    assert Dc.worst_of(E) == (E["tex", "xz"], ("tex", "xz")) and E["tex", "xz"] > FACTOR * max(clean.values()), (E, clean)
    assert all(E[k] == clean[k] for k in E if k != ("tex", "xz"))
    assert max(Dc.old_gate(f, r) for g in feats for f, r in zip(feats[g], r64[g])) < OLD_GATE


# ---------------------------------------------------------------------------------------------------------- structural faults
def _row_errors(case, n, y, y64):
    """[n]: each point's worst column error on the case's column scale"""
    return (np.abs(np.asarray(y, np.float64) - y64) / Dc.column_scale(case)).max(axis=1)


@pytest.mark.parametrize("sampler", ["padding_mode=zeros", "align_corners=True"])
@pytest.mark.parametrize("case", list(Dc.CASES))
def test_a_wrong_sampler_shows_at_full_size_and_is_located(case, sampler, record_property):
    """Where each wrong sampler differs from the network's, per coordinate (s = the plane size along the axis):
    zero padding     beyond the outermost texel centres, |x| > 1 - 1/s (a row all of whose coordinates lie within them reads the
                     same texels with the same weights: it must stay at the float32 restatement's error);
    align_corners    strictly between the borders, 0 < |x| < 1, by x/2 texels, most at the outermost texel centres (at |x| >= 1
                     both samplers clamp to the same border texel: such a row must stay at the float32 restatement's error).
    Located: the worst point of the point set that can carry the statement is a designed row.  For zero padding that set is the
    designed rows and the uniform rows the sampler cannot reach; the uniform rows beyond the outermost centres (they go to
    +-1.15) are hit as fully as the designed ones and are left out of this maximum, and held to the band instead: every point
    above 100 times the cap has a coordinate in the band.  For align_corners every uniform row is reached, so the maximum is
    over the designed rows, and what is asserted of them is where it falls: on a row with a coordinate between the borders, with
    the row on the outermost centres of all three planes above 100 times the cap and the rows on and beyond the borders clean."""
    zeros = sampler.startswith("padding")
    wrong = Dc.restated(case, False, **(dict(padding_mode="zeros") if zeros else dict(align_corners=True)))
    r64 = Dc.restated(case, True)
    sizes = np.asarray(Dc.CASES[case]["hwd"], np.float64)
    big, clean_cap = 100 * Dc.CAPS["point"], Dc.CAPS["point"]
    for n in Dc.CASES[case]["n"]:
        rows = np.asarray(Dc.designed_rows(n))
        x = Dc.normalised(case, n)
        tol = 1e-6                                                      # (a designed coordinate carried by a rounded float32 point)
        reached = (np.abs(x) > 1 - 1 / sizes + tol).any(axis=1) if zeros else ((np.abs(x) > tol) & (np.abs(x) < 1 - tol)).any(axis=1)
        err = _row_errors(case, n, wrong["out"][n], r64["out"][n])
        e, j, where, _ = Dc.point_error(case, n, wrong["out"][n], r64["out"][n])
        record_property(f"n={n}", dict(worst=(e, j, where), reached=int(reached.sum()), designed_reached=int(reached[rows].sum())))
        print(case, sampler, n, f"all rows {e:.2e} at {where}; {int(reached.sum())} rows reached, {int(reached[rows].sum())} of them designed")
        # at full size, on all rows and on the designed rows alone
        assert e > big and err[rows].max() > big, (case, sampler, n, e, err[rows].max())
        # a row the sampler cannot reach stays under the float32 restatement's cap (from 96 points on there is a designed one: the
        # interior centres of row 5 for zero padding, the rows at +-1 and +-1.5 for align_corners)
        assert n < 96 or (~reached[rows]).sum() >= 1, (case, n, "no designed row out of the sampler's reach")
        if (~reached).any():
            assert err[~reached].max() <= clean_cap, (case, sampler, n, err[~reached].max())
        # every point far over the cap is one the sampler reaches
        assert reached[err > big].all() and (err > big).sum() >= 1
        # located
        keep = np.zeros(n, bool)
        keep[rows] = True
        if zeros:
            keep |= ~reached
        at = int(np.argmax(np.where(keep, err, -1.0)))
        assert reached[at] and err[at] > big, (case, sampler, n, at, err[at])
        if zeros:                                                       # (for align_corners the maximum is over the designed rows)
            assert at in rows, (case, sampler, n, at, err[at])
        if not zeros and n >= 64:                                       # TABLE row 3: the outermost centres of all three planes
            assert Dc.TABLE[3] == (3, 2, 3) and err[rows[3]] > big, (case, n, rows[3], err[rows[3]])
    assert wrong["feats"].keys() == r64["feats"].keys()                 # (the plane stage is not touched by the sampler)
