"""The decode path on the MI355X against the restatement tests/pbr_cases.py evaluated in float64: the plane stage
(s3d_decoder_prepare_triplane) per feature group and plane, and every output column of the fused gather + MLP point kernel
k_decode<UPT,HIDT>, for each of the five compiled tile pairs and the padded forms of each (tests/decoder_f64_cases.py: cases,
points, metrics), in point mode and in grid mode.

Bounds.  A device error is held to a multiple of the float32 restatement's error on the same case, computed here on the CPU:
err_dev <= K * max(err_32, 2^-23), per stage; the sdf column, which decides the mesh, is held to its OWN float32 error as well
(in the PBR cases a normal column sets the stage's yardstick, several times the sdf column's).  The float32 restatement is itself
held under fixed caps (Dc.CAPS; tests/test_decoder_f64_host.py, and again here on the values this run computed), so no plane error
above K_PLANE * 1.1e-6 of a plane's maximum, no column error above K_POINT * 3e-6 of the column's maximum (grid mode: K_GRID *
3.2e-6) can pass.

K = twice the worst device / yardstick ratio over all cases, rounded up to a power of two.  Measured on an
MI355X (profiles/decoder_f64.txt, from tools/decoder_f64_report.py):
  stage    worst device / float32 ratio                       2x, to a power of two    device errors over the cases
  plane    2.71 (A, geo xy; device 1.53e-6, float32 5.6e-7)   K_PLANE = 8              1.3e-7 - 1.5e-6
  point    1.89 (B, column 0; device 5.9e-7, float32 3.1e-7)  K_POINT = 4              5.2e-7 - 2.2e-6
  sdf      1.89 (B;           device 5.9e-7, float32 3.1e-7)  K_SDF   = 4              5.2e-7 - 1.2e-6
  grid     1.57 (D, column 5; device 2.2e-6, float32 1.4e-6)  K_GRID  = 4              6.2e-7 - 2.7e-6
No ratio exceeds 8.  The plane stage sits furthest from the yardstick: its 5x5 convolutions accumulate 800 and 1600 (2400 at
width 96) products in one fp32 MFMA chain per output, the CPU's convolution in blocked partial sums.  The float32 restatement's
own error moves with the host's convolution and GEMM kernels (case C, point stage: 1.75e-6 and 2.0e-6 on two hosts), which is
why the bound takes it at run time and the caps hold it.
"""
import numpy as np
import pytest
import torch

import decoder_f64_cases as Dc
import pbr_cases as P
from sin3dm_amd import testing as T

pytestmark = pytest.mark.gpu

K_PLANE, K_POINT, K_SDF, K_GRID = 8, 4, 4, 4


@pytest.fixture(scope="module")
def runs():
    """device_run of each case, once"""
    cache = {}

    def get(case):
        if case not in cache:
            cache[case] = Dc.device_run(case)
        return cache[case]
    return get


def _yardstick(case):
    y = Dc.yardstick(case)
    over = {k: (y[k], cap) for k, cap in Dc.CAPS.items() if k in y and y[k] > cap}
    assert not over, f"reference ill-conditioned: choose other inputs ({case}: {over})"
    return y


@pytest.mark.parametrize("case", list(Dc.CASES))
def test_point_mode(case, runs, record_property):
    """Plane features and decoded points of a fresh net against float64, per plane and per output column."""
    c = Dc.CASES[case]
    yard = _yardstick(case)
    res = runs(case)
    dev = Dc.device_errors(case, res)
    rat = Dc.ratios(dev, yard)
    record_property("errors", {k: (dev[k], yard[k], rat[k]) for k in ("plane", "point", "sdf")})
    print(case, c["kernel"], {k: f"{dev[k]:.2e} / {yard[k]:.2e} = {rat[k]:.2f}" for k in ("plane", "point", "sdf")},
          "worst column", dev["point_col"], "at", dev["point_place"])
    bound = K_PLANE * max(yard["plane"], Dc.EPS32)
    bad = {k: e for k, e in dev["planes"].items() if not e <= bound}
    assert not bad, (case, "plane stage", bad, "float32 restatement", yard["plane"], yard["plane_at"])
    bound = K_POINT * max(yard["point"], Dc.EPS32)
    for n, E in dev["columns"].items():
        assert np.isfinite(res["out"][n]).all()
        bad = {j: float(e) for j, e in enumerate(E) if not e <= bound}
        assert not bad, (case, c["kernel"], f"{n} points", "columns over the bound", bad, "worst", dev["point_col"], "at",
                         dev["point_place"], "float32 restatement", yard["point"])
    assert dev["sdf"] <= K_SDF * max(yard["sdf"], Dc.EPS32), (case, c["kernel"], "sdf column", dev["sdf"], "its float32 error", yard["sdf"])
    if len(c["n"]) > 1:                                   # the one-point launch is the same lane of the same kernel
        assert np.array_equal(res["out"][1][0], res["out"][max(c["n"])][0])


@pytest.mark.parametrize("case", Dc.GRID_CASES)
def test_grid_mode(case, runs, record_property):
    """decode_grid against float64 on the float32 cell centres as the reference computes them, material columns clamped; and
    against point mode on those centres."""
    yard = _yardstick(case)
    dev = Dc.device_errors(case, runs(case))
    rat = dev["grid"] / max(yard["grid"], Dc.EPS32)
    record_property("errors", (dev["grid"], yard["grid"], rat, dev["grid_vs_points"]))
    print(case, f"grid {dev['grid']:.2e} / {yard['grid']:.2e} = {rat:.2f}, column {dev['grid_col']}, cell {dev['grid_cell']}; "
          f"grid mode vs point mode {dev['grid_vs_points']:.2e}")
    assert dev["grid"] <= K_GRID * max(yard["grid"], Dc.EPS32), (case, dev["grid"], dev["grid_col"], dev["grid_cell"], yard["grid"])
    assert dev["grid_vs_points"] < 1e-5, "grid mode and point mode must agree"


# --------------------------------------------------------------------------------------------------- live against fresh
def _fresh(case, state):
    net = Dc.make_net(case)
    net.load_state_dict(state, strict=False)
    return net


@pytest.mark.parametrize("case", ["C", "F"])
def test_live_net_equals_a_fresh_one(case):
    """In-place parameter updates (the version stamp moves, the storage does not) and a triplane of another size and back: the
    live net decodes the bits of a net built fresh from its state.  A write through `p.data` moves neither the stamp nor the
    storage (`.data` is a view with a version counter of its own): it is announced with mark_parameters_changed(), as for the
    UNet, and then gives the fresh net's bits too."""
    c = Dc.CASES[case]
    n = max(c["n"])
    pts = torch.from_numpy(Dc.points(case, n).copy()).to("cuda:0")
    aabb = torch.from_numpy(Dc.AABB32)
    fm = [f.to("cuda:0") for f in Dc.inputs(case)]
    other = [torch.from_numpy(np.ascontiguousarray(f)).to("cuda:0") for f in P.synthetic_planes(3, 4, 5, seed=70)]
    live = Dc.make_net(case)
    first = live.decode(pts, fm, aabb=aabb).clone()
    head = "normal_decoder" if c["kind"] == "pbr" else "tex_decoder"
    names = ("geo_decoder.second_layers.0.weight", f"{head}.first_layers.2.bias", "geo_convs.out_layers.1.weight")
    params = dict(live.named_parameters())
    with torch.no_grad():
        for k, name in enumerate(names):
            before, where = params[name]._version, params[name].data_ptr()
            params[name].mul_(1.0 + 0.125 * (k + 1))
            assert params[name]._version > before and params[name].data_ptr() == where
    state = {k: v.detach().clone() for k, v in live.state_dict().items()}
    updated = live.decode(pts, fm, aabb=aabb).clone()
    fresh = _fresh(case, state)
    want = fresh.decode(pts, fm, aabb=aabb)
    assert torch.equal(updated, want), "a live net after in-place updates decodes other bits than a fresh one"
    assert not torch.equal(updated[:, 0], first[:, 0]) and not torch.equal(updated[:, -1], first[:, -1])
    for g in Dc.restated(case, True)["feats"]:
        for a, b in zip(live.plane_features(fm, g), fresh.plane_features(fm, g)):
            assert torch.equal(a, b), g
    # another triplane size and back
    elsewhere = live.decode(pts, other, aabb=aabb)
    assert torch.equal(elsewhere, fresh.decode(pts, other, aabb=aabb)) and not torch.equal(elsewhere, want)
    assert torch.equal(live.decode(pts, fm, aabb=aabb), want)
    assert torch.equal(live.decode_grid(fm, 9, aabb=aabb), _fresh(case, state).decode_grid(fm, 9, aabb=aabb))
    # a write through .data, announced
    before = params[names[0]]._version
    params[names[0]].data.mul_(0.5)
    assert params[names[0]]._version == before
    live.mark_parameters_changed()
    state2 = {k: v.detach().clone() for k, v in live.state_dict().items()}
    again = live.decode(pts, fm, aabb=aabb)
    assert torch.equal(again, _fresh(case, state2).decode(pts, fm, aabb=aabb)) and not torch.equal(again[:, 0], want[:, 0])
    # and the updated net is still the network: against float64 on the updated values
    y = {}
    for dt in (torch.float32, torch.float64):
        sd = {k: v.to("cpu", dt) for k, v in state.items()}
        y[dt] = P.decode(c["kind"], sd, Dc.points(case, n).copy(), [f.to(dt) for f in Dc.inputs(case)], Dc.AABB32, dtype=dt).numpy()
    E32, _ = Dc.column_errors(y[torch.float32], y[torch.float64])
    E, _ = Dc.column_errors(updated.cpu().numpy(), y[torch.float64])
    assert E32.max() <= Dc.CAPS["point"] and E.max() <= K_POINT * max(E32.max(), Dc.EPS32), (E, E32)


def test_width_pair_without_a_kernel_is_refused():
    """up 64 / hidden 64 pads to tiles <2,2>, which is not compiled: an error naming both widths.  decode allocates its result
    itself and run_decode refuses before any launch, so the raise is the whole check that nothing is produced."""
    from sin3dm_amd.encoding.networks import AutoEncoderGroupSkip
    net = AutoEncoderGroupSkip(4, 8, 64, 64, 4, use_tex=True, tex_channels=3)
    net.load_state_dict(T.synthetic_state_dict(P.shapes_of("skip", 64, 64), 5), strict=False)
    net.to("cuda:0").eval()
    fm = [torch.from_numpy(np.ascontiguousarray(f)).to("cuda:0") for f in P.synthetic_planes(2, 3, 2)]
    pts = torch.from_numpy(Dc.points("E", 127).copy()).to("cuda:0")
    with pytest.raises(NotImplementedError) as e:
        net.decode(pts, fm, aabb=torch.from_numpy(Dc.AABB32))
    assert "feat_channel_up=64" in str(e.value) and "mlp_hidden_channels=64" in str(e.value), str(e.value)
    with pytest.raises(NotImplementedError, match="mlp_hidden_channels=64"):
        net.decode_grid(fm, 9, aabb=torch.from_numpy(Dc.AABB32))
    torch.cuda.synchronize()
