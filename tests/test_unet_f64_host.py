"""The float64-reference harness of the UNet tests (tests/unet_f64_cases.py) on the CPU alone.

1. The float32 port stays under fixed caps on every case.  The GPU test (tests/test_hip_unet_f64.py) holds the device to a
   multiple of the float32 port's own error, so a case whose float32 evaluation drifts or is ill-conditioned would loosen it
   silently; the caps are the ceiling of that yardstick.  They are conditions on the inputs: a case that breaks one needs other
   inputs, never a wider cap.
2. The metrics see faults the older gates cannot: relerr < 1e-4 on a forward, and the per-tensor L2 error floored at 1 % of
   the largest tensor norm < 5e-4 on gradients (tests/test_hip_train.py:test_grads_vs_oracle_wider).
3. The same for faults that only an error in the latent width produces (cases W4 and W16): the last output channel, the first
   channel beyond 12, the last row / column / element of the gradients of out.2 and in_conv.0, a loss mean over 12 channels."""
import numpy as np
import pytest

import unet_f64_cases as U
from conftest import relerr


@pytest.mark.parametrize("case", list(U.CASES))
def test_float32_port_stays_under_the_caps(case, oracle, record_property):
    e = U.port_errors(case)
    record_property("errors", e)
    cap = U.CAPS[U.CASES[case]["large_t"]]
    msg = f"reference ill-conditioned: choose other inputs ({case}: {e})"
    assert e["fwd"] <= cap["fwd"], msg
    assert e["loss_only"] <= cap["loss"], msg
    assert e["loss"] <= cap["terms"], msg
    assert e["grad"] <= cap["grad"], msg
    assert e["zero"] <= cap["zero"], msg


def test_float64_run_takes_the_float32_values_promoted(oracle):
    """Same parameter, x0 and noise values on both sides; x_t is formed in float64 from the float64 tables (so it differs from the
    float32 x_t by that one rounding and no more), and the float32 run is the port as it always was (float32 throughout)."""
    p32, p64 = U.port("A'", False), U.port("A'", True)
    assert p32["x_t"].dtype == np.float32 and p64["x_t"].dtype == np.float64
    d = np.abs(p32["x_t"] - p64["x_t"])
    assert 0 < d.max() <= 3 * 2.0 ** -24 * np.abs(p64["x_t"]).max()
    assert all(v.dtype == np.float64 for v in p64["grads"].values())
    assert sorted(p64["grads"]) == sorted(U.param_shapes("A'"))


def test_zero_gradient_tensors_are_the_one_channel_groups(oracle):
    """12 to 16 zero-gradient tensors at 32 channels (conv biases in front of a one-channel-per-group GroupNorm and, without
    scale-shift norm, the timestep projections added in front of one), none at wider models; the smallest other tensor is large
    enough that E_k needs no floor: 2 % of G at width 12 and above.  G is out.2's gradient, one output channel's signal per
    element, while an inner tensor's element adds the signals of all `ch` output channels with mixed signs, about sqrt(ch) of one:
    below width 12 the smallest tensor is held to 2 % * sqrt(ch / 12) of G (seven decades above ZERO_GRAD_REL either way)."""
    for case, c in U.CASES.items():
        g64 = U.port(case, True)["grads"]
        E, Z, G = U.grad_errors(g64, g64)
        assert all(k.endswith(".bias") and ".conv_" in k or ".emb_layers." in k and not c["ssn"] for k in Z), (case, sorted(Z))
        assert (12 <= len(Z) <= 16) if c["mc"] == 32 else not Z, (case, len(Z))
        assert min(float(np.max(np.abs(g64[k]))) for k in E) >= 2e-2 * min(1.0, (c["ch"] / 12) ** 0.5) * G, case


def _l2_floored(grads, grads64):
    """The measure of test_grads_vs_oracle_wider: per-tensor L2 error over max(the tensor's norm, 1 % of the largest norm)."""
    gmax = max(float(np.linalg.norm(v)) for v in grads64.values())
    return max(float(np.linalg.norm(grads[k].astype(np.float64) - r)) / max(float(np.linalg.norm(r)), 1e-2 * gmax)
               for k, r in grads64.items())


FACTOR = 4.0                     # every injected fault must push its metric above 4x the clean value


def test_one_weight_gradient_element_off_by_3e_5(oracle):
    p32, p64 = U.port("B", False), U.port("B", True)
    k = "input_blocks.0.0.out_layers.2.conv_xy.weight"
    clean = U.worst_of(U.grad_errors(p32["grads"], p64["grads"])[0])[0]
    g = dict(p32["grads"])
    g[k] = g[k].copy()
    g[k][5, 7, 2, 1] += np.float32(3e-5 * np.abs(p64["grads"][k]).max())
    E, _, _ = U.grad_errors(g, p64["grads"])
    assert U.worst_of(E) == (E[k], k) and E[k] > FACTOR * clean, (E[k], clean)
    assert _l2_floored(g, p64["grads"]) < 5e-4                      # the old gate does not move


def test_last_column_of_one_output_plane_scaled(oracle):
    H, W, D = U.CASES["B"]["hwd"]
    p32, p64 = U.port("B", False), U.port("B", True)
    clean = U.forward_error(p32["y"], p64["y"], (H, W, D))[0]
    y = p32["y"].copy()
    y[1, :, :H, W - 1] *= np.float32(1 + 3e-5)                      # sample 1, plane xy, its last column
    e, at = U.forward_error(y, p64["y"], (H, W, D))
    assert at == (1, "xy") and e > FACTOR * clean, (e, at, clean)
    assert relerr(y, p64["y"]) < 1e-4                               # the old gate does not move


def test_one_sample_contribution_scaled(oracle):
    p32, p64 = U.port("B", False), U.port("B", True)
    only1 = U.port("B", False, w=(0.0, 1.0))["grads"]               # sample 1's share of the batch-mean gradient
    clean = U.worst_of(U.grad_errors(p32["grads"], p64["grads"])[0])[0]
    g = {k: v + np.float32(1e-3) * only1[k] for k, v in p32["grads"].items()}
    E, _, _ = U.grad_errors(g, p64["grads"])
    assert U.worst_of(E)[0] > FACTOR * clean, (U.worst_of(E), clean)


def test_one_bias_gradient_quad_zeroed(oracle):
    p32, p64 = U.port("B", False), U.port("B", True)
    k = "output_blocks.1.0.out_layers.2.conv_xy.bias"
    clean = U.worst_of(U.grad_errors(p32["grads"], p64["grads"])[0])[0]
    g = dict(p32["grads"])
    g[k] = g[k].copy()
    g[k][4:8] = 0                                                   # the second output-channel quad
    E, _, _ = U.grad_errors(g, p64["grads"])
    assert U.worst_of(E) == (E[k], k) and E[k] > FACTOR * clean, (E[k], clean)


# ------------------------------------------------------------------------------------- faults only a width error produces
WIDTH_CASES = ("W4", "W16")


def _clean(case):
    """The unfaulted float32 port's errors on the case, under the caps."""
    e, cap = U.port_errors(case), U.CAPS[False]
    assert e["fwd"] <= cap["fwd"] and e["loss"] <= cap["terms"] and e["grad"] <= cap["grad"], (case, e)
    return e


@pytest.mark.parametrize("case,channel", [("W4", 3), ("W16", 15), ("W16", 12)])
def test_one_output_channel_of_one_plane_off(case, channel, oracle):
    """The last output channel (a head that masks or stages one channel too few), and on W16 channel 12, the first beyond the width
    every other case has: one plane of one sample off by 1e-4 of the plane's maximum."""
    H, W, D = U.CASES[case]["hwd"]
    p32, p64 = U.port(case, False), U.port(case, True)
    assert p32["y"].shape[1] == U.CASES[case]["ch"] > channel
    y = p32["y"].copy()
    y[1, channel, :H, W:] += np.float32(1e-4 * np.abs(p64["y"][1, :, :H, W:]).max())        # sample 1, plane xz
    e, at = U.forward_error(y, p64["y"], (H, W, D))
    assert at == (1, "xz") and e > FACTOR * _clean(case)["fwd"], (e, at)


def _grad_fault(case, k, edit):
    p32, p64 = U.port(case, False), U.port(case, True)
    g = dict(p32["grads"])
    g[k] = g[k].copy()
    edit(g[k], U.CASES[case]["ch"])
    assert not np.array_equal(g[k], p32["grads"][k])
    E, _, _ = U.grad_errors(g, p64["grads"])
    assert U.worst_of(E) == (E[k], k) and E[k] > FACTOR * _clean(case)["grad"], (case, k, E[k])


def _scale_last_row(g, ch):
    g[ch - 1] *= np.float32(ch / 12)


def _zero_last_column(g, ch):
    g[:, ch - 1] = 0


def _zero_last_element(g, ch):
    g[ch - 1] = 0


@pytest.mark.parametrize("case", WIDTH_CASES)
@pytest.mark.parametrize("k,edit", [("out.2.conv_yz.weight", _scale_last_row),           # a mean over 12 channels in one row
                                    ("in_conv.0.conv_xz.weight", _zero_last_column),     # an input channel the outer product skips
                                    ("out.2.conv_xy.bias", _zero_last_element)],         # the last of the S channel sums
                         ids=["out2_row_scaled", "in_conv_column_zeroed", "out2_bias_zeroed"])
def test_gradient_faults_of_the_last_channel(case, k, edit, oracle):
    _grad_fault(case, k, edit)


@pytest.mark.parametrize("case", WIDTH_CASES)
def test_loss_terms_as_a_mean_over_12_channels(case, oracle):
    p32, p64 = U.port(case, False), U.port(case, True)
    ch = U.CASES[case]["ch"]
    terms = {k: v * np.float32(ch / 12) for k, v in p32["terms"].items()}
    e, _ = U.loss_error(terms, p64["terms"])
    assert e > FACTOR * max(_clean(case)["loss"], U.EPS32) and e > 0.2, e
