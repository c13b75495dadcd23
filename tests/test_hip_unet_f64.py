"""The diffusion UNet on the MI355X against oracle/torch_port.py evaluated in float64: the inference forward, the loss terms and
every element of every gradient of a training step, in the default kernel forms and with each form forced that a launch size
or an option would select (tests/unet_f64_cases.py: cases, forms, metrics).

Bounds.  A device error is held to a multiple of the float32 port's error on the same case, computed here on the CPU:
err_dev <= K * max(err_port32, 2^-23).  The float32 port is itself held under fixed caps (U.CAPS; tests/test_unet_f64_host.py,
and again here on the values this run computed), so with timesteps <= 3 no forward error above K_FWD * 2.5e-6 = 1e-5 of a
plane's maximum, no loss term error above K_LOSS * 5e-7 = 2e-6 and no gradient element error above K_GRAD * 8e-6 = 6.4e-5 of its
tensor's maximum can pass (A', B': 8e-5, 8e-6, 6.4e-4).

A forced form must show that it ran: by the kernel names the library reports for its launches, or, where the form changes a
summation order, by output bits that differ from the default's (U.FORWARD_ENGAGED, U.FORWARD_DIFFERS, U.TRAINING_ENGAGED).

K = twice the worst ratio measured over all cases in the default forms, rounded up to a power of two; the forced forms are held
to the same K.  Measured on an MI355X (profiles/unet_f64.txt, from tools/unet_f64_report.py):
  quantity     worst device / port ratio, default forms    2x, to a power of two    worst ratio, forced forms
  forward      1.42 (Be;  device 1.2e-6, port 8.4e-7)      K_FWD  = 4               1.75 (Be, CONV_IMPL=naive)
  loss terms   1.25 (G4;  device 1.5e-7, port floored)     K_LOSS = 4               0.84 (D, WGRAD_WINO=0)
  E_k          2.24 (G2;  device 4.6e-6, port 2.1e-6)      K_GRAD = 8               1.19 (H, GNB_FUSED=0)
  Z_k          0.75 (G3;  device 1.5e-7, port 2.0e-7)      K_ZERO = 2               0.42 (A, WGRAD_WINO=0)

No ratio exceeds 8.  Device errors with timesteps <= 3: forward 0.87e-6 to 1.25e-6, worst E_k 1.5e-6 to 4.7e-6; at t = 999
(A', B'): forward 7.6e-6 / 8.9e-6, E_k 2.2e-5 / 3.8e-5, as the float32 port.  Width 96 (case F) passes.  G1 (no
rollout, odd planes) is refused by the library as by the reference; the test asserts the message, G1e runs the model on even planes.

Latent widths other than 12 (the W cases: 1, 4, 8, 11, 16, 20; `--data_type sdf` trains and samples at 4).  The inference side
changes form between 16 and 17 (k_in_conv_lds and k_out_head_px take up to 16 channels at 64 / 128 / 256 model channels, k_in_conv
and k_out_head + k_sampler the rest), the training side refuses above 12 (k_small_outer's register arrays): W16, W20 and W20n
have their forward held and their step refused, by message, from s3d_unet_train_attach.  Same K's; worst ratios of the ten
cases in the default forms: forward 1.39 (W20), loss terms 1.37 (W1), E_k 1.51 (W11), Z_k 0.39 (W4n); forced forms on W4 and W16:
forward 1.42 (W4, CONV_IMPL=naive), E_k 1.37.  Nothing was found wrong in the kernels at these widths.

Checked by hand on a scratch build: with sample 0's weight used for every sample in k_mse_grad, every test of case H here fails
while test_grads_vs_oracle_wider, test_training_losses_and_grads and test_unet_forward_golden pass.
Two more, for the width cases (values only, no address or bound changed).  k_mse_finalize dividing by 12 * h * w where it divides
by C * h * w: test_default_forms fails on its loss terms for W4, W4n, W4w, W4e, W1, W8 and W11, and so does
test_three_optimizer_steps_at_width_4, while the sixteen cases at width 12, the refused ones and test_training_losses_and_grads
pass.  k_in_conv_lds taking the weights of input channels below min(Cin, 12) only: test_default_forms[W16], both
test_fused_step_against_float64[W16-*] and the carried in_conv at width 16
(test_next_steps_in_conv_carried_by_the_output_head_is_the_same_bits[128-1-hwd5-False-16]: the head's tail keeps all sixteen) fail,
while every other case, width, fused step and test_unet_forward_golden pass.
"""
import numpy as np
import pytest

import unet_f64_cases as U

pytestmark = pytest.mark.gpu

K_FWD, K_LOSS, K_GRAD, K_ZERO = 4, 4, 8, 2


@pytest.fixture(scope="module", autouse=True)
def _port_on_path(oracle):                       # (the oracle fixture builds the C oracle the schedule tables come from)
    yield


def _hold(case, dev, record):
    """Every part of device_errors present in `dev` against the float32 port's error on the case."""
    prt = U.port_errors(case)
    cap = U.CAPS[U.CASES[case]["large_t"]]
    over = {k: (prt[k], cap[c]) for k, c in (("fwd", "fwd"), ("loss_only", "loss"), ("loss", "terms"), ("grad", "grad"), ("zero", "zero"))
            if prt[k] > cap[c]}
    assert not over, f"reference ill-conditioned: choose other inputs ({case}: {over})"
    rat = U.ratios(dev, prt)
    record("errors", {k: (dev[k], prt[k], rat[k]) for k in rat})
    print(case, {k: f"{dev[k]:.2e} / {prt[k]:.2e} = {rat[k]:.2f}" for k in rat})

    def floor(e):
        return max(e, U.EPS32)
    if "fwd" in dev:
        assert dev["fwd"] <= K_FWD * floor(prt["fwd"]), (case, "forward", dev["fwd"], dev["fwd_at"], prt["fwd"])
    if "loss" in dev:
        assert dev["loss"] <= K_LOSS * floor(prt["loss"]), (case, "loss", dev["loss"], dev["loss_at"], prt["loss"])
        bad = sorted(((e, k) for k, e in dev["E"].items() if not e <= K_GRAD * floor(prt["grad"])), reverse=True)
        assert not bad, (case, "gradient", bad[:6], prt["grad"])
        bad = sorted(((z, k) for k, z in dev["Z"].items() if not z <= K_ZERO * floor(prt["zero"])), reverse=True)
        assert not bad, (case, "zero-gradient noise", bad[:6], prt["zero"])


def _refused(case):
    with pytest.raises(NotImplementedError, match=U.CASES[case]["refused"]):
        U.device_forward(case)
    with pytest.raises(NotImplementedError, match=U.CASES[case]["refused"]):
        U.device_step(case)


@pytest.mark.parametrize("case", list(U.CASES))
def test_default_forms(case, record_property):
    """The inference forward on the float32 x_t and the graph-free training step; each twice, the same bits."""
    c = U.CASES[case]
    if c["refused"]:
        return _refused(case)
    y = U.device_forward(case)
    if c["train_refused"]:                       # wider than the training kernels take: the forward is held, the step is refused
        for autograd in (False, True):
            with pytest.raises(NotImplementedError, match=c["train_refused"]):
                U.device_step(case, autograd=autograd)
        return _hold(case, U.device_errors(case, y, None), record_property)
    _hold(case, U.device_errors(case, y, U.device_step(case)), record_property)


def test_autograd_path_with_unequal_weights(record_property):
    """Case H through (terms["loss"] * w).mean().backward() with w = [1, 0.25, 2]."""
    _hold("H", U.device_errors("H", None, U.device_step("H", autograd=True)), record_property)


_default_forward = {}


@pytest.mark.parametrize("form", [f"{n}={v}" for n, v in U.FORWARD_FORMS])
@pytest.mark.parametrize("case", U.FORWARD_FORM_CASES)
def test_forward_forms(case, form, record_property):
    name, value = form.split("=")
    kernels = {}
    with U.forced(name, value):
        y = U.device_forward(case, kernels)
    record_property("kernels", kernels)
    if form in U.FORWARD_ENGAGED:
        assert not U.engaged(kernels, U.FORWARD_ENGAGED[form]), (case, form, U.engaged(kernels, U.FORWARD_ENGAGED[form]))
    if case in U.FORWARD_DIFFERS.get(form, ()):
        if case not in _default_forward:
            _default_forward[case] = U.device_forward(case)
        assert not np.array_equal(y, _default_forward[case]), f"{form} gives the default's bits on case {case}: it did not engage"
    _hold(case, U.device_errors(case, y, None), record_property)


@pytest.mark.parametrize("form", [f"{n}={v}" for n, v in U.TRAINING_FORMS])
@pytest.mark.parametrize("case", U.TRAINING_FORM_CASES)
def test_training_forms(case, form, record_property):
    name, value = form.split("=")
    kernels = {}
    with U.forced(name, value):
        step = U.device_step(case, kernels=kernels)
    record_property("kernels", kernels)
    if form in U.TRAINING_ENGAGED:
        assert not U.engaged(kernels, U.TRAINING_ENGAGED[form]), (case, form, U.engaged(kernels, U.TRAINING_ENGAGED[form]))
    _hold(case, U.device_errors(case, None, step), record_property)
