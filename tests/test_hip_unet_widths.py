"""The diffusion stage at latent widths other than 12 on the MI355X (tests/unet_f64_cases.py: the W cases; the forward and the
training step of every one of them are held to float64 in tests/test_hip_unet_f64.py).

1. One fused sampler step per width against float64.  tests/test_hip_parity.py compares the fused step and the carried in_conv
   with the unfused forms of the same device; this anchors them once per width: the DDPM and the DDIM (eta = 0) update of
   U.step_reference, error measure and bound of the forward (err_dev <= K_FWD * max(err_port32, 2^-23)).  The DDIM bound is wide at
   t = 1: the float32 reference itself is off by 1.1e-4 there, because the update's coefficients are the float64 tables rounded
   to float32 (sqrt(1 - alphas_cumprod_prev) from a float32 0.9999 carries 1.5e-4) and the synthetic model's x0 prediction is far
   from x_t, so that coefficient multiplies an eps of order 100.  The DDPM update and pred_xstart have no such term
   (port: 5.5e-7 to 1.8e-6).
2. A width the training kernels do not take (k_small_outer's register arrays, kSmallMaxS = 12) is refused when the flat
   parameter vector is attached, before any launch, and leaves the handle and the process as they were.
3. Three optimizer steps at width 4, the sdf latent, against the port in float64."""
import numpy as np
import pytest
import torch

import unet_f64_cases as U
from sin3dm_amd import testing as T

pytestmark = pytest.mark.gpu

K_FWD = 4                                       # tests/test_hip_unet_f64.py


@pytest.fixture(scope="module", autouse=True)
def _port_on_path(oracle):
    yield


# ------------------------------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize("mode", U.STEP_MODES)
@pytest.mark.parametrize("case", U.STEP_CASES)
def test_fused_step_against_float64(case, mode, record_property):
    ref = U.step_reference(case)[mode]
    H, W, D = U.CASES[case]["hwd"]
    sample, pred = U.device_fused_step(case, mode)
    dev = U.step_errors(case, mode, sample, pred)
    prt = U.step_errors(case, mode, *ref["f32"])
    record_property("errors", {"device": dev, "port32": prt})
    print(case, mode, {n: f"{d[0]:.2e} / {p[0]:.2e} = {d[0] / max(p[0], U.EPS32):.2f}" for n, d, p in zip(("sample", "pred_xstart"), dev, prt)})
    assert np.abs(ref["f64"][0][..., H:, W:]).max() > 0.5, "the corner of x_{t-1} is not a trivial one"
    for name, d, p in zip(("sample", "pred_xstart"), dev, prt):
        assert d[0] <= K_FWD * max(p[0], U.EPS32), (case, mode, name, d, p)


# ------------------------------------------------------------------------------------------------------------------ 2
def test_untrainable_width_is_refused_at_attach_and_leaves_everything_as_it_was():
    """W16 (inference serves it in its fast forms): training_losses_and_grads and the autograd path raise at the attach; the same
    model's inference forward then gives a fresh model's bits, and a width-12 training step gives the same bits before and after."""
    case = "W16"
    c = U.CASES[case]
    H, W, D = c["hwd"]
    dev = torch.device("cuda:0")
    before = U.device_step("Be")
    fresh = U.device_forward(case)
    m = U.device_model(case)
    diffusion = U.device_diffusion(case)
    x0, noise, t, w = (v.to(dev) for v in U.inputs(case))
    kw = dict(H=H, W=W, D=D)
    with pytest.raises(NotImplementedError, match=c["train_refused"]):
        diffusion.training_losses_and_grads(m, x0, t, w, kw, noise=noise)
    with pytest.raises(NotImplementedError, match=c["train_refused"]):
        terms = diffusion.training_losses(m, x0, t, model_kwargs=kw, noise=noise)
        (terms["loss"] * w).mean().backward()
    assert m._flat is None and all(p.grad is None for p in m.parameters())
    x_t = torch.from_numpy(U.port(case, False)["x_t"].copy()).to(dev)
    with torch.no_grad():
        y = m.eval()(x_t, t, H=H, W=W, D=D)
    assert torch.equal(y.cpu(), torch.from_numpy(fresh))
    after = U.device_step("Be")
    for a, b in zip(before, after):
        assert sorted(a) == sorted(b) and all(np.array_equal(a[k], b[k]) for k in a)


# ------------------------------------------------------------------------------------------------------------------ 3
TRAIN_FULL = ("input_blocks.0.0.in_layers.2.conv_xy.weight",)        # tests/golden/make_golden.py: the tensors a digest stores whole


class _Digest(dict):
    files = property(lambda self: list(self))


def _digest(named, prefix, out, full_max, full_names=()):
    """tests/golden/make_golden.py:grad_digest of float64 arrays, in the layout conftest.digest_errors reads."""
    norms, projs, heads = [], [], []
    for k, a in named.items():
        a = np.asarray(a, np.float64).reshape(-1)
        r = T.synthetic_tensor("digest/" + k, (a.size,), 7).astype(np.float64)
        norms.append(float(np.linalg.norm(a)))
        projs.append(float(a @ r))
        heads.append(np.pad(a[:8], (0, max(0, 8 - a.size))))
        if a.size <= full_max or k in full_names:
            out[f"{prefix}/full/{k}"] = a
    out[f"{prefix}/names"] = np.asarray(list(named))
    out[f"{prefix}/norm"], out[f"{prefix}/proj"], out[f"{prefix}/head"] = np.asarray(norms), np.asarray(projs), np.stack(heads)


STEP_T = ([700, 3], [12, 999], [450, 451])       # tests/test_hip_train.py:test_optimizer_steps, as its seeds and hyper-parameters
LR0, EMA_RATE, ANNEAL = 5e-4, 0.99, 10


def _port_steps(ch, mc, hwd, B, wd):
    """Three TrainLoop.run_step iterations of the port in float64: (losses [3][B], dparam, dema, zero-gradient names)."""
    orc, tp = U._port_modules()
    H, W, D = hwd
    sd0 = T.synthetic_state_dict(T.unet_param_shapes(in_channels=ch, model_channels=mc, out_channels=ch), 0)
    names = list(sd0)
    params = [sd0[k].double().clone() for k in names]
    m, v, ema = [torch.zeros_like(p) for p in params], [torch.zeros_like(p) for p in params], [p.clone() for p in params]
    x0 = torch.from_numpy(T.synthetic_noise((B, ch, H + D, W + D), 400)).clamp(-1, 1).double()
    tabs = orc.schedule_tables_named(1000)
    lr, losses, skip = LR0, [], set()
    n = torch.get_num_threads()
    torch.set_num_threads(min(16, n))
    try:
        for step in range(3):
            noise = torch.from_numpy(T.synthetic_noise((B, ch, H + D, W + D), 500 + step)).double()
            sd = {k: p.clone().requires_grad_(True) for k, p in zip(names, params)}
            terms, _ = tp.training_losses(sd, x0, torch.tensor(STEP_T[step]), noise, tabs, H, W, D, weights=torch.ones(B), model_channels=mc)
            grads = torch.autograd.grad(terms["objective"], [sd[k] for k in names])
            if step == 0:                                             # conftest.zero_grad_params' rule
                gn = [float(g.norm()) for g in grads]
                skip = {k for k, x in zip(names, gn) if x < 1e-6 * max(gn)}
            with torch.no_grad():
                tp.adamw_ema_step(params, grads, m, v, ema, step + 1, lr, wd, EMA_RATE)
            lr = LR0 * (1 - step / ANNEAL)
            losses.append(terms["loss"].detach().numpy())
    finally:
        torch.set_num_threads(n)
    return (losses, {k: (p - sd0[k].double()).numpy() for k, p in zip(names, params)},
            {k: (e - sd0[k].double()).numpy() for k, e in zip(names, ema)}, skip)


@pytest.mark.parametrize("wd", [0.0, 0.01], ids=["wd0", "wd01"])
def test_three_optimizer_steps_at_width_4(wd):
    """test_optimizer_steps at the sdf width: FlatAdamW (AdamW -> EMA -> linear anneal) at mc 32, (10, 14, 6), batch 2 against
    torch_port.training_losses + adamw_ema_step in float64, in conftest.digest_errors' measures and under test_optimizer_steps'
    thresholds (its comment says why they are not tighter: a gradient element within round-off of zero flips a whole +-lr step).
    Measured on an MI355X (wd0 / wd01): dparam norm 4.5e-5 / 2.9e-5, proj 3.5e-3 / 3.5e-3, full_l2 1.9e-4 / 1.9e-4; dema norm
    1.2e-3 / 1.1e-3, proj 8.5e-3 / 6.7e-3; the losses of the three steps within 1.5e-6 of float64 (bound 2e-4, as there)."""
    from conftest import digest_errors, relerr
    from sin3dm_amd.diffusion.train_util import FlatAdamW
    from sin3dm_amd.diffusion.unet_triplane import TriplaneUNetModelSmall
    ch, mc, B, (H, W, D) = 4, 32, 2, (10, 14, 6)
    losses64, dparam64, dema64, skip = _port_steps(ch, mc, (H, W, D), B, wd)
    assert len(skip) == 12, sorted(skip)
    g = _Digest()
    _digest(dparam64, "dparam", g, 512, TRAIN_FULL)
    _digest(dema64, "dema", g, 64)
    dev = torch.device("cuda:0")
    m = TriplaneUNetModelSmall(ch, mc, ch, use_scale_shift_norm=True)
    m.load_state_dict(T.synthetic_state_dict(T.unet_param_shapes(in_channels=ch, model_channels=mc, out_channels=ch), 0))
    m.to(dev)
    diffusion = U.device_diffusion("W4n")
    init = {k: v.detach().clone() for k, v in m.named_parameters()}
    opt = FlatAdamW(m, lr=LR0, weight_decay=wd, ema_rates=[EMA_RATE])
    x0 = torch.from_numpy(T.synthetic_noise((B, ch, H + D, W + D), 400)).clamp(-1, 1).to(dev)
    worst_loss = 0.0
    for step in range(3):
        noise = torch.from_numpy(T.synthetic_noise((B, ch, H + D, W + D), 500 + step)).to(dev)
        terms, grads = diffusion.training_losses_and_grads(m, x0, torch.tensor(STEP_T[step], device=dev), torch.ones(B, device=dev),
                                                           dict(H=H, W=W, D=D), noise=noise)
        worst_loss = max(worst_loss, relerr(terms["loss"].cpu().numpy(), losses64[step]))
        opt.step(grads)
        opt.lr = LR0 * (1 - step / ANNEAL)
    dparam = {k: (p.detach() - init[k]).cpu().numpy() for k, p in m.named_parameters()}
    dema = {k: (v - init[k]).cpu().numpy() for k, v in m.split_flat(opt.ema[0]).items()}
    wp, we = digest_errors(dparam, g, "dparam", skip), digest_errors(dema, g, "dema", skip)
    print("width 4, three steps:", wd, "losses", f"{worst_loss:.2e}", "dparam", wp, "dema", we)
    assert worst_loss < 2e-4, worst_loss
    assert wp["norm"] < 5e-3 and wp["proj"] < 3e-2 and wp["full_l2"] < 3e-2, wp
    assert we["norm"] < 5e-3 and we["proj"] < 3e-2, we
