"""GPU: the DPM-Solver++ multistep update in the stand-alone kernel (k_sampler_multistep) and in the output
head's launch (k_out_head_px_ms), the loops built on it, the chains and the CLI.

The update is held to its definition evaluated op by op in fp32 on the CPU,
    s = (cx * x_t) + (c0 * x0);   order 2: s = s + (c1 * x0_prev);   with eps: s = s + (cn * eps)
with x0 the pred_xstart that the existing STEP_DDIM entry returns for the same (x, t): bit equality, no tolerance (a difference
means an operation was contracted or reordered).  Shapes: multistep_cases.CONFIGS (those of test_edit_gpu.py); the 256-channel
instantiation of the head is covered by test_multistep_resources.py only."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import multistep_cases as MC
from conftest import REPO, relerr
from sin3dm_amd import _lib
from sin3dm_amd import testing as T

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TRAJ_TOL = 2e-4             # the project's trajectory tolerance (README.md "Parity", tests/test_hip_parity.py)
CONFIGS = MC.CONFIGS


def make_model(mc, C=12, seed=0):
    from sin3dm_amd.diffusion.unet_triplane import TriplaneUNetModelSmall
    m = TriplaneUNetModelSmall(C, mc, C, use_scale_shift_norm=True)
    m.load_state_dict(T.synthetic_state_dict(T.unet_param_shapes(in_channels=C, model_channels=mc, out_channels=C), seed))
    return m.to(DEV).eval()


@functools.lru_cache(maxsize=None)
def diffusion(px=True, resp="logsnr20"):
    from sin3dm_amd.diffusion.script_util import create_gaussian_diffusion
    return create_gaussian_diffusion(steps=1000, noise_schedule="linear", predict_xstart=px, timestep_respacing=resp)


def noise(shape, seed):
    return torch.from_numpy(T.synthetic_noise(tuple(shape), seed)).to(DEV)


def ht(ti, B):
    from sin3dm_amd.diffusion.gaussian_diffusion import HostTimesteps
    return HostTimesteps(torch.full((B,), ti, device=DEV, dtype=torch.int64), (ti,) * B)


def ddim_step(diff, model, x, ti, hwd, clip=True):
    """The existing entry: the fused STEP_DDIM step, eta = 0 -> (sample, pred_xstart)."""
    H, W, D = hwd
    with torch.no_grad():
        s, p, _ = diff._step(_lib.STEP_DDIM, model, x, ht(ti, x.shape[0]), clip, None, dict(H=H, W=W, D=D), fuse=True, noise=None, eta=0.0)
    return s, p


def ms_step(diff, model, x, ti, hwd, tables, order=1, x0_prev=None, eps=None, clip=True, known=None, fuse=True, carry=0):
    H, W, D = hwd
    with torch.no_grad():
        return diff._multistep_step(model, x, ht(ti, x.shape[0]), clip, dict(H=H, W=W, D=D), order=order, x0_prev=x0_prev, noise=eps,
                                    carry=carry, known=known, fuse=fuse, tables=tables)


def expression_cpu(tab, ti, x, x0, order, x0_prev, eps):
    """The three-line definition, every product and sum its own fp32 torch operation on the CPU."""
    cx, c0, c1, cn = (tab[r, ti] for r in range(4))
    x, x0 = x.cpu(), x0.cpu()
    s = (cx * x) + (c0 * x0)
    if order == 2:
        s = s + (c1 * x0_prev.cpu())
    if eps is not None:
        s = s + (cn * eps.cpu())
    return s


def inputs(cfg):
    mc, C, B, hwd = CONFIGS[cfg]
    H, W, D = hwd
    shape = (B, C, H + D, W + D)
    return mc, C, B, hwd, shape


def test_device_tables_are_casts_of_float64_values():
    d = diffusion()
    for order, sde in ((1, False), (2, False), (2, True)):
        img, orders = d._multistep_tables(torch.device(DEV), order, sde)
        tab, exp_orders = d.multistep_tables(order, sde)
        assert img.device == torch.device(DEV) and np.array_equal(img.cpu().numpy(), tab.astype(np.float32)) and np.array_equal(orders, exp_orders)


@pytest.mark.parametrize("cfg", sorted(CONFIGS))
def test_update_is_the_three_line_expression_bit_for_bit(cfg):
    mc, C, B, hwd, shape = inputs(cfg)
    model = make_model(mc, C)
    x, eps, xp = noise(shape, 1), noise(shape, 2), noise(shape, 3).clamp(-1, 1)
    n = 0
    for px in (True, False):
        diff = diffusion(px)
        own = diff._multistep_tables(torch.device(DEV), 2, True)[0]            # the schedule's own (the SDE rows: cn != 0 above index 0)
        synth = torch.from_numpy(MC.synthetic_tables(diff.num_timesteps)).to(DEV)
        for tables in (own, synth):
            tab_cpu = tables.cpu()
            for clip in (True, False):
                for ti in (19, 10, 1, 0):                                   # T - 1, a middle one, 1 and 0 of logsnr20
                    _, x0 = ddim_step(diff, model, x, ti, hwd, clip)
                    for order in (1, 2):
                        for e in (None, eps):
                            s, p = ms_step(diff, model, x, ti, hwd, tables, order=order, x0_prev=xp if order == 2 else None, eps=e, clip=clip)
                            assert torch.equal(p, x0), (cfg, px, clip, ti, order, e is not None, "pred_xstart")
                            exp = expression_cpu(tab_cpu, ti, x, x0, order, xp, e)
                            got = s.cpu()
                            assert torch.equal(got, exp), (cfg, px, clip, ti, order, e is not None, float((got - exp).abs().max()))
                            n += 1
    assert n == 128


@pytest.mark.parametrize("cfg", sorted(CONFIGS))
def test_fused_equals_forward_then_the_stand_alone_kernel(cfg):
    mc, C, B, hwd, shape = inputs(cfg)
    model, diff = make_model(mc, C), diffusion()
    x, eps, xp = noise(shape, 1), noise(shape, 2), noise(shape, 3).clamp(-1, 1)
    synth = torch.from_numpy(MC.synthetic_tables(diff.num_timesteps)).to(DEV)
    for ti in (19, 7, 0):
        for order in (1, 2):
            for e in (None, eps):
                kw = dict(order=order, x0_prev=xp if order == 2 else None, eps=e)
                ref = ms_step(diff, model, x, ti, hwd, synth, fuse=False, **kw)          # forward + s3d_sampler_step_multistep
                for carry in (0, _lib.CARRY_OUT):
                    got = ms_step(diff, model, x, ti, hwd, synth, fuse=True, carry=carry, **kw)
                    assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1]), (cfg, ti, order, e is not None, carry)


@pytest.mark.parametrize("cfg", ["fused_odd", "fused_tail", "fused_geo", "fused_cq32"])
def test_carried_step_equals_the_same_step_without_carry(cfg):
    mc, C, B, hwd, shape = inputs(cfg)
    diff = diffusion()
    x, eps = noise(shape, 1), noise(shape, 2)
    tables = diff._multistep_tables(torch.device(DEV), 2, True)[0]
    plain = make_model(mc, C)
    r1 = ms_step(diff, plain, x, 10, hwd, tables, order=1, eps=eps)
    r2 = ms_step(diff, plain, r1[0], 9, hwd, tables, order=2, x0_prev=r1[1], eps=eps)
    model = make_model(mc, C)
    assert model.carries_in_conv
    g1 = ms_step(diff, model, x, 10, hwd, tables, order=1, eps=eps, carry=_lib.CARRY_OUT)
    g2 = ms_step(diff, model, g1[0], 9, hwd, tables, order=2, x0_prev=g1[1], eps=eps, carry=_lib.CARRY_IN | _lib.CARRY_OUT)
    g3 = ms_step(diff, model, g2[0], 8, hwd, tables, order=2, x0_prev=g2[1], eps=eps, carry=_lib.CARRY_IN)
    r3 = ms_step(diff, plain, r2[0], 8, hwd, tables, order=2, x0_prev=r2[1], eps=eps)
    for g, r in ((g1, r1), (g2, r2), (g3, r3)):
        assert torch.isfinite(g[0]).all() and torch.equal(g[0], r[0]) and torch.equal(g[1], r[1])


@pytest.mark.parametrize("cfg", ["standalone32", "fused_odd", "fused_tail"])
def test_known_region_is_the_blend_of_the_plain_sample(cfg):
    from test_edit_gpu import blend_cpu, masks
    mc, C, B, hwd, shape = inputs(cfg)
    model, diff = make_model(mc, C), diffusion()
    x, eps, xp, y0, ek = noise(shape, 1), noise(shape, 2), noise(shape, 3).clamp(-1, 1), noise(shape, 4).clamp(-1, 1), noise(shape, 5)
    synth = torch.from_numpy(MC.synthetic_tables(diff.num_timesteps)).to(DEV)
    for name, m in masks(shape, hwd).items():
        for ti in (19, 7, 0):
            for order, e in ((1, None), (2, eps)):
                kw = dict(order=order, x0_prev=xp if order == 2 else None, eps=e)
                plain_s, plain_p = ms_step(diff, model, x, ti, hwd, synth, **kw)
                s, p = ms_step(diff, model, x, ti, hwd, synth, known=(y0, m, ek), **kw)
                assert torch.equal(p, plain_p), (cfg, name, ti, order)
                assert torch.equal(s.cpu(), blend_cpu(diff, ti, plain_s, y0, m, ek)), (cfg, name, ti, order)


# ------------------------------------------------------------------ loops
class Recorded:
    """A noise_fn that hands out prepared tensors in order."""

    def __init__(self, shape, n, seed=100):
        self.t = [noise(shape, seed + k) for k in range(n)]
        self.k = 0

    def __call__(self, like):
        self.k += 1
        return self.t[self.k - 1]


def port_loop(diff, sd, xT, hwd, mc, order, sde, draws):
    """The same loop in torch on the CPU port's UNet (oracle/torch_port.py), float32, coefficients = the fp32 casts of multistep_tables."""
    import torch_port as tp
    H, W, D = hwd
    tab64, orders = diff.multistep_tables(order, sde)
    tab = torch.from_numpy(tab64.astype(np.float32))
    x, x0_prev = xT.cpu(), None
    B = x.shape[0]
    with torch.no_grad():
        for i in range(diff.num_timesteps - 1, -1, -1):
            mo = tp.unet_forward(sd, x, torch.full((B,), float(diff.timestep_map[i])), H, W, D, mc)
            x0 = mo.clamp(-1, 1)
            s = tab[0, i] * x + tab[1, i] * x0
            if orders[i] == 2:
                s = s + tab[2, i] * x0_prev
            if sde:
                s = s + tab[3, i] * next(draws)
            x, x0_prev = s, x0
    return x


@pytest.mark.parametrize("sampler,resp", [("dpmpp2m", "logsnr10"), ("dpmpp2m_sde", "20")])
def test_loop_against_the_cpu_port(oracle, sampler, resp):
    from sin3dm_amd.diffusion.gaussian_diffusion import multistep_sampler
    mc, C, B, hwd = 32, 12, 2, (10, 14, 6)
    H, W, D = hwd
    shape = (B, C, H + D, W + D)
    order, sde = multistep_sampler(sampler)
    diff = diffusion(True, resp)
    xT = noise(shape, 7)
    rec = Recorded(shape, diff.num_timesteps if sde else 0)
    model = make_model(mc, C)
    diff.noise_fn = rec
    try:
        got = diff.multistep_sample_loop(model, shape, order=order, sde=sde, noise=xT, model_kwargs=dict(H=H, W=W, D=D))
    finally:
        diff.noise_fn = None
    assert rec.k == (diff.num_timesteps if sde else 0)                  # the ODE form draws nothing after x_T
    sd = T.synthetic_state_dict(T.unet_param_shapes(model_channels=mc), 0)
    exp = port_loop(diff, sd, xT, hwd, mc, order, sde, iter(t.cpu() for t in rec.t))
    err = relerr(got.cpu().numpy(), exp.numpy())
    print(f"{sampler} at {resp} vs CPU port: relerr {err:.3e}")
    assert err <= TRAJ_TOL


@pytest.mark.parametrize("cfg", ["standalone32", "fused_odd"])
def test_dpmpp1_is_ddim_eta0(cfg):
    """Equal algebraically, rounded differently: the trajectory tolerance."""
    mc, C, B, hwd, shape = inputs(cfg)
    H, W, D = hwd
    diff, model = diffusion(True, "logsnr10"), make_model(mc, C)
    xT = noise(shape, 7)
    kw = dict(noise=xT, model_kwargs=dict(H=H, W=W, D=D))
    got = diff.multistep_sample_loop(model, shape, order=1, **kw)
    ref = diff.ddim_sample_loop(model, shape, eta=0.0, **kw)
    err = relerr(got.cpu().numpy(), ref.cpu().numpy())
    print(f"dpmpp1 vs ddim eta 0 ({cfg}): relerr {err:.3e}")
    assert err <= TRAJ_TOL


def test_loop_history_orders_and_draws():
    """The progressive loop: one dict per kept step, order 2 between the ends (the second step differs from an order-1 run, the first
    does not), the SDE form draws one eps per step and with a known region one more."""
    from sin3dm_amd.diffusion.gaussian_diffusion import KnownRegion
    from test_edit_gpu import masks
    mc, C, B, hwd, shape = inputs("fused_odd")
    H, W, D = hwd
    diff, model = diffusion(True, "logsnr10"), make_model(mc, C)
    kw = dict(noise=noise(shape, 7), model_kwargs=dict(H=H, W=W, D=D))
    two = [(o["sample"], o["pred_xstart"]) for o in diff.multistep_sample_loop_progressive(model, shape, order=2, **kw)]
    one = [(o["sample"], o["pred_xstart"]) for o in diff.multistep_sample_loop_progressive(model, shape, order=1, **kw)]
    assert len(two) == len(one) == 10
    assert torch.equal(two[0][0], one[0][0]) and not torch.equal(two[1][0], one[1][0])
    assert torch.equal(two[-1][0], two[-1][1])                          # index 0 returns the model's (clamped) x0
    known = KnownRegion(noise(shape[1:], 3).clamp(-1, 1), masks(shape, hwd)["hard"][0])
    for sde, kn, n in ((False, None, 0), (True, None, 10), (False, known, 10), (True, known, 20)):
        rec = Recorded(shape, n)
        diff.noise_fn = rec
        try:
            out = diff.multistep_sample_loop(model, shape, order=2, sde=sde, known=kn, **kw)
        finally:
            diff.noise_fn = None
        assert rec.k == n and torch.isfinite(out).all()
        if kn is not None:
            keep = (kn.mask == 1)[None].expand(shape)
            assert torch.equal(out[keep], kn.y0[None].expand(shape)[keep])           # where the mask is 1 the final sample IS y0


def test_carried_loop_equals_uncarried():
    from test_edit_gpu import poison
    mc, C, B, hwd, shape = inputs("fused_odd")
    H, W, D = hwd
    diff = diffusion(True, "logsnr10")
    runs = []
    for carry_on in (True, False):
        model = make_model(mc, C)
        model.carries_in_conv = carry_on
        poison(model, B + 1, C, tuple(v + 2 for v in hwd))
        poison(model, B, C, hwd)
        runs.append([(o["sample"].clone(), o["pred_xstart"].clone())
                     for o in diff.multistep_sample_loop_progressive(model, shape, order=2, noise=noise(shape, 7), model_kwargs=dict(H=H, W=W, D=D))])
    for k, ((s1, p1), (s0, p0)) in enumerate(zip(*runs)):
        assert torch.isfinite(s1).all() and torch.equal(s1, s0) and torch.equal(p1, p0), k


def test_two_chains_equal_the_serial_runs():
    mc, C, hwd = 64, 12, (12, 9, 7)
    H, W, D = hwd
    one = (1, C, H + D, W + D)
    diff, model = diffusion(True, "logsnr10"), make_model(mc, C)
    kw = dict(model_kwargs=dict(H=H, W=W, D=D))
    gen = lambda s: torch.Generator(device=DEV).manual_seed(s)
    for sampler, order, sde in (("dpmpp2m", 2, False), ("dpmpp2m_sde", 2, True)):
        alone = [diff.multistep_sample_loop(model, one, order=order, sde=sde, generator=[gen(s)], **kw) for s in (11, 12, 13)]
        chains = diff.sample_loop_chains(model, one, 3, chains=2, generators=[[gen(s)] for s in (11, 12, 13)], device=DEV, sampler=sampler, **kw)
        torch.cuda.synchronize()
        for a, c in zip(alone, chains):
            assert torch.equal(a, c), sampler
        assert not torch.equal(alone[0], alone[1])


def test_sample_cli_with_a_multistep_sampler(tmp_path):
    from test_cli_gpu import make_experiment
    tag = make_experiment(str(tmp_path), hwd=(12, 16, 10), mc=32)
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""), S3D_SAMPLER="dpmpp2m")
    r = subprocess.run([sys.executable, "-m", "sin3dm_amd.sample", "--tag", tag, "--n_samples", "2", "--timestep_respacing", "logsnr10", "--vox",
                        "--reso", "16", "--output", "few"], capture_output=True, text=True, timeout=600, env=env, cwd=REPO)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "sampler dpmpp2m: 10 model evaluations per sample" in r.stdout
    feats = [np.load(os.path.join(tag, "few", f"{i:03d}", "feat.npz")) for i in range(2)]
    for d in feats:
        assert d["feat_xy"].shape == (12, 12, 16) and all(np.isfinite(d[k]).all() for k in d.files)
    assert not np.array_equal(feats[0]["feat_xy"], feats[1]["feat_xy"])
    assert all(os.path.exists(os.path.join(tag, "few", f"{i:03d}", "r16_voxel.npz")) for i in range(2))
