"""GPU: known-region sampling (outpainting / local editing) — the blend in the stand-alone sampler kernel and
in the output head's launch, the re-noise kernel, the loops with `known=` / `resample=`, and the edit CLI.

The blend is held to its two-line definition evaluated op by op in fp32 on the CPU,
    k = (sa[i] * y0) + (sb[i] * ek);   sample = (m * k) + ((1 - m) * plain)
with `plain` the existing entry point's sample: bit equality, no tolerance (a difference means an operation was contracted)."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import REPO, relerr
from sin3dm_amd import _lib
from sin3dm_amd import testing as T

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TRAJ_TOL = 2e-4             # the project's trajectory tolerance (README.md "Parity", tests/test_hip_parity.py)


def head_blocks(hwd):
    """Blocks per sample of the pixel-chunk output head: 64-pixel segments of every line of the three planes."""
    H, W, D = hwd
    seg = lambda n: (n + 63) // 64
    return H * seg(W) + H * seg(D) + D * seg(W)


def corner_tail_runs(hwd, cout):
    """The head's corner tail loop runs when the D x D corner has more elements than two per thread of the launch's blocks."""
    return cout * hwd[2] ** 2 > 512 * head_blocks(hwd)


S_TAIL = (2, 2, 47)         # the smallest shape the UNet accepts (H = W = 2: one pooling) whose corner reaches the tail loop at Cout = 12
# (mc, latent channels, B, hwd): the stand-alone path; fused, odd sizes, line tails shorter than 64; the corner tail loop; geometry only
CONFIGS = {"standalone32": (32, 12, 2, (10, 14, 6)), "fused_odd": (64, 12, 1, (12, 9, 7)), "fused_tail": (64, 12, 2, S_TAIL),
           "fused_geo": (64, 4, 2, (12, 9, 7)), "standalone_geo": (32, 4, 1, (10, 14, 6))}


def test_shapes_reach_the_paths_they_are_there_for():
    assert corner_tail_runs(S_TAIL, 12) and not corner_tail_runs((2, 2, 46), 12)
    assert not corner_tail_runs((12, 9, 7), 12) and not corner_tail_runs((10, 14, 6), 12)


def make_model(mc, C=12, seed=0):
    from sin3dm_amd.diffusion.unet_triplane import TriplaneUNetModelSmall
    m = TriplaneUNetModelSmall(C, mc, C, use_scale_shift_norm=True)
    m.load_state_dict(T.synthetic_state_dict(T.unet_param_shapes(in_channels=C, model_channels=mc, out_channels=C), seed))
    return m.to(DEV).eval()


@functools.lru_cache(maxsize=None)
def diffusion(px=True, resp="20"):
    from sin3dm_amd.diffusion.script_util import create_gaussian_diffusion
    return create_gaussian_diffusion(steps=1000, noise_schedule="linear", predict_xstart=px, timestep_respacing=resp)


def noise(shape, seed):
    return torch.from_numpy(T.synthetic_noise(tuple(shape), seed)).to(DEV)


def masks(shape, hwd):
    """hard (a box: rows of xy / xz and a patch of the corner), soft (0.25 / 0.75)"""
    H, W, D = hwd
    hard = torch.zeros(shape, device=DEV)
    hard[:, :, : max(H // 2, 1), :] = 1
    hard[:, :, H:, : max(W // 2, 1)] = 1
    hard[:, :, H + D // 2:, W + D // 3:] = 1
    soft = torch.where(noise(shape, 91) > 0, 0.75, 0.25).to(torch.float32)
    return {"hard": hard, "soft": soft}


def ht(ti, B):
    from sin3dm_amd.diffusion.gaussian_diffusion import HostTimesteps
    return HostTimesteps(torch.full((B,), ti, device=DEV, dtype=torch.int64), (ti,) * B)


def step(diff, model, mode, x, ti, eps, hwd, clip=True, eta=0.0, known=None, fuse=True, carry=0):
    H, W, D = hwd
    with torch.no_grad():
        s, p, _ = diff._step(mode, model, x, ht(ti, x.shape[0]), clip, None, dict(H=H, W=W, D=D), fuse=fuse, noise=eps, eta=eta,
                             known=known, carry=carry)
    return s, p


def blend_cpu(diff, ti, plain, y0, m, ek):
    tab = diff._known_tables(torch.device(DEV)).cpu()
    sa, sb = tab[0, ti], tab[1, ti]
    plain, y0, m, ek = (v.cpu() for v in (plain, y0, m, ek))
    k = (sa * y0) + (sb * ek)
    return (m * k) + ((1 - m) * plain)


def test_known_tables_are_casts_of_float64_values():
    d = diffusion()
    tab = d._known_tables(torch.device(DEV)).cpu().numpy()
    exp = np.stack([np.sqrt(d.alphas_cumprod_prev), np.sqrt(1 - d.alphas_cumprod_prev), np.sqrt(1 - d.betas), np.sqrt(d.betas)])
    assert tab.shape == (4, 20) and np.array_equal(tab, exp.astype(np.float32))
    assert tab[0, 0] == 1.0 and tab[1, 0] == 0.0


@pytest.mark.parametrize("cfg", sorted(CONFIGS))
def test_blend_is_the_two_line_expression_bit_for_bit(cfg):
    mc, C, B, hwd = CONFIGS[cfg]
    H, W, D = hwd
    shape = (B, C, H + D, W + D)
    model = make_model(mc, C)
    x, eps, y0, ek = noise(shape, 1), noise(shape, 2), noise(shape, 3).clamp(-1, 1), noise(shape, 4)
    ms = masks(shape, hwd)
    n = 0
    for px in (True, False):
        diff = diffusion(px)
        for mode, eta in ((_lib.STEP_DDPM, 0.0), (_lib.STEP_DDIM, 0.0), (_lib.STEP_DDIM, 0.5)):
            for clip in (True, False):
                for ti in (19, 10, 0):
                    plain_s, plain_p = step(diff, model, mode, x, ti, eps, hwd, clip, eta)
                    for name, m in ms.items():
                        s, p = step(diff, model, mode, x, ti, eps, hwd, clip, eta, known=(y0, m, ek))
                        assert torch.equal(p, plain_p), (cfg, px, mode, eta, clip, ti, name, "pred_xstart")
                        exp = blend_cpu(diff, ti, plain_s, y0, m, ek)
                        got = s.cpu()
                        assert torch.equal(got, exp), (cfg, px, mode, eta, clip, ti, name, float((got - exp).abs().max()))
                        n += 1
    assert n == 72


@pytest.mark.parametrize("cfg", ["standalone32", "fused_odd", "fused_tail"])
def test_limits(cfg):
    mc, C, B, hwd = CONFIGS[cfg]
    H, W, D = hwd
    shape = (B, C, H + D, W + D)
    model, diff = make_model(mc, C), diffusion()
    x, eps, y0, ek = noise(shape, 1), noise(shape, 2), noise(shape, 3).clamp(-1, 1), noise(shape, 4)
    zeros, ones = torch.zeros(shape, device=DEV), torch.ones(shape, device=DEV)
    for ti in (19, 10, 0):
        plain_s, _ = step(diff, model, _lib.STEP_DDPM, x, ti, eps, hwd)
        s, _ = step(diff, model, _lib.STEP_DDPM, x, ti, eps, hwd, known=(y0, zeros, ek))
        assert torch.equal(s, plain_s), ti                              # mask 0 everywhere: the plain step
    s, _ = step(diff, model, _lib.STEP_DDPM, x, 0, eps, hwd, known=(y0, ones, ek))
    assert torch.equal(s, y0)                                           # mask 1 everywhere at i = 0: y0
    corner = zeros.clone()
    corner[..., H:, W:] = 1
    plain_s, _ = step(diff, model, _lib.STEP_DDPM, x, 0, eps, hwd)
    s, _ = step(diff, model, _lib.STEP_DDPM, x, 0, eps, hwd, known=(y0, corner, ek))
    assert torch.equal(s[..., H:, W:], y0[..., H:, W:])                 # mask 1 only inside the D x D corner: the corner takes y0
    out = corner == 0
    assert torch.equal(s[out], plain_s[out])
    plain_s, _ = step(diff, model, _lib.STEP_DDPM, x, 10, eps, hwd)
    s, _ = step(diff, model, _lib.STEP_DDPM, x, 10, eps, hwd, known=(y0, corner, ek))
    assert torch.equal(s.cpu(), blend_cpu(diff, 10, plain_s, y0, corner, ek))


@pytest.mark.parametrize("cfg", sorted(CONFIGS))
def test_fused_equals_forward_then_known_sampler_kernel(cfg):
    mc, C, B, hwd = CONFIGS[cfg]
    H, W, D = hwd
    shape = (B, C, H + D, W + D)
    model, diff = make_model(mc, C), diffusion()
    x, eps, y0, ek = noise(shape, 1), noise(shape, 2), noise(shape, 3).clamp(-1, 1), noise(shape, 4)
    for mode, eta in ((_lib.STEP_DDPM, 0.0), (_lib.STEP_DDIM, 0.5)):
        for name, m in masks(shape, hwd).items():
            for ti in (19, 0):
                ref = step(diff, model, mode, x, ti, eps, hwd, eta=eta, known=(y0, m, ek), fuse=False)      # s3d_unet_forward_film + s3d_sampler_step_known
                for carry in (0, _lib.CARRY_OUT):
                    got = step(diff, model, mode, x, ti, eps, hwd, eta=eta, known=(y0, m, ek), fuse=True, carry=carry)
                    assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1]), (cfg, mode, name, ti, carry)


class CallerBuffer:
    """The model's known-region step with a caller buffer for the model output (s3d_unet_step_film_known's `model_out`), which the
    module's own denoise_step never passes: the step then runs as output head + k_sampler_known."""
    carries_in_conv = True

    def __init__(self, model):
        self.model, self.buf = model, None

    def denoise_step(self, x, timesteps, step, H=None, W=None, D=None, carry=0, known=None):
        import ctypes as C
        m = self.model
        lib = m._ensure_handle()
        self.buf = torch.empty_like(x)
        t = timesteps.to(device=x.device, dtype=torch.float32).contiguous()
        with torch.cuda.device(x.device):
            film, stride = m._film_for(lib, timesteps.host_values, t)
            _lib.check(lib.s3d_unet_step_film_known(m._handle, _lib.ptr(film), stride, x.shape[0], int(H), int(W), int(D), C.byref(step),
                                                    C.byref(known), _lib.ptr(self.buf), _lib.stream_ptr(), int(carry)))


@pytest.mark.parametrize("cfg", ["standalone32", "fused_odd"])
def test_step_with_a_model_output_buffer(cfg):
    """model_out != NULL: the model output is stored, sample and pred_xstart are those of the in-head form, and a CARRY_OUT asked of
    such a step leaves nothing that the next step could take by mistake."""
    mc, C, B, hwd = CONFIGS[cfg]
    H, W, D = hwd
    shape = (B, C, H + D, W + D)
    model, diff = make_model(mc, C), diffusion()
    x, eps, y0, ek = noise(shape, 1), noise(shape, 2), noise(shape, 3).clamp(-1, 1), noise(shape, 4)
    m = masks(shape, hwd)["soft"]
    ref = step(diff, model, _lib.STEP_DDPM, x, 10, eps, hwd, known=(y0, m, ek))
    with torch.no_grad():
        mo = diff._wrap_model(model)(x, ht(10, B), H=H, W=W, D=D)        # (the step conditions on the ORIGINAL timestep of index 10)
    buf = CallerBuffer(model)
    got = step(diff, buf, _lib.STEP_DDPM, x, 10, eps, hwd, known=(y0, m, ek), carry=_lib.CARRY_OUT)
    assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1]) and torch.equal(buf.buf, mo)
    nxt_ref = step(diff, make_model(mc, C), _lib.STEP_DDPM, ref[0], 9, eps, hwd, known=(y0, m, ek))
    nxt = step(diff, model, _lib.STEP_DDPM, got[0], 9, eps, hwd, known=(y0, m, ek), carry=_lib.CARRY_IN)
    assert torch.equal(nxt[0], nxt_ref[0]) and torch.equal(nxt[1], nxt_ref[1])


def poison(model, B, C, hwd):
    """An all-NaN forward: every workspace buffer it touches holds NaN afterwards (tests/handle_sequences.py)."""
    H, W, D = hwd
    with torch.no_grad():
        y = model(torch.full((B, C, H + D, W + D), float("nan"), device=DEV), torch.full((B,), 5.0, device=DEV), H=H, W=W, D=D)
    assert bool(torch.isnan(y[..., :H, :]).all())


class Recorded:
    """A noise_fn that hands out prepared tensors in order."""

    def __init__(self, shape, n, seed=100):
        self.t = [noise(shape, seed + k) for k in range(n)]
        self.k = 0

    def __call__(self, like):
        self.k += 1
        return self.t[self.k - 1]


@pytest.mark.parametrize("cfg", ["fused_odd", "fused_geo"])
@pytest.mark.parametrize("resample", [1, 2])
def test_carried_loop_equals_uncarried(cfg, resample):
    mc, C, B, hwd = CONFIGS[cfg]
    B = 2
    H, W, D = hwd
    shape = (B, C, H + D, W + D)
    from sin3dm_amd.diffusion.gaussian_diffusion import KnownRegion
    diff = diffusion(True, "4")
    known = KnownRegion(noise(shape[1:], 3).clamp(-1, 1), masks(shape, hwd)["hard"][0])
    n_evals = 3 * resample + 1
    runs = []
    for carry_on in (True, False):
        model = make_model(mc, C)
        model.carries_in_conv = carry_on
        poison(model, B + 1, C, tuple(v + 2 for v in hwd))              # another, larger shape: the loop's workspace lies inside it
        poison(model, B, C, hwd)
        diff.noise_fn = Recorded(shape, 3 * n_evals)
        try:
            outs = [(o["sample"].clone(), o["pred_xstart"].clone())
                    for o in diff.p_sample_loop_progressive(model, shape, noise=noise(shape, 7), model_kwargs=dict(H=H, W=W, D=D),
                                                            known=known, resample=resample)]
        finally:
            diff.noise_fn = None
        assert len(outs) == n_evals
        runs.append(outs)
    for k, ((s1, p1), (s0, p0)) in enumerate(zip(*runs)):
        assert torch.isfinite(s1).all() and torch.isfinite(p1).all(), k
        assert torch.equal(s1, s0) and torch.equal(p1, p0), k


def test_renoise_kernel():
    diff = diffusion()
    shape = (3, 12, 9, 11)
    x, er = noise(shape, 1), noise(shape, 2)
    t = torch.tensor([19, 7, 0], device=DEV)
    got = diff.renoise(x, t, er).cpu()
    tab = diff._known_tables(torch.device(DEV)).cpu()
    a, b = tab[2][t.cpu()][:, None, None, None], tab[3][t.cpu()][:, None, None, None]
    assert torch.equal(got, (a * x.cpu()) + (b * er.cpu()))


def test_loop_against_the_cpu_port(oracle):
    """10-step DDPM, resample 2, hard box mask, every draw from a recorded noise_fn; against a restatement that drives the CPU
    port's UNet (oracle/torch_port.py) with the same tensors in float32."""
    import torch_port as tp
    from sin3dm_amd.diffusion.gaussian_diffusion import KnownRegion, known_region_schedule
    from sin3dm_amd.utils import region_util as R
    mc, C, B, hwd = 32, 12, 2, (10, 14, 6)
    H, W, D = hwd
    shape = (B, C, H + D, W + D)
    diff = diffusion(True, "10")
    src = tuple(torch.tanh(torch.from_numpy(T.synthetic_noise(s, k))) for k, s in enumerate(((C, H, W), (C, H, D), (C, W, D)), 1))
    y0, mask = R.build_known(src, hwd, [R.keep((0, 5, 0, 14, 0, 6))])
    xT = noise(shape, 7)
    evals = list(known_region_schedule(10, 2))
    n_draws = sum(2 + int(rn) for _, rn in evals)
    rec = Recorded(shape, n_draws)
    model = make_model(mc, C)
    diff.noise_fn = rec
    try:
        got = diff.p_sample_loop(model, shape, noise=xT, model_kwargs=dict(H=H, W=W, D=D), known=KnownRegion(y0, mask), resample=2)
    finally:
        diff.noise_fn = None
    assert rec.k == n_draws

    sd = T.synthetic_state_dict(T.unet_param_shapes(model_channels=mc), 0)
    tmap = diff.timestep_map
    f64 = lambda a: torch.from_numpy(np.asarray(a))
    c1, c2 = f64(diff.posterior_mean_coef1).float(), f64(diff.posterior_mean_coef2).float()
    _, logvar = diff._model_variance_tables()
    logvar = f64(logvar).float()
    ktab = torch.from_numpy(np.stack([np.sqrt(diff.alphas_cumprod_prev), np.sqrt(1 - diff.alphas_cumprod_prev), np.sqrt(1 - diff.betas),
                                      np.sqrt(diff.betas)]).astype(np.float32))
    y0b, mb = y0.cpu()[None].expand(shape), mask.cpu()[None].expand(shape)
    draws = iter(t.cpu() for t in rec.t)
    x = xT.cpu()
    with torch.no_grad():
        for i, rn in evals:
            eps, ek = next(draws), next(draws)
            mo = tp.unet_forward(sd, x, torch.full((B,), float(tmap[i])), H, W, D, mc)
            x0 = mo.clamp(-1, 1)
            mean = c1[i] * x0 + c2[i] * x
            plain = mean + (0.0 if i == 0 else 1.0) * torch.exp(0.5 * logvar[i]) * eps
            x = mb * (ktab[0, i] * y0b + ktab[1, i] * ek) + (1 - mb) * plain
            if rn:
                x = ktab[2, i] * x + ktab[3, i] * next(draws)
    err = relerr(got.cpu().numpy(), x.numpy())
    print("known-region loop vs CPU port: relerr", err)
    assert err < TRAJ_TOL
    keep = mb == 1
    assert bool(keep.any()) and torch.equal(got.cpu()[keep], y0b[keep])                 # where the mask is 1 the final sample IS y0


def test_determinism_of_chains_batches_and_cpu_stream_chunks():
    from sin3dm_amd.diffusion.cpu_stream import TorchCpuStream
    from sin3dm_amd.diffusion.gaussian_diffusion import KnownRegion
    mc, C, hwd = 64, 12, (12, 9, 7)
    H, W, D = hwd
    one = (1, C, H + D, W + D)
    diff = diffusion(True, "4")
    model = make_model(mc, C)
    known = KnownRegion(noise(one[1:], 3).clamp(-1, 1), masks(one, hwd)["hard"][0])
    kw = dict(model_kwargs=dict(H=H, W=W, D=D), known=known, resample=2)
    gen = lambda s: torch.Generator(device=DEV).manual_seed(s)
    alone = [diff.p_sample_loop(model, one, generator=[gen(s)], **kw) for s in (11, 12, 13)]
    chains = diff.sample_loop_chains(model, one, 3, chains=2, generators=[[gen(s)] for s in (11, 12, 13)], device=DEV, **kw)
    torch.cuda.synchronize()
    for a, c in zip(alone, chains):
        assert torch.equal(a, c)
    both = diff.p_sample_loop(model, (2,) + one[1:], generator=[gen(11), gen(12)], **kw)
    assert torch.equal(both[0:1], alone[0]) and torch.equal(both[1:2], alone[1])        # a sample does not depend on its batch
    a = diff.p_sample_loop(model, (2,) + one[1:], generator=TorchCpuStream(5, device=DEV), **kw)
    old = type(diff)._NOISE_AHEAD_BYTES
    try:
        type(diff)._NOISE_AHEAD_BYTES = 0
        b = diff.p_sample_loop(model, (2,) + one[1:], generator=TorchCpuStream(5, device=DEV), **kw)
    finally:
        type(diff)._NOISE_AHEAD_BYTES = old
    assert torch.equal(a, b)


def test_known_with_x0_replacement_is_refused():
    from sin3dm_amd.diffusion.gaussian_diffusion import KnownRegion
    mc, C, B, hwd = CONFIGS["standalone32"]
    H, W, D = hwd
    shape = (B, C, H + D, W + D)
    z = torch.zeros(shape, device=DEV)
    with pytest.raises(ValueError):
        diffusion().ddim_sample_loop(make_model(mc, C), shape, model_kwargs=dict(H=H, W=W, D=D), known=KnownRegion(z[0], z[0]), y0=z, mask=z)


def test_edit_cli_outpaint_and_keep_paste(tmp_path):
    from test_cli_gpu import make_experiment
    hwd = (12, 16, 10)
    tag = make_experiment(str(tmp_path), hwd=hwd, mc=32)
    src = np.load(os.path.join(tag, "encoding", "feat.npz"))
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
    common = ["--tag", tag, "--n_samples", "2", "--timestep_respacing", "5", "--vox", "--reso", "16"]

    def run(extra, out):
        r = subprocess.run([sys.executable, "-m", "sin3dm_amd.edit", *common, "--output", out, *extra], capture_output=True, text=True,
                           timeout=600, env=env, cwd=REPO)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        return [np.load(os.path.join(tag, out, f"{i:03d}", "feat.npz")) for i in range(2)]

    # grow y by half above: W 16 -> 24; xy and yz keep the source at offset 0, xz (no grown axis) stays free
    outs = run(["--outpaint", "0", "0", "0", "0.5", "0", "0", "--resample", "2"], "outpaint")
    for d in outs:
        assert d["feat_xy"].shape == (12, 12, 24) and d["feat_xz"].shape == (12, 12, 10) and d["feat_yz"].shape == (12, 24, 10)
        assert np.array_equal(d["feat_xy"][:, :, :16], src["feat_xy"]) and np.array_equal(d["feat_yz"][:, :16, :], src["feat_yz"])
        assert not np.array_equal(d["feat_xz"], src["feat_xz"]) and all(np.isfinite(d[k]).all() for k in d.files)
    assert not np.array_equal(outs[0]["feat_xy"][:, :, 16:], outs[1]["feat_xy"][:, :, 16:])
    assert os.path.exists(os.path.join(tag, "outpaint", "000", "r16_voxel.npz"))
    # keep the low-y quarter, paste it again at y = 0.75
    outs = run(["--keep", "0", "1", "0", "0.25", "0", "1", "--paste", "0", "1", "0", "0.25", "0", "1", "0", "0.75", "0"], "edit")
    for d in outs:
        assert d["feat_xy"].shape == (12, 12, 16)
        for k, ax in (("feat_xy", 2), ("feat_yz", 1)):
            a, s = np.moveaxis(d[k], ax, 0), np.moveaxis(src[k], ax, 0)
            assert np.array_equal(a[0:4], s[0:4]) and np.array_equal(a[12:16], s[0:4]), k
        assert np.array_equal(d["feat_xz"], src["feat_xz"])             # the box spans x and z: xz is kept whole
