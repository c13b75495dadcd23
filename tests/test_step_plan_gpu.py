"""GPU: whatever route a step's plan takes (plan_step, s3d_common.h) — the update in the output head's launch, or head + stand-alone
kernel; the next in_conv carried or launched — two consecutive steps give the bits of forward + stand-alone entry.  The existing
tests assert this piecewise (test_hip_parity.py, test_edit_gpu.py, test_multistep_gpu.py); here it runs over the whole grid of
requests at the smallest shapes that take both head forms: 64 channels (the pixel-chunk head) and 32 (k_out_head + stand-alone
kernel), one level, 8 x 8 x 4 planes, batch 2."""
import ctypes as C
import functools

import pytest
import torch

from sin3dm_amd import _lib
from sin3dm_amd import testing as T

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CH, B, HWD = 12, 2, (8, 8, 4)
SHAPE = (B, CH, HWD[0] + HWD[2], HWD[1] + HWD[2])
KW = dict(H=HWD[0], W=HWD[1], D=HWD[2])
T1, T2 = 10, 9                                       # two consecutive indices of the schedule
OUT, IN = _lib.CARRY_OUT, _lib.CARRY_IN


def make_model(mc):
    from sin3dm_amd.diffusion.unet_triplane import TriplaneUNetModelSmall
    m = TriplaneUNetModelSmall(CH, mc, CH, channel_mult=(1,), use_scale_shift_norm=True)
    m.load_state_dict(T.synthetic_state_dict(T.unet_param_shapes(in_channels=CH, model_channels=mc, out_channels=CH, channel_mult=(1,)), 0))
    return m.to(DEV).eval()


@functools.lru_cache(maxsize=None)
def diffusion():
    from sin3dm_amd.diffusion.script_util import create_gaussian_diffusion
    return create_gaussian_diffusion(steps=1000, noise_schedule="linear", predict_xstart=True, timestep_respacing="logsnr20")


def noise(seed):
    return torch.from_numpy(T.synthetic_noise(SHAPE, seed)).to(DEV)


def ht(ti):
    from sin3dm_amd.diffusion.gaussian_diffusion import HostTimesteps
    return HostTimesteps(torch.full((B,), ti, device=DEV, dtype=torch.int64), (ti,) * B)


class WithBuffer:
    """The model's one-call step with a caller buffer for the model output (`model_out` of the s3d_unet_step_film_* entries), which
    the module's own denoise_step never passes; `outs` keeps what each step stored."""
    carries_in_conv = True

    def __init__(self, model):
        self.model, self.outs = model, []

    def denoise_step(self, x, timesteps, step, H=None, W=None, D=None, carry=0, known=None, multistep=None):
        m = self.model
        lib = m._ensure_handle()
        self.outs.append(torch.empty_like(x))
        t = timesteps.to(device=x.device, dtype=torch.float32).contiguous()
        with torch.cuda.device(x.device):
            film, stride = m._film_for(lib, timesteps.host_values, t)
            head = (m._handle, _lib.ptr(film), stride, x.shape[0], int(H), int(W), int(D), C.byref(step))
            tail = (_lib.ptr(self.outs[-1]), _lib.stream_ptr(), int(carry))
            if multistep is not None:
                _lib.check(lib.s3d_unet_step_film_multistep(*head, C.byref(multistep), *tail))
            elif known is not None:
                _lib.check(lib.s3d_unet_step_film_known(*head, C.byref(known), *tail))
            else:
                _lib.check(lib.s3d_unet_step_film_carry(*head, *tail))


def two_steps(kind, model, fuse, carries=(0, 0)):
    """Two consecutive steps of `kind` on the module's inputs -> [sample 1, pred 1, sample 2, pred 2]."""
    diff = diffusion()
    x, eps, y0, mask, ek = noise(1), noise(2), noise(3).clamp(-1, 1), (noise(4) > 0).float(), noise(5)
    out, prev = [], None
    with torch.no_grad():
        for ti, carry in zip((T1, T2), carries):
            if kind == "multistep":
                tables = diff._multistep_tables(torch.device(DEV), 2, True)[0]
                s, p = diff._multistep_step(model, x, ht(ti), True, KW, order=1 if prev is None else 2, x0_prev=prev, noise=eps, carry=carry,
                                            fuse=fuse, tables=tables)
                prev = p
            else:
                s, p, _ = diff._step(_lib.STEP_DDPM, model, x, ht(ti), True, None, KW, fuse=fuse, noise=eps, carry=carry,
                                     known=(y0, mask, ek) if kind == "known" else None)
            out += [s, p]
            x = s
    return out


@functools.lru_cache(maxsize=None)
def reference(mc, kind):
    """forward + the stand-alone entry, twice: computed once per width and kind, shared by the cases below and left unchanged."""
    return tuple(two_steps(kind, make_model(mc), fuse=False))


def same(got, ref, what):
    for k, (g, r) in enumerate(zip(got, ref)):
        assert torch.equal(g, r), (what, ("sample 1", "pred_xstart 1", "sample 2", "pred_xstart 2")[k], float((g - r).abs().max()))


@pytest.mark.parametrize("kind", ["plain", "known", "multistep"])
@pytest.mark.parametrize("mc", [64, 32])
def test_two_steps_equal_forward_then_the_stand_alone_entry(mc, kind):
    ref = reference(mc, kind)
    assert all(bool(torch.isfinite(r).all()) for r in ref)
    same(two_steps(kind, make_model(mc), fuse=True), ref, (mc, kind, "one call per step"))
    # the next in_conv asked of the first step, then offered to the second or not: the second step's result does not depend on it
    for second in (IN, 0):
        same(two_steps(kind, make_model(mc), fuse=True, carries=(OUT, second)), ref, (mc, kind, "carry out, then in" if second else "carry out, not taken"))
    # ... and with a caller buffer for the model output (known, multistep: head + stand-alone kernel at either width)
    buf = WithBuffer(make_model(mc))
    same(two_steps(kind, buf, fuse=True, carries=(OUT, IN)), ref, (mc, kind, "model_out"))
    assert len(buf.outs) == 2
    with torch.no_grad():                                      # (the steps condition on the ORIGINAL timesteps of the two indices)
        mo = [diffusion()._wrap_model(buf.model)(x, ht(ti), **KW) for x, ti in ((noise(1), T1), (ref[0], T2))]
    for k in range(2):
        assert torch.equal(buf.outs[k], mo[k]), (mc, kind, "stored model output", k)
