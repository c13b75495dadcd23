"""CPU-only: the argument rules of the seven denoising-step entry points (include/sin3dm_hip.h), as a literal table.

Every request below is settled before any device work, so the table runs without a GPU:
  * a rejected request returns ERR_INVALID and the entry's name leads s3d_last_error();
  * a request a model entry (s3d_unet_step_film*) ACCEPTS goes on to the forward, which stops at the handle's missing parameters
    (ERR_MISSING, "parameter ...": nothing was ever set on it) before it touches the device;
  * a request a stand-alone entry (s3d_sampler_step*) accepts has batch == 0 and launches nothing (0).
The expected values were recorded from the library as it stood before the entries shared one validator; where the entries differ
(the plain and carry forms do not look at the mode's range, at eta or at y0 / mask; only the multistep entries look at T) the
table says so, row by row."""
import ctypes as C

import pytest

from sin3dm_amd import _lib

INVALID, MISSING, OK = _lib.ERR_INVALID, _lib.ERR_MISSING, 0
B, H, W, D, CH = 1, 2, 2, 2, 12
PER = CH * (H + D) * (W + D)
DDPM, DDIM, MEAN_ONLY = _lib.STEP_DDPM, _lib.STEP_DDIM, _lib.STEP_MEAN_ONLY
P, Q, R = 64, 128, 192                      # three distinct non-null "pointers": never dereferenced on the host

FILM = ("unet_step_film", "unet_step_film_carry", "unet_step_film_known", "unet_step_film_multistep")
ALONE = ("sampler_step", "sampler_step_known", "sampler_step_multistep")


def make_handle(in_ch=CH, out_ch=CH):
    cfg = _lib.UNetCfg(in_channels=in_ch, model_channels=32, out_channels=out_ch, num_res_blocks=1, n_levels=1,
                       use_scale_shift_norm=1, is_rollout=1)
    cfg.channel_mult[0] = 1
    h = C.c_void_p()
    assert _lib.load().s3d_unet_create(C.byref(cfg), C.byref(h)) == 0, _lib.last_error()       # (builds the parameter list: no device)
    return h


@pytest.fixture(scope="module")
def handles():
    hs = {"model": make_handle(), "uneven": make_handle(CH, 8)}
    yield hs
    for h in hs.values():
        _lib.load().s3d_unet_destroy(h)


def good_step(entry):
    """A complete request of `entry`: DDPM for the plain / carry / known forms, DDIM for multistep; batch 0 for the stand-alone ones."""
    alone = entry in ALONE
    return dict(mode=DDIM if "multistep" in entry else DDPM, mean_type=_lib.MEAN_START_X, clip_denoised=1, eta=0.0, T=20,
                batch=0 if alone else B, per_sample=PER, model_out=P if alone else None, x=P, noise=P, t=P, tables=P, sample=Q,
                pred_xstart=R)


GOOD_KNOWN = dict(y0=P, mask=P, noise=P, tables=P)
GOOD_MS = dict(x0_prev=P, tables=P, order=2)
NULL = "null"                                 # (in place of a struct: pass a null pointer)


def call(handles, entry, step=None, known=None, ms=None, handle="model", film=P, stride=0, b=B, model_out=None, flags=0):
    """One call of `entry`: `step` / `known` / `ms` are field overrides of the good request (NULL: a null pointer)."""
    lib = _lib.load()
    a = None if step == NULL else _lib.SamplerArgs(**dict(good_step(entry), **(step or {})))
    kr = None if known == NULL else _lib.KnownRegionArgs(**dict(GOOD_KNOWN, **(known or {})))
    m = None if ms == NULL else _lib.MultistepArgs(**dict(GOOD_MS, **(ms or {})))
    h = None if handle is None else handles[handle]
    if stride == "full":
        stride = lib.s3d_unet_film_width(h)
    if entry == "sampler_step":
        return lib.s3d_sampler_step(a, None)
    if entry == "sampler_step_known":
        return lib.s3d_sampler_step_known(a, kr, None)
    if entry == "sampler_step_multistep":
        return lib.s3d_sampler_step_multistep(a, m, None if known is None else kr, None)      # (the known region is optional here)
    head = (h, film, stride, b, H, W, D, a)
    if entry == "unet_step_film":
        return lib.s3d_unet_step_film(*head, model_out, None)
    if entry == "unet_step_film_carry":
        return lib.s3d_unet_step_film_carry(*head, model_out, None, flags)
    if entry == "unet_step_film_known":
        return lib.s3d_unet_step_film_known(*head, kr, model_out, None, flags)
    assert entry == "unet_step_film_multistep"
    return lib.s3d_unet_step_film_multistep(*head, m, model_out, None, flags)


def S(**kw):
    return dict(step=kw)


# (entry or entries, keyword arguments of call(), return code, leading word of s3d_last_error() or None when the call succeeds)
TABLE = [
    # ---- the good requests themselves
    (FILM, {}, MISSING, "parameter"),
    (FILM, dict(stride="full"), MISSING, "parameter"),
    (FILM[1:], dict(flags=3), MISSING, "parameter"),
    (ALONE, {}, OK, None),
    # ---- null arguments
    (FILM, dict(handle=None), INVALID, "{e}"),
    (FILM, dict(film=None), INVALID, "{e}"),
    (FILM + ALONE, dict(step=NULL), INVALID, "{e}"),
    (("unet_step_film_known", "sampler_step_known"), dict(known=NULL), INVALID, "{e}"),
    (("unet_step_film_multistep", "sampler_step_multistep"), dict(ms=NULL), INVALID, "{e}"),
    # ---- carry flags, film stride
    (FILM[1:], dict(flags=4), INVALID, "{e}"),
    (FILM[1:], dict(flags=-1), INVALID, "{e}"),
    (FILM, dict(stride=1), INVALID, "{e}"),
    # ---- required pointers
    (FILM + ALONE, S(x=None), INVALID, "{e}"),
    (FILM + ALONE, S(t=None), INVALID, "{e}"),
    (FILM + ALONE, S(tables=None), INVALID, "{e}"),
    (FILM + ALONE, S(pred_xstart=None), INVALID, "{e}"),
    (FILM + ALONE, S(sample=None), INVALID, "{e}"),
    (ALONE, S(model_out=None), INVALID, "{e}"),
    (("unet_step_film", "unet_step_film_carry", "unet_step_film_known", "sampler_step", "sampler_step_known"), S(noise=None), INVALID, "{e}"),
    (("unet_step_film_multistep", "sampler_step_multistep"), S(noise=None), "accept", None),            # (the ODE form has no eps)
    # ---- MEAN_ONLY: the plain and carry forms and s3d_sampler_step, and there without a sample
    (("unet_step_film", "unet_step_film_carry"), S(mode=MEAN_ONLY, sample=None, noise=None), MISSING, "parameter"),
    ("sampler_step", S(mode=MEAN_ONLY, sample=None, noise=None), OK, None),
    (("unet_step_film_known", "sampler_step_known"), S(mode=MEAN_ONLY), INVALID, "{e}"),
    (("unet_step_film_multistep", "sampler_step_multistep"), S(mode=MEAN_ONLY), INVALID, "{e}"),
    # ---- DDIM: eta != 0 needs the noise — not looked at by the plain and carry model entries, nor by the multistep ones
    (FILM[:3] + ALONE[:2], S(mode=DDIM, noise=None), "accept", None),
    (("unet_step_film", "unet_step_film_carry"), S(mode=DDIM, eta=0.5, noise=None), MISSING, "parameter"),
    (("unet_step_film_known", "sampler_step", "sampler_step_known"), S(mode=DDIM, eta=0.5, noise=None), INVALID, "{e}"),
    (("unet_step_film_multistep", "sampler_step_multistep"), S(eta=0.5, noise=None), "accept", None),
    (("unet_step_film_known", "sampler_step", "sampler_step_known"), S(mode=DDIM, eta=0.5), "accept", None),
    # ---- a mode out of range: the plain and carry model entries do not look
    (("unet_step_film", "unet_step_film_carry"), S(mode=7), MISSING, "parameter"),
    (("unet_step_film_known", "unet_step_film_multistep") + ALONE, S(mode=7), INVALID, "{e}"),
    (("unet_step_film_multistep", "sampler_step_multistep"), S(mode=DDPM), INVALID, "{e}"),
    # ---- the step's own y0 / mask (x0 replacement)
    (("unet_step_film", "unet_step_film_carry", "sampler_step"), S(y0=P, mask=P), "accept", None),
    (("unet_step_film", "unet_step_film_carry"), S(y0=P), MISSING, "parameter"),
    (("unet_step_film", "unet_step_film_carry"), S(mask=P), MISSING, "parameter"),
    ("sampler_step", S(y0=P), INVALID, "{e}"),
    ("sampler_step", S(mask=P), INVALID, "{e}"),
    (("unet_step_film_known", "sampler_step_known", "unet_step_film_multistep", "sampler_step_multistep"), S(y0=P, mask=P), INVALID, "{e}"),
    (("unet_step_film_known", "sampler_step_known", "unet_step_film_multistep", "sampler_step_multistep"), S(y0=P), INVALID, "{e}"),
    (("unet_step_film_known", "sampler_step_known", "unet_step_film_multistep", "sampler_step_multistep"), S(mask=P), INVALID, "{e}"),
    # ---- the posterior mean
    (("unet_step_film", "unet_step_film_carry", "sampler_step", "sampler_step_known"), S(mean=P), "accept", None),
    ("unet_step_film_known", S(mean=P), INVALID, "{e}"),
    ("unet_step_film_known", dict(step=dict(mean=P), model_out=P), MISSING, "parameter"),
    (("unet_step_film_multistep", "sampler_step_multistep"), S(mean=P), INVALID, "{e}"),
    ("unet_step_film_multistep", dict(step=dict(mean=P), model_out=P), INVALID, "{e}"),
    (FILM, dict(model_out=P), MISSING, "parameter"),
    # ---- the known region's fields
    (("unet_step_film_known", "sampler_step_known", "sampler_step_multistep"), dict(known=dict(y0=None)), INVALID, "{e}"),
    (("unet_step_film_known", "sampler_step_known", "sampler_step_multistep"), dict(known=dict(mask=None)), INVALID, "{e}"),
    (("unet_step_film_known", "sampler_step_known", "sampler_step_multistep"), dict(known=dict(noise=None)), INVALID, "{e}"),
    (("unet_step_film_known", "sampler_step_known", "sampler_step_multistep"), dict(known=dict(tables=None)), INVALID, "{e}"),
    ("sampler_step_multistep", dict(known={}), OK, None),
    # ---- the multistep update's fields
    (("unet_step_film_multistep", "sampler_step_multistep"), dict(ms=dict(tables=None)), INVALID, "{e}"),
    (("unet_step_film_multistep", "sampler_step_multistep"), dict(ms=dict(order=3)), INVALID, "{e}"),
    (("unet_step_film_multistep", "sampler_step_multistep"), dict(ms=dict(order=0)), INVALID, "{e}"),
    (("unet_step_film_multistep", "sampler_step_multistep"), dict(ms=dict(x0_prev=None)), INVALID, "{e}"),
    (("unet_step_film_multistep", "sampler_step_multistep"), dict(ms=dict(x0_prev=R)), INVALID, "{e}"),       # (aliases pred_xstart)
    (("unet_step_film_multistep", "sampler_step_multistep"), dict(ms=dict(order=1, x0_prev=None)), "accept", None),
    (("unet_step_film_multistep", "sampler_step_multistep"), dict(ms=dict(order=1, x0_prev=R)), "accept", None),
    # ---- sizes: T, batch and per_sample on their own are looked at by the stand-alone entries and by the two multistep entries
    (ALONE + ("unet_step_film_multistep",), S(T=0), INVALID, "{e}"),
    (FILM[:3], S(T=0), MISSING, "parameter"),
    (ALONE, S(batch=-1), INVALID, "{e}"),
    (ALONE, S(per_sample=-1), INVALID, "{e}"),
    # ---- a shape that is not the model's
    (FILM, S(batch=2), INVALID, "{e}"),
    (FILM, S(per_sample=PER - 1), INVALID, "{e}"),
    (FILM, dict(b=2), INVALID, "{e}"),
    (FILM, dict(handle="uneven", step=dict(per_sample=8 * (H + D) * (W + D))), INVALID, "{e}"),       # (in_channels != out_channels)
    (FILM, dict(b=0, step=dict(batch=0)), INVALID, "unet_forward"),                                    # (the forward's own check)
]


def expand():
    for entries, kw, rc, lead in TABLE:
        for e in ((entries,) if isinstance(entries, str) else entries):
            if rc == "accept":
                want = (MISSING, "parameter") if e in FILM else (OK, None)
            else:
                want = (rc, lead.format(e=e) if lead else None)
            yield pytest.param(e, kw, *want, id=f"{e}-{'-'.join(f'{k}={v}' for k, v in sorted(kw.items())) or 'good'}")


@pytest.mark.parametrize("entry,kw,rc,lead", list(expand()))
def test_request_table(handles, entry, kw, rc, lead):
    got = call(handles, entry, **kw)
    err = _lib.last_error()
    print(entry, kw, "->", got, repr(err[:60]))
    assert got == rc, err
    if lead is not None:
        assert err.split(":")[0].split(" ")[0] == lead, err


def test_create_and_the_table_need_no_device():
    """s3d_unet_create only builds the parameter list: the handle exists where hipGetDeviceCount finds nothing, or errs."""
    h = make_handle()
    assert h.value and _lib.load().s3d_unet_num_params(h) > 0
    _lib.load().s3d_unet_destroy(h)
