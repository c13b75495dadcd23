"""The cases and metrics of the UNet float64-reference tests, shared by tests/test_unet_f64_host.py, tests/test_hip_unet_f64.py
and tools/unet_f64_report.py.  A plain module: no fixtures, no GPU.

Reference: oracle/torch_port.py evaluated in float64 on the same float32 parameter values (T.synthetic_state_dict(.., 0)),
x0 (T.synthetic_noise(.., 400).clamp(-1, 1)) and noise (T.synthetic_noise(.., 401)), promoted; x_t is formed in float64 from the
float64 schedule tables.  The same port in float32 is the yardstick: a device error is judged as a multiple of the float32
port's error on the same case (see tests/test_hip_unet_f64.py), and the float32 port itself is held under the caps below.

Two timestep classes.  With t <= 3 the argument t * freq of the sinusoidal embedding is nearly exact in float32; at t = 999 its
rounding alone is about 6e-5 rad and dominates the error of ANY float32 evaluation ("UNet against float64")."""
import functools
import os
import sys

import numpy as np

from sin3dm_amd import testing as T

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARAM_SEED, X0_SEED, NOISE_SEED = 0, 400, 401
TERMS = ("mse_xy", "mse_xz", "mse_yz", "loss")
PLANE_NAMES = ("xy", "xz", "yz")
ZERO_GRAD_REL = 1e-9                       # max|g64_k| < ZERO_GRAD_REL * G: a zero-gradient tensor
EPS32 = 2.0 ** -23


TRAIN_MAX_CH = 12                          # kSmallMaxS (s3d_bwd.h): s3d_unet_train_attach refuses a wider in/out_channels
TRAIN_REFUSED = "in/out_channels <= 12"


def _case(mc, hwd, B, t, cm=(1, 2), ssn=True, rollout=True, predict_xstart=True, w=None, refused=None, ch=12):
    """ch: the latent width, in_channels = out_channels (fdim_geo for --data_type sdf, fdim_geo + fdim_tex otherwise).
    refused: the message with which the library refuses the model's forward and training step; train_refused: the training step alone."""
    assert len(t) == B and (w is None or len(w) == B)
    return dict(mc=mc, hwd=hwd, B=B, t=tuple(t), cm=cm, ssn=ssn, rollout=rollout, predict_xstart=predict_xstart, w=w,
                large_t=max(t) > 3, refused=refused, ch=ch, train_refused=TRAIN_REFUSED if ch > TRAIN_MAX_CH else None)


CASES = {
    "A": _case(32, (9, 13, 7), 5, (0, 1, 2, 3, 1)),                       # batch > 4: the second pass of the bias-gradient sums
    "A'": _case(32, (9, 13, 7), 5, (999, 700, 250, 500, 998)),
    "B": _case(64, (17, 33, 9), 2, (0, 2)),                               # one pixel past 8x16 regions / 4x16 tiles
    "B'": _case(64, (17, 33, 9), 2, (999, 700)),
    "Be": _case(64, (16, 32, 8), 2, (1, 3)),                              # even planes: the output blocks' virtual concat is taken
    "C": _case(128, (17, 33, 9), 1, (1,)),
    "D": _case(128, (9, 12, 5), 3, (2, 0, 3)),
    "E": _case(64, (7, 2, 9), 5, (0, 1, 2, 3, 1)),                        # a two-pixel-wide plane
    "F": _case(96, (10, 14, 6), 2, (1, 3)),                               # 3 channels per GroupNorm group, 288-channel concat
    # The model without rollout has no skip-size resize (the reference's torch.cat fails on planes that are not divisible by
    # 2^levels; the port resizes regardless): the library refuses G1's odd planes with this message, G1e is the same model on even ones.
    "G1": _case(32, (9, 13, 7), 2, (1, 3), rollout=False, refused="no skip-size resize"),
    "G1e": _case(32, (10, 14, 6), 2, (1, 3), rollout=False),
    "G2": _case(32, (9, 13, 7), 2, (1, 3), ssn=False),
    "G2b": _case(64, (9, 13, 7), 2, (1, 3), ssn=False),
    "G3": _case(32, (12, 20, 8), 2, (1, 3), cm=(1, 2, 2)),
    "G4": _case(64, (9, 13, 7), 2, (1, 3), cm=(1, 2, 2)),
    "H": _case(64, (9, 13, 7), 3, (3, 0, 1), predict_xstart=False, w=(1.0, 0.25, 2.0)),
    # Latent widths other than 12 (parser_util.train_args: fdim_geo for --data_type sdf, both options of the command line).  The
    # inference side changes form at 16 | 17 (k_in_conv_lds: Cin <= 16 at 64 / 128 / 256 channels; k_out_head_px: Cout <= 16; the
    # carried in_conv: Cin == Cout <= 16), the training side refuses above 12 (TRAIN_MAX_CH).
    "W4": _case(64, (9, 13, 7), 2, (1, 3), ch=4),                         # the sdf width: LDS in_conv, pixel-chunk head
    "W4n": _case(32, (9, 13, 7), 2, (1, 3), ch=4),                        # width 4 in k_in_conv / k_out_head
    "W4w": _case(128, (9, 12, 5), 1, (2,), ch=4),
    "W4e": _case(64, (9, 13, 7), 3, (3, 0, 1), predict_xstart=False, w=(1.0, 0.25, 2.0), ch=4),
    "W1": _case(64, (9, 13, 7), 2, (1, 3), ch=1),
    "W8": _case(64, (17, 33, 9), 1, (2,), ch=8),                          # the head's first weight-register half exactly, none of the second
    "W11": _case(128, (9, 12, 5), 2, (0, 3), ch=11),                      # an odd width just under the training limit
    "W16": _case(64, (9, 13, 7), 2, (1, 3), ch=16),                       # the last width of the fast forms; training refused
    "W20": _case(64, (9, 13, 7), 2, (1, 3), ch=20),                       # k_in_conv / k_out_head + k_sampler at 64 channels
    "W20n": _case(32, (9, 13, 7), 2, (1, 3), ch=20),
}

# What the float32 port must stay under on every case (conditions on the inputs, about twice its worst error over the cases as
# first measured): a case that breaks one is ill-conditioned and needs other inputs, never a wider cap.  Two caps on the loss
# terms.  `loss`: the per-sample `loss` term alone, which the first cap was taken from (the float32 port's worst: 9.3e-8 /
# 3.4e-7).  `terms`: the worst of all four terms, the quantity the device is judged against.  A plane term is a mean over a third
# of the values or fewer (168 on case E's xy plane) and its float32 error moves with the CPU's summation order; worst seen on
# two hosts 2.41e-7 (E) / 9.74e-7 (B'), and the cap is twice that by the same rule.
CAPS = {False: dict(fwd=2.5e-6, loss=2e-7, terms=5e-7, grad=8e-6, zero=1e-6),       # timesteps <= 3
        True: dict(fwd=2e-5, loss=1e-6, terms=2e-6, grad=8e-5, zero=1e-6)}          # large timesteps (A', B')


def _port_modules():
    p = os.path.join(REPO, "oracle")
    if p not in sys.path:
        sys.path.insert(0, p)
    import oracle as orc
    import torch_port as tp
    return orc, tp


def param_shapes(case):
    c = CASES[case]
    return T.unet_param_shapes(in_channels=c["ch"], model_channels=c["mc"], out_channels=c["ch"], rollout=c["rollout"], use_scale_shift_norm=c["ssn"], channel_mult=c["cm"])


def state_dict(case):
    return T.synthetic_state_dict(param_shapes(case), PARAM_SEED)


def inputs(case):
    """(x0, noise, t, w): float32, float32, int64, float32 torch CPU tensors; w is all ones where the case sets none."""
    import torch
    c = CASES[case]
    H, W, D = c["hwd"]
    shape = (c["B"], c["ch"], H + D, W + D)
    x0 = torch.from_numpy(T.synthetic_noise(shape, X0_SEED)).clamp(-1, 1)
    noise = torch.from_numpy(T.synthetic_noise(shape, NOISE_SEED))
    w = torch.tensor(c["w"] if c["w"] is not None else [1.0] * c["B"], dtype=torch.float32)
    return x0, noise, torch.tensor(c["t"], dtype=torch.int64), w


@functools.lru_cache(maxsize=None)
def port(case, double, w=None):
    """The port's result for a case in float64 (double) or float32, as numpy arrays that callers leave unchanged:
    {"x_t", "y" (the model output on x_t), "terms": {name: [B]}, "grads": {name: array}}; the gradients are those of
    (loss * w).mean() with the case's weights, or with the tuple `w` in their place."""
    import torch
    orc, tp = _port_modules()
    c = CASES[case]
    H, W, D = c["hwd"]
    dt = torch.float64 if double else torch.float32
    x0, noise, t, wc = inputs(case)
    if w is not None:
        wc = torch.tensor(w, dtype=torch.float32)
    sd = {k: v.to(dt).requires_grad_(True) for k, v in state_dict(case).items()}
    n = torch.get_num_threads()
    torch.set_num_threads(min(16, n))
    try:
        terms, x_t = tp.training_losses(sd, x0.to(dt), t, noise.to(dt), orc.schedule_tables_named(1000), H, W, D,
                                        predict_xstart=c["predict_xstart"], weights=wc, model_channels=c["mc"],
                                        channel_mult=c["cm"], use_scale_shift_norm=c["ssn"], rollout=c["rollout"])
        terms["objective"].backward()
        with torch.no_grad():
            y = tp.unet_forward(sd, x_t, t.to(dt), H, W, D, model_channels=c["mc"], channel_mult=c["cm"],
                                use_scale_shift_norm=c["ssn"], rollout=c["rollout"])
    finally:
        torch.set_num_threads(n)
    assert x_t.dtype == dt and y.dtype == dt and all(v.grad.dtype == dt for v in sd.values())
    out = {"x_t": x_t.detach().numpy(), "y": y.numpy(), "terms": {k: terms[k].detach().numpy() for k in TERMS},
           "grads": {k: v.grad.numpy() for k, v in sd.items()}}
    for a in (out["x_t"], out["y"], *out["terms"].values(), *out["grads"].values()):
        a.setflags(write=False)
    return out


# ---------------------------------------------------------------------------------------------------------------- metrics
def planes(c, H, W, D):
    """The three plane regions of a composite [..., H + D, W + D], as views."""
    return c[..., :H, :W], c[..., :H, W:], c[..., H:, :W]


def forward_error(y, y64, hwd, zero_corner=True):
    """(worst, (sample, plane)): max|y - y64| / max|y64| over each plane of each sample, the worst of them and where it is.
    The padding corner y[..., H:, W:] must be exactly zero; with zero_corner=False (a sampler step's x_{t-1}, whose corner is the
    update of a model output of 0) it is a fourth region, "corner", compared like the planes."""
    H, W, D = hwd
    y, y64 = np.asarray(y, np.float64), np.asarray(y64, np.float64)
    assert y.shape == y64.shape, (y.shape, y64.shape)
    if zero_corner:
        assert not np.any(y[..., H:, W:]), "the padding corner of the output is not zero"
    worst = (-1.0, None)
    for b in range(y.shape[0]):
        regions = list(zip(PLANE_NAMES, planes(y[b], H, W, D), planes(y64[b], H, W, D)))
        if not zero_corner:
            regions.append(("corner", y[b][..., H:, W:], y64[b][..., H:, W:]))
        for name, a, r in regions:
            worst = max(worst, (float(np.max(np.abs(a - r)) / np.max(np.abs(r))), (b, name)))
    return worst


def loss_error(terms, terms64, keys=TERMS):
    """(worst, (term, sample)) of |a - b| / |b| over the four loss terms of every sample."""
    worst = (-1.0, None)
    for k in keys:
        a, r = np.asarray(terms[k], np.float64), np.asarray(terms64[k], np.float64)
        assert a.shape == r.shape, (k, a.shape, r.shape)
        e = np.abs(a - r) / np.abs(r)
        worst = max(worst, (float(e.max()), (k, int(e.argmax()))))
    return worst


def grad_errors(grads, grads64):
    """(E, Z, G).  G = max_k max|g64_k|.  A tensor with max|g64_k| < ZERO_GRAD_REL * G is a zero-gradient tensor (a conv bias in
    front of a one-channel-per-group GroupNorm) and gets Z[k] = max|g_k| / G; every other tensor gets
    E[k] = max|g_k - g64_k| / max|g64_k|: elementwise, relative to the tensor's own largest element, no floor."""
    assert sorted(grads) == sorted(grads64)
    G = max(float(np.max(np.abs(v))) for v in grads64.values())
    E, Z = {}, {}
    for k, r in grads64.items():
        a = np.asarray(grads[k], np.float64)
        assert a.shape == r.shape, (k, a.shape, r.shape)
        m = float(np.max(np.abs(r)))
        if m < ZERO_GRAD_REL * G:
            Z[k] = float(np.max(np.abs(a))) / G
        else:
            E[k] = float(np.max(np.abs(a - r))) / m
    return E, Z, G


def worst_of(d):
    """(value, name) of the largest entry; (0.0, None) for an empty map."""
    return max(((v, k) for k, v in d.items()), default=(0.0, None))


def port_errors(case):
    """The float32 port against the float64 port: {"fwd", "loss" (all four terms), "grad", "zero"} (worst values), "grad_name",
    and "loss_only": the error of the per-sample `loss` term alone."""
    p32, p64 = port(case, False), port(case, True)
    E, Z, _ = grad_errors(p32["grads"], p64["grads"])
    e, name = worst_of(E)
    return {"fwd": forward_error(p32["y"], p64["y"], CASES[case]["hwd"])[0], "loss": loss_error(p32["terms"], p64["terms"])[0],
            "loss_only": loss_error(p32["terms"], p64["terms"], ("loss",))[0], "grad": e, "grad_name": name, "zero": worst_of(Z)[0]}


# ------------------------------------------------------------------------------------------------------------- the device
def device_model(case):
    """A fresh HIP model of the case on cuda:0 with the case's parameters."""
    import torch
    from sin3dm_amd.diffusion.unet_triplane import TriplaneUNetModelSmall, TriplaneUNetModelSmallRaw
    c = CASES[case]
    cls = TriplaneUNetModelSmall if c["rollout"] else TriplaneUNetModelSmallRaw
    m = cls(c["ch"], c["mc"], c["ch"], channel_mult=c["cm"], use_scale_shift_norm=c["ssn"])
    m.load_state_dict(state_dict(case))
    return m.to(torch.device("cuda:0"))


def device_diffusion(case):
    from sin3dm_amd.diffusion.script_util import create_gaussian_diffusion
    return create_gaussian_diffusion(steps=1000, noise_schedule="linear", predict_xstart=CASES[case]["predict_xstart"])


def device_forward(case, kernels=None):
    """The inference forward of a fresh model on the float32 port's x_t (twice, the same bits): a float32 numpy array.
    kernels: a dict that receives the names of the kernels the 3x3, 1x1 and rank-1 launches dispatched (s3d_unet_profile_kernel)."""
    import torch
    c = CASES[case]
    H, W, D = c["hwd"]
    m = device_model(case).eval()
    dev = torch.device("cuda:0")
    x_t = torch.from_numpy(port(case, False)["x_t"].copy()).to(dev)
    t = torch.tensor(c["t"], dtype=torch.int64, device=dev)
    if kernels is not None:
        m.profile(1, classes=7)
    with torch.no_grad():
        y = m(x_t, t, H=H, W=W, D=D).clone()
        y2 = m(x_t, t, H=H, W=W, D=D)
    assert torch.equal(y, y2), "the second forward gives other bits"
    if kernels is not None:
        m.profile_read()
        kernels.update(conv3x3=m.profile_kernel(0), conv1x1=m.profile_kernel(1), rank1=m.profile_kernel(2))
    return y.cpu().numpy()


def device_step(case, autograd=False, kernels=None):
    """One training step of a fresh model on the device: (terms {name: [B] numpy}, grads {name: numpy}).  The graph-free path
    (training_losses_and_grads) or, with autograd, (terms["loss"] * w).mean().backward(); run twice, the same bits both times.  kernels: a dict that receives the names of the
    kernels the 3x3 convolutions (forward and input gradient) and the 3x3 weight gradients dispatched."""
    import torch
    c = CASES[case]
    H, W, D = c["hwd"]
    m = device_model(case)
    diffusion = device_diffusion(case)
    dev = torch.device("cuda:0")
    x0, noise, t, w = (v.to(dev) for v in inputs(case))
    kw = dict(H=H, W=W, D=D)
    if kernels is not None:
        m.profile(1, classes=1 | 8)
    runs = []
    for _ in range(2):
        if autograd:
            for p in m.parameters():
                p.grad = None
            terms = diffusion.training_losses(m, x0, t, model_kwargs=kw, noise=noise)
            (terms["loss"] * w).mean().backward()
            grads = {k: p.grad.detach().clone() for k, p in m.named_parameters()}
        else:
            terms, flat = diffusion.training_losses_and_grads(m, x0, t, w, kw, noise=noise)
            grads = {k: v.clone() for k, v in m.split_flat(flat).items()}
        runs.append(({k: terms[k].detach().clone() for k in TERMS}, grads))
    for a, b in zip(runs[0], runs[1]):
        for k in a:
            assert torch.equal(a[k], b[k]), f"the second step gives other bits: {k}"
    if kernels is not None:
        m.profile_read()
        kernels.update(conv3x3=m.profile_kernel(0), wgrad=m.profile_kernel(3))
    return tuple({k: v.cpu().numpy() for k, v in d.items()} for d in runs[0])


def device_errors(case, y=None, step=None):
    """Errors of device results against the float64 port, in the shape of port_errors (only the parts given), with where the
    worst forward plane and loss term are."""
    p64 = port(case, True)
    out = {}
    if y is not None:
        out["fwd"], out["fwd_at"] = forward_error(y, p64["y"], CASES[case]["hwd"])
    if step is not None:
        terms, grads = step
        out["loss"], out["loss_at"] = loss_error(terms, p64["terms"])
        E, Z, _ = grad_errors(grads, p64["grads"])
        out["E"], out["Z"] = E, Z
        out["grad"], out["grad_name"] = worst_of(E)
        out["zero"], out["zero_name"] = worst_of(Z)
    return out


# ------------------------------------------------------------------------------------------------------ one sampler step
# One fused denoising step at the case's timesteps on the float32 port's x_t, eps = T.synthetic_noise(.., STEP_EPS_SEED): the DDPM
# update and the DDIM update with eta = 0 (gaussian_diffusion.py:396-440, 538-600; x0 prediction, clipped, no respacing).
STEP_EPS_SEED = 402
STEP_MODES = ("ddpm", "ddim")
STEP_CASES = ("W4", "W1", "W16", "W20")


def step_eps(case):
    return T.synthetic_noise(port(case, False)["x_t"].shape, STEP_EPS_SEED)


@functools.lru_cache(maxsize=None)
def step_reference(case):
    """{mode: {"f64": (sample, pred_xstart), "f32": (sample, pred_xstart)}}.  f64: the port's forward in float64 on the float32 x_t
    promoted, then the update in float64 from the float64 tables; f32: the float32 port's forward, then the C oracle's updates."""
    import torch
    orc, tp = _port_modules()
    c = CASES[case]
    assert c["predict_xstart"] and min(c["t"]) > 0
    H, W, D = c["hwd"]
    p32 = port(case, False)
    x, eps = p32["x_t"].copy(), step_eps(case)
    tab, _ = orc.schedule_tables()
    sd = {k: v.double() for k, v in state_dict(case).items()}
    n = torch.get_num_threads()
    torch.set_num_threads(min(16, n))
    try:
        with torch.no_grad():
            y64 = tp.unet_forward(sd, torch.from_numpy(x).double(), torch.tensor(c["t"], dtype=torch.float64), H, W, D,
                                  model_channels=c["mc"], channel_mult=c["cm"], use_scale_shift_norm=c["ssn"], rollout=c["rollout"])
    finally:
        torch.set_num_threads(n)
    out = {m: {"f64": ([], []), "f32": ([], [])} for m in STEP_MODES}
    for b, t in enumerate(c["t"]):
        xb, eb = torch.from_numpy(x[b]).double(), torch.from_numpy(eps[b]).double()
        s, p = tp.p_sample_update(y64[b], xb, eb, tab, t)
        out["ddpm"]["f64"][0].append(s.numpy()), out["ddpm"]["f64"][1].append(p.numpy())
        # DDIM, eta = 0 (:538-600): eps from the clipped x0, then the deterministic step to alphas_cumprod_prev
        e = (float(tab[3][t]) * xb - p) / float(tab[4][t])
        s = p * float(np.sqrt(tab[2][t])) + float(np.sqrt(1.0 - tab[2][t])) * e
        out["ddim"]["f64"][0].append(s.numpy()), out["ddim"]["f64"][1].append(p.numpy())
        for m, fn in (("ddpm", orc.p_sample_update), ("ddim", orc.ddim_update)):
            s, p = fn(p32["y"][b], x[b], eps[b], tab, t)
            out[m]["f32"][0].append(s), out[m]["f32"][1].append(p)
    return {m: {k: tuple(np.stack(a) for a in v) for k, v in d.items()} for m, d in out.items()}


def step_errors(case, mode, sample, pred):
    """(sample, pred_xstart) errors against the float64 step: forward_error's measure; x_{t-1}'s corner is a region of its own
    and pred_xstart's is exactly zero."""
    s64, p64 = step_reference(case)[mode]["f64"]
    hwd = CASES[case]["hwd"]
    return forward_error(sample, s64, hwd, zero_corner=False), forward_error(pred, p64, hwd)


def device_fused_step(case, mode):
    """One fused step (the sampling loops' one-call form) of a fresh model: (sample, pred_xstart) as numpy arrays."""
    import torch
    from sin3dm_amd import _lib
    from sin3dm_amd.diffusion.gaussian_diffusion import HostTimesteps
    c = CASES[case]
    H, W, D = c["hwd"]
    dev = torch.device("cuda:0")
    m = device_model(case).eval()
    x = torch.from_numpy(port(case, False)["x_t"].copy()).to(dev)
    eps = torch.from_numpy(step_eps(case)).to(dev)
    t = HostTimesteps(torch.tensor(c["t"], dtype=torch.int64, device=dev), c["t"])
    with torch.no_grad():
        s, p, _ = device_diffusion(case)._step(_lib.STEP_DDPM if mode == "ddpm" else _lib.STEP_DDIM, m, x, t, True, None,
                                               dict(H=H, W=W, D=D), eta=0.0, fuse=True, noise=eps)
    return s.cpu().numpy(), p.cpu().numpy()


# ------------------------------------------------------------------------------------------------------------ kernel forms
# Forms the library takes by launch size or by option (include/sin3dm_hip.h: s3d_set_option), forced so that they run at test
# sizes.  CONV_IMPL=naive is the control: one thread per output, plain summation order.
FORWARD_FORMS = (("WINO", 0), ("WINO", 4), ("WINO24W", 1), ("VCAT", 0), ("GN_FUSED", 0), ("CONV1X1_T", 1), ("RANK1_BATCH", 0),
                 ("RANK1_SLICES", 0), ("CONV_IMPL", "naive"))
FORWARD_FORM_CASES = ("A", "B", "Be", "C", "D", "W4", "W16")
TRAINING_FORMS = (("WGRAD_WINO", 0), ("GNB_FUSED", 0), ("BWD_SIDE", 0), ("EDGE_SIGNAL", 0), ("WINO", 4))
TRAINING_FORM_CASES = ("A", "B", "D", "H", "W4")

# How a forced form shows that it ran.  By name: (launch class, a string the library's kernel names must hold, strings they must
# not hold).  By result: the cases on which the form's summation order differs from the default's, so the output bits must.
# VCAT=0 applies where the default takes the virtual concat (even planes: Be); RANK1_SLICES=0 where the default slices the
# rollout tables' K (own channels of 256 and more in whole 128-channel chunks: the 128-channel models).  GN_FUSED=0, BWD_SIDE=0
# and EDGE_SIGNAL=0 move sums or launches without changing a bit or a reported kernel: for them only the stored option is seen.
FORWARD_ENGAGED = {
    "WINO=0": ("conv3x3", "k_conv_mfma<3x3>", ("wino", "naive")),
    "WINO=4": ("conv3x3", "k_conv_wino4", ("wino24", "naive")),
    "WINO24W=1": ("conv3x3", "k_conv_wino24w", ("naive",)),
    "CONV1X1_T=1": ("conv1x1", "transposed accumulators", ("naive",)),
    "RANK1_BATCH=0": ("rank1", "k_rank1<", ("k_rank1b",)),
    "CONV_IMPL=naive": ("conv3x3", "k_conv_naive", ("mfma", "wino")),
}
FORWARD_DIFFERS = {"VCAT=0": ("Be",), "RANK1_SLICES=0": ("C", "D")}
TRAINING_ENGAGED = {
    "WGRAD_WINO=0": ("wgrad", "k_wgrad_mfma<9>", ("k_wgrad_wino",)),
    "GNB_FUSED=0": ("conv3x3", "k_conv_wino24s", ("gnb",)),
    "WINO=4": ("conv3x3", "k_conv_wino4", ("wino24",)),
}


def engaged(kernels, rule):
    """None, or why the kernel names do not show the form."""
    cls, must, must_not = rule
    name = kernels[cls]
    if must not in name or any(s in name for s in must_not):
        return f"{cls} launches ran {name!r}: expected {must!r} and none of {must_not}"
    return None


class forced:
    """with forced(name, value): the option is set process-wide and handed back to the library's own choice afterwards.  Build the
    model inside: a training handle refuses a form change after attach."""

    def __init__(self, name, value):
        self.name, self.value = name, value

    def __enter__(self):
        from sin3dm_amd import _lib
        if self.name is not None:
            _lib.set_option(self.name, self.value)
            assert _lib.get_option(self.name) == (1 if self.value == "naive" else int(self.value)), self.name
        return self

    def __exit__(self, *exc):
        from sin3dm_amd import _lib
        if self.name is not None:
            _lib.set_option(self.name, None)
        return False


def ratios(dev, prt):
    """err_dev / max(err_port32, 2^-23) for the parts of device_errors present."""
    return {k: dev[k] / max(prt[k], EPS32) for k in ("fwd", "loss", "grad", "zero") if k in dev}
