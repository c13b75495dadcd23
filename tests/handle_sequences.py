"""Sequences of calls on ONE live handle, and the fresh-handle reference of each of their steps: the cases of
tests/test_hip_handle_state.py and tests/test_handle_state_host.py.  A plain module: no fixtures, importable without a GPU
(torch and the library are only touched inside GpuBackend).

A sequence is a list of steps, a step a dict built by the constructors below.  `run_sequence` executes a sequence on one model
object and keeps every compute step's outputs; `reference` executes one compute step ALONE on a fresh model created with the
weights and under the options in force at that step (cached by the step's signature: fresh references repeat).  The comparison is
bit equality of every output of every compute step (`check_sequence`); nothing here has a tolerance.

What a step may carry from its predecessors on the reused handle and must not: the measured workspace, the carried in_conv, the
lanes, the training tape, and the Python mirror's FiLM cache / parameter stamp / flat attachment ("What a handle
remembers").  A step whose input is an earlier step's sample (`x_from`) has as its reference the plain, uncarried step on the
REFERENCE's sample of that earlier step (test_next_steps_in_conv_carried... holds carried and uncarried to the same bits).

`poison`: a forward on the reused handle with an all-NaN input, at a shape and batch at least as large as the next compute step's:
every activation, statistic and partial-sum buffer of the workspace it touches then holds NaN, so whatever the next step reads
without having written it shows up as NaN instead of a plausible stale number.  NaN arithmetic is no fault and the inference
forward addresses nothing by data: its kernels (k_in_conv*, k_gn_*, k_conv_*, k_rank1*, k_means_finalize, k_avgpool*, k_upcat*,
k_bilinear, k_copy_slice, k_out_head*; s3d_kernels.hip, s3d_conv.hip, s3d_wino*.hip) index by thread, block and geometry only —
the bilinear kernels' int(fy) / int(fx) are functions of the pixel coordinate.  The poison is a plain `forward` (no sampler update:
k_sampler reads its tables at the caller's integer timestep, also no data), and is left out of the training tier."""
import functools

# ---------------------------------------------------------------------------------------------------- options
# Every option of the library (kOptNames, s3d_common.h) is switched on a live handle by one of the two groups below, or is listed
# in NOT_APPLICABLE with the reason (tests/test_handle_state_host.py holds this against the header).
INFERENCE_OPTIONS = (("VCAT", "0"), ("GN_FUSED", "0"), ("GN_FUSED", "1"), ("WINO24W", "0"), ("WINO24W", "1"), ("CONV1X1_T", "0"),
                     ("CONV1X1_T", "1"), ("RANK1_BATCH", "0"), ("RANK1_SLICES", "0"), ("WINO", "4"), ("WINO", "0"),
                     ("CONV_IMPL", "naive"))
TRAINING_OPTIONS = (("GNB_FUSED", "0"), ("BWD_SIDE", "0"), ("EDGE_SIGNAL", "0"), ("WGRAD_WINO", "0"))
NOT_APPLICABLE = {}                       # name -> reason (none today)


def option_class(name):
    """'inference' (group 4), 'training' (group 5) or ('n/a', reason); None: unclassified."""
    if any(n == name for n, _ in INFERENCE_OPTIONS):
        return "inference"
    if any(n == name for n, _ in TRAINING_OPTIONS):
        return "training"
    if name in NOT_APPLICABLE:
        return ("n/a", NOT_APPLICABLE[name])
    return None


# ---------------------------------------------------------------------------------------------------- steps
COMPUTE_OPS = ("forward", "forward_host_t", "step", "mean_only", "train")
CARRY_OUT, CARRY_IN = 1, 2                # s3d_unet_step_film_carry flags


def forward(hwd, B, seed, t=None):
    """model(x, t) with a device timestep tensor."""
    return dict(op="forward", hwd=tuple(hwd), B=B, seed=seed, t=tuple(t) if t else tuple(5.0 + 37.0 * b for b in range(B)))


def forward_host_t(hwd, B, seed, t):
    """model(x, HostTimesteps(t)): the FiLM table of host-known values is cached on the Python side."""
    assert len(t) == B
    return dict(op="forward_host_t", hwd=tuple(hwd), B=B, seed=seed, t=tuple(float(v) for v in t))


def step(hwd, B, seed, ti, mode="ddpm", eta=0.0, inpaint=None, clip=True, px=True, buf=False, carry=0, x_from=None, clone=False):
    """One fused denoising step (s3d_unet_step_film[_carry]) at respaced index ti of a 10-step schedule (px: START_X) or of the
    full 1000-step one (EPSILON).  inpaint: None / 'mask' / 'mask_t0'; buf: the caller gives a model-output buffer; x_from: index
    (in the sequence) of the step whose sample is this step's input — the same tensor, or a clone of it."""
    assert mode in ("ddpm", "ddim") and inpaint in (None, "mask", "mask_t0") and not (buf and carry)
    return dict(op="step", hwd=tuple(hwd), B=B, seed=seed, ti=ti, mode=mode, eta=float(eta), inpaint=inpaint, clip=bool(clip),
                px=bool(px), buf=bool(buf), carry=carry, x_from=x_from, clone=bool(clone))


def mean_only(hwd, B, seed, ti):
    """p_mean_variance: forward, then the MEAN_ONLY sampler kernel."""
    return dict(op="mean_only", hwd=tuple(hwd), B=B, seed=seed, ti=ti)


def train(hwd, B, seed, t):
    """One training_losses_and_grads: loss terms and the flat gradient."""
    assert len(t) == B
    return dict(op="train", hwd=tuple(hwd), B=B, seed=seed, t=tuple(int(v) for v in t))


def option(name, value):
    return dict(op="option", name=name, value=None if value is None else str(value))


def set_weights(seed=None, tensor=None, add=None, how="load_state_dict"):
    """Other weights on the live model: T.synthetic_state_dict(.., seed), or `tensor` += add.  how: 'load_state_dict', 'inplace'
    (under no_grad; on a non-flat model this reaches the handle through s3d_unet_set_param, on a flat-attached one through
    s3d_unet_repack), 'to_roundtrip' (the edit happens on the CPU between .cpu() and .to(device))."""
    assert (seed is None) != (tensor is None) and how in ("load_state_dict", "inplace", "to_roundtrip")
    assert how == "load_state_dict" or tensor is not None
    return dict(op="set_weights", seed=seed, tensor=tensor, add=add, how=how)


def lane(k):
    return dict(op="lane", k=int(k))


def attach_flat():
    """Re-home the parameters in one flat device vector and attach it (model.flat_parameters): the training tier's handle."""
    return dict(op="attach_flat")


def poison(hwd, B):
    return dict(op="poison", hwd=tuple(hwd), B=B)


# ---------------------------------------------------------------------------------------------------- planning (pure)
_NOT_IN_SIGNATURE = ("carry", "x_from", "clone")       # how a step is fed, not what it computes


def _freeze(d):
    return tuple(sorted((k, v) for k, v in d.items() if k not in _NOT_IN_SIGNATURE))


def covers(p, s):
    """the poison step p is at least as large as the compute step s in every plane and in the batch"""
    return p["B"] >= s["B"] and all(a >= b for a, b in zip(p["hwd"], s["hwd"]))


def plan(cfg, steps, inference=True):
    """Per step: the signature of a compute step — (model config, weights, options, the step, the signature of the step that
    produced its input) — or None.  Checks the sequence's own shape: x_from names an earlier `step` of the same shape; an inference
    sequence has its poison step (poisoned_steps)."""
    weights, opts, sigs = (("seed", 0),), {}, []
    for i, s in enumerate(steps):
        op = s["op"]
        if op == "option":
            if s["value"] is None:
                opts.pop(s["name"], None)
            else:
                opts[s["name"]] = s["value"]
        elif op == "set_weights":
            weights = (("seed", s["seed"]),) if s["seed"] is not None else weights + (("add", s["tensor"], float(s["add"])),)
        if op not in COMPUTE_OPS:
            sigs.append(None)
            continue
        x_sig = None
        if s.get("x_from") is not None:
            j = s["x_from"]
            assert 0 <= j < i and steps[j]["op"] == "step" and steps[j]["hwd"] == s["hwd"] and steps[j]["B"] == s["B"], (i, j)
            x_sig = sigs[j]
        sigs.append((_freeze(cfg), weights, tuple(sorted(opts.items())), _freeze(s), x_sig))
    if inference:
        assert poisoned_steps(steps), "no poison step before the last compute step"
    return sigs


def poisoned_steps(steps):
    """The indices of the compute steps that the sequence's last poison step is there for, or [] when the sequence lacks one: the
    last compute step — or, when that one takes the carried in_conv of the compute step right in front of it (a poison between
    the two would void the very carry under test), that pair.  The poison covers every one of them."""
    comp = [i for i, s in enumerate(steps) if s["op"] in COMPUTE_OPS]
    if len(comp) < 2:
        return []
    last, target = steps[comp[-1]], [comp[-1]]
    gap = [s for s in steps[comp[-2] + 1:comp[-1]] if s["op"] == "poison"]
    if not gap and (last.get("carry", 0) & CARRY_IN) and last.get("x_from") == comp[-2] and len(comp) >= 3:
        target = [comp[-2], comp[-1]]
        gap = [s for s in steps[comp[-3] + 1:comp[-2]] if s["op"] == "poison"]
    if not gap or not all(covers(p, steps[i]) for p in gap for i in target):
        return []
    return target


def run_sequence(backend, cfg, steps, inference=True):
    """Execute `steps` on one model object.  Returns (signatures, outputs), both parallel to steps (None for non-compute steps)."""
    sigs = plan(cfg, steps, inference)
    backend.clear_options()
    model = backend.make_model(cfg, (("seed", 0),))
    outs = []
    try:
        for s in steps:
            op, out = s["op"], None
            if op == "option":
                backend.set_option(s["name"], s["value"])
            elif op == "set_weights":
                backend.set_weights(model, s)
            elif op == "lane":
                backend.select_lane(model, s["k"])
            elif op == "attach_flat":
                backend.attach_flat(model)
            elif op == "poison":
                backend.poison(model, s)
            else:
                x = None
                if s.get("x_from") is not None:
                    x = outs[s["x_from"]][0]
                    if s["clone"]:
                        x = backend.clone(x)
                out = backend.run(model, s, x)
            outs.append(out)
    finally:
        backend.clear_options()
    return sigs, outs


def reference(backend, sig, cache):
    """The outputs of the compute step `sig` run alone on a fresh model (weights and options of the signature)."""
    if sig in cache:
        return cache[sig]
    cfg, weights, opts, s, x_sig = sig
    x = reference(backend, x_sig, cache)[0] if x_sig is not None else None
    backend.clear_options()
    try:
        for name, value in opts:
            backend.set_option(name, value)
        model = backend.make_model(dict(cfg), weights)
        out = backend.run(model, dict(s, carry=0, x_from=None, clone=False), x)
    finally:
        backend.clear_options()
    cache[sig] = out
    return out


def check_sequence(backend, cfg, steps, cache, inference=True):
    """Run the sequence, then hold every output of every compute step to its fresh reference, bit for bit."""
    sigs, outs = run_sequence(backend, cfg, steps, inference)
    for i, (sig, out) in enumerate(zip(sigs, outs)):
        if sig is None:
            continue
        ref = reference(backend, sig, cache)
        assert len(ref) == len(out), (i, steps[i])
        for k, (a, b) in enumerate(zip(out, ref)):
            assert backend.equal(a, b), f"step {i} output {k} differs from a fresh handle's: {steps[i]}"
    return sigs, outs


# ---------------------------------------------------------------------------------------------------- the GPU backend
class GpuBackend:
    """The steps on TriplaneUNetModelSmall / GaussianDiffusion (cfg: mc, cm; ssn is on)."""

    def __init__(self):
        import torch
        assert torch.cuda.is_available(), "GPU tests need an MI355X"
        self.dev = torch.device("cuda:0")
        self._touched = set()

    # -- options
    def set_option(self, name, value):
        from sin3dm_amd import _lib
        self._touched.add(name)
        _lib.set_option(name, value)

    def clear_options(self):
        from sin3dm_amd import _lib
        for name in sorted(self._touched):
            _lib.set_option(name, None)
        self._touched.clear()

    # -- weights
    @staticmethod
    @functools.lru_cache(maxsize=None)
    def _shapes(mc, cm):
        from sin3dm_amd import testing as T
        return T.unet_param_shapes(model_channels=mc, channel_mult=cm, use_scale_shift_norm=True)

    def state_dict(self, cfg, weights):
        from sin3dm_amd import testing as T
        sd = T.synthetic_state_dict(self._shapes(cfg["mc"], tuple(cfg["cm"])), weights[0][1])
        for _, name, c in weights[1:]:
            sd[name] = sd[name] + c
        return sd

    def make_model(self, cfg, weights):
        from sin3dm_amd.diffusion.unet_triplane import TriplaneUNetModelSmall
        m = TriplaneUNetModelSmall(12, cfg["mc"], 12, channel_mult=tuple(cfg["cm"]), use_scale_shift_norm=True)
        m.load_state_dict(self.state_dict(cfg, weights))
        m = m.to(self.dev).eval()
        m._seq_cfg = dict(cfg)
        return m

    def set_weights(self, model, s):
        import torch
        if s["how"] == "load_state_dict":
            if s["seed"] is not None:
                model.load_state_dict(self.state_dict(model._seq_cfg, (("seed", s["seed"]),)))
            else:
                sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
                sd[s["tensor"]] = sd[s["tensor"]] + s["add"]
                model.load_state_dict(sd)
            return
        if s["how"] == "to_roundtrip":
            model.cpu()
        with torch.no_grad():
            dict(model.named_parameters())[s["tensor"]].add_(s["add"])
        if s["how"] == "to_roundtrip":
            model.to(self.dev)

    def select_lane(self, model, k):
        model._select_lane(k)

    def attach_flat(self, model):
        assert model.flat_parameters is not None

    # -- inputs
    def _noise(self, s, seed, B=None):
        import torch
        from sin3dm_amd import testing as T
        H, W, D = s["hwd"]
        return torch.from_numpy(T.synthetic_noise((B or s["B"], 12, H + D, W + D), seed)).to(self.dev)

    @staticmethod
    @functools.lru_cache(maxsize=None)
    def _diffusion(px, resp):
        from sin3dm_amd.diffusion.script_util import create_gaussian_diffusion
        return create_gaussian_diffusion(steps=1000, noise_schedule="linear", predict_xstart=px, timestep_respacing=resp)

    def clone(self, x):
        return x.clone()

    def equal(self, a, b):
        import torch
        return a.shape == b.shape and torch.equal(a, b)

    # -- steps
    def poison(self, model, s):
        import torch
        H, W, D = s["hwd"]
        x = torch.full((s["B"], 12, H + D, W + D), float("nan"), device=self.dev)
        t = torch.full((s["B"],), 5.0, device=self.dev)
        with torch.no_grad():
            y = model(x, t, H=H, W=W, D=D)
        corner = torch.zeros_like(y, dtype=torch.bool)
        corner[..., H:, W:] = True                                     # (the composed map's corner is written as zero)
        assert bool(torch.isnan(y[~corner]).all()) and float(y[corner].abs().max()) == 0.0, "the poison forward's output is not all NaN"

    def run(self, model, s, x=None):
        import torch
        from sin3dm_amd import _lib
        from sin3dm_amd.diffusion.gaussian_diffusion import HostTimesteps
        H, W, D = s["hwd"]
        B, kw, op = s["B"], dict(H=H, W=W, D=D), s["op"]
        if x is None and op != "train":
            x = self._noise(s, s["seed"])
        if op == "forward":
            with torch.no_grad():
                return (model(x, torch.tensor(s["t"], device=self.dev, dtype=torch.float32), **kw),)
        if op == "forward_host_t":
            with torch.no_grad():
                return (model(x, HostTimesteps(torch.tensor(s["t"], device=self.dev, dtype=torch.float32), s["t"]), **kw),)
        if op == "mean_only":
            diff = self._diffusion(True, "10")
            with torch.no_grad():
                r = diff.p_mean_variance(model, x, torch.full((B,), s["ti"], device=self.dev, dtype=torch.int64), model_kwargs=kw)
            return (r["mean"], r["pred_xstart"])
        if op == "train":
            diff = self._diffusion(True, "")
            x0 = self._noise(s, s["seed"]).clamp(-1, 1)
            noise = self._noise(s, s["seed"] + 1)
            w = torch.tensor([1.0, 0.5, 2.0, 0.25][:B], device=self.dev)
            terms, g = diff.training_losses_and_grads(model, x0, torch.tensor(s["t"], device=self.dev), w, kw, noise=noise)
            return tuple(terms[k].clone() for k in sorted(terms)) + (g.clone(),)
        assert op == "step"
        diff = self._diffusion(s["px"], "10" if s["px"] else "")
        ti = s["ti"]
        ht = HostTimesteps(torch.full((B,), ti, device=self.dev, dtype=torch.int64), (ti,) * B)
        extra = dict(eta=s["eta"])
        if s["inpaint"]:
            extra.update(y0=self._noise(s, s["seed"] + 2), mask=(self._noise(s, s["seed"] + 3) > 0).float(),
                         is_mask_t0=s["inpaint"] == "mask_t0")
        mode = _lib.STEP_DDPM if s["mode"] == "ddpm" else _lib.STEP_DDIM
        eps = self._noise(s, s["seed"] + 1)
        target = _CallerBuffer(model) if s["buf"] else model
        with torch.no_grad():
            sample, pred, _ = diff._step(mode, target, x, ht, s["clip"], None, kw, fuse=True, noise=eps, carry=s["carry"], **extra)
        return (sample, pred) + ((target.buf,) if s["buf"] else ())


class _CallerBuffer:
    """The model's fused step with a caller buffer for the model output (s3d_unet_step_film's `model_out`), which the module's own
    denoise_step never passes."""
    carries_in_conv = False

    def __init__(self, model):
        self.model, self.buf = model, None

    def parameters(self):
        return self.model.parameters()

    def denoise_step(self, x, timesteps, step, H=None, W=None, D=None, carry=0):
        import ctypes as C
        import torch
        from sin3dm_amd import _lib
        m = self.model
        lib = m._ensure_handle()
        self.buf = torch.empty_like(x)
        t = timesteps.to(device=x.device, dtype=torch.float32).contiguous()
        with torch.cuda.device(x.device):
            film, stride = m._film_for(lib, timesteps.host_values, t)
            _lib.check(lib.s3d_unet_step_film(m._handle, _lib.ptr(film), stride, x.shape[0], int(H), int(W), int(D), C.byref(step),
                                              _lib.ptr(self.buf), _lib.stream_ptr()))


# ---------------------------------------------------------------------------------------------------- the sequences
S_A, S_MIN, S_ODD, S_EVEN, S_128 = (12, 9, 7), (2, 2, 2), (17, 33, 9), (16, 32, 8), (8, 12, 4)


def shapes_and_batches():
    """Group 1: shrink, grow, and return to a measured key after the buffer moved."""
    return [forward(S_A, 2, 11), forward(S_MIN, 1, 12), forward(S_ODD, 1, 13), forward(S_A, 2, 11), forward(S_A, 3, 14),
            forward(S_A, 1, 15), poison(S_ODD, 3), forward(S_A, 2, 11)]


def modes_at_one_shape(width):
    """Group 2.  At width 32 the generic output head takes a workspace buffer for a fused step without a caller buffer (the
    1 << 40 bit of the key): the two step forms alternate twice."""
    h, B = S_A, 2
    seq = [forward(h, B, 21), forward_host_t(h, B, 21, (999.0, 3.0)), forward_host_t(h, B, 22, (500.0, 500.0)),
           step(h, B, 23, 9), step(h, B, 23, 9, buf=True)]
    if width == 32:
        seq += [step(h, B, 24, 5), step(h, B, 24, 5, buf=True)]
    seq += [mean_only(h, B, 25, 7), step(h, B, 26, 4, mode="ddim", eta=0.7), step(h, B, 27, 4, mode="ddim", inpaint="mask"),
            step(h, B, 27, 4, mode="ddim", inpaint="mask_t0"), step(h, B, 28, 700, px=False, clip=False), step(h, B, 29, 0),
            poison(h, B), forward(h, B, 21)]
    return seq


def carry_cases(hwd, B):
    """Group 3: {case: sequence}.  Every sequence has a CARRY_OUT step, the case's disturbance, then the CARRY_IN step on that
    step's sample.  The poison is itself a forward and would void the carry: where the disturbance is a forward anyway (b, c, g) it
    follows it, at the step's own shape and batch (no growth, which would void the carry by another route); elsewhere it comes
    before the pair, so that what the disturbance ought to drop is still there to be taken by mistake."""
    w_in = "in_conv.0.conv_xz.weight"

    def seq(middle, clone=False, pre=(), poison_between=False):
        s = list(pre) + [forward(hwd, B, 31)] + ([] if poison_between else [poison(hwd, B)])
        s.append(step(hwd, B, 32, 9, carry=CARRY_OUT))
        i = len(s) - 1
        s += list(middle) + ([poison(hwd, B)] if poison_between else [])
        s.append(step(hwd, B, 33, 8, carry=CARRY_OUT | CARRY_IN, x_from=i, clone=clone))
        return s

    return {
        "a_taken": seq([]),
        "b_other_shape": seq([forward(S_MIN, 1, 34)], poison_between=True),
        "c_same_shape": seq([forward(hwd, B, 35)], poison_between=True),
        "d_set_param": seq([set_weights(tensor=w_in, add=0.125, how="inplace")]),
        "e_flat_repack": seq([set_weights(tensor=w_in, add=0.125, how="inplace")], pre=[attach_flat()]),
        "f_lane": seq([lane(1)]),
        "g_bigger_batch": seq([forward(hwd, B + 2, 36)], poison_between=True),
        "h_clone": seq([], clone=True),
        "i_option": seq([option("GN_FUSED", "0")], pre=[option("GN_FUSED", "1")]),
    }


def live_option(hwd, B, name, value, as_loop):
    """Group 4: default -> option -> default -> option on one handle, as forwards or as carried two-step loops."""
    s = []
    for k, v in enumerate((None, value, None, value)):
        if k:
            s.append(option(name, v))
        if k == 3:
            s.append(poison(hwd, B))
        seed = 41 + (k & 1)
        if as_loop:
            s.append(step(hwd, B, seed, 9, carry=CARRY_OUT))
            s.append(step(hwd, B, 43, 8, carry=CARRY_IN, x_from=len(s) - 1))
        else:
            s.append(forward(hwd, B, seed))
    return s


def train_then_infer_then_train(hwd, B):
    """Group 5a: the arena moves under the training tier's measurement."""
    big = tuple(2 * v + 1 for v in hwd)
    return [train(hwd, B, 51, (700, 3)), forward(big, B + 1, 52), train(hwd, B, 51, (700, 3))]


def sample_between_train_steps(hwd, B):
    """Group 5b: TrainLoop._sample_and_visualize's pattern, a carried six-step loop between two train steps."""
    s = [train(hwd, B, 51, (700, 3)), step(hwd, B, 53, 9, carry=CARRY_OUT)]
    for n in range(1, 6):
        s.append(step(hwd, B, 53 + n, 9 - n, carry=(CARRY_OUT if n < 5 else 0) | CARRY_IN, x_from=len(s) - 1))
    return s + [train(hwd, B, 51, (700, 3))]


def live_training_option(hwd, B, name, value):
    """Group 5e: default -> option -> default on a live training handle."""
    return [train(hwd, B, 51, (700, 3)), option(name, value), train(hwd, B, 51, (700, 3)), option(name, None),
            train(hwd, B, 51, (700, 3))]


def parameter_sync(kind):
    """Group 6: the weights of a live model change; forward, forward with host timesteps and a carried loop follow."""
    h, B = S_A, 2
    w = "input_blocks.0.0.emb_layers.1.weight"             # (a FiLM weight: a stale FiLM table would show)
    change = {"load_state_dict": [set_weights(seed=1)],
              "inplace": [set_weights(tensor=w, add=0.0625, how="inplace")],
              "to_roundtrip": [set_weights(tensor=w, add=0.0625, how="to_roundtrip")],
              "load_on_lane_2": [lane(2), set_weights(seed=1)]}[kind]
    s = [forward_host_t(h, B, 61, (500.0, 500.0)), forward_host_t(h, B, 61, (999.0, 3.0)), step(h, B, 62, 9)]
    s += change
    s += [forward(h, B, 61), forward_host_t(h, B, 61, (500.0, 500.0)), forward_host_t(h, B, 61, (999.0, 3.0)),
          poison(h, B), step(h, B, 62, 9, carry=CARRY_OUT)]
    s.append(step(h, B, 63, 8, carry=CARRY_IN, x_from=len(s) - 1))
    return s
