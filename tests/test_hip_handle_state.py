"""What a handle remembers between calls ("What a handle remembers"): sequences of calls on ONE live handle against
each step run alone on a fresh handle (tests/handle_sequences.py).  Every comparison is torch.equal or an asserted error message;
there is no tolerance in this file.  The product keeps one handle through a 1000-step loop, through sampling in the middle of
training, through lanes and through s3d_set_option; the rest of the suite builds a fresh model per case."""
import ctypes as C

import numpy as np
import pytest
import torch

import handle_sequences as hs
from conftest import REPO  # noqa: F401
from sin3dm_amd import testing as T

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def backend():
    b = hs.GpuBackend()
    yield b
    b.clear_options()


@pytest.fixture(scope="module")
def cache():
    return {}                              # step signature -> fresh-handle outputs, shared by every test of the module


def _cfg(mc):
    return dict(mc=mc, cm=(1, 2))


# ------------------------------------------------------------------ 1
@pytest.mark.parametrize("mc", [32, 64])
def test_shapes_and_batches_on_one_handle(backend, cache, mc):
    """(12, 9, 7) B2 -> (2, 2, 2) B1 -> (17, 33, 9) B1 -> (12, 9, 7) B2 -> B3 -> B1 -> poison (17, 33, 9) B3 -> (12, 9, 7) B2:
    the workspace shrinks, grows and returns to a key measured before the buffer moved; ragged planes take the skip-size resize."""
    hs.check_sequence(backend, _cfg(mc), hs.shapes_and_batches(), cache)


# ------------------------------------------------------------------ 2
@pytest.mark.parametrize("mc", [32, 64])
def test_modes_at_one_shape(backend, cache, mc):
    """forward with a device t; with HostTimesteps (mixed and equal values: the FiLM cache); the fused DDPM step without and with
    a caller buffer for the model output (width 32: the generic head takes one from the workspace, twice back and forth);
    MEAN_ONLY; DDIM with eta; both in-painting branches; EPSILON unclipped; t = 0; poison; forward again."""
    hs.check_sequence(backend, _cfg(mc), hs.modes_at_one_shape(mc), cache)


# ------------------------------------------------------------------ 3
@pytest.mark.parametrize("mc,hwd,B", [(64, hs.S_A, 2), (64, hs.S_EVEN, 1), (128, hs.S_128, 1)])
@pytest.mark.parametrize("case", ["a_taken", "b_other_shape", "c_same_shape", "d_set_param", "e_flat_repack", "f_lane",
                                  "g_bigger_batch", "h_clone", "i_option"])
def test_carry_hygiene(backend, cache, case, mc, hwd, B):
    """A CARRY_OUT step, a disturbance, then a CARRY_IN step on that step's sample: a. none (the carried in_conv is taken);
    b. a forward of another shape; c. of the same shape; d. in_conv's weight changed through s3d_unet_set_param; e. the same on a
    flat-attached handle through s3d_unet_repack; f. lane 1 selected, same pointer; g. a larger batch that moves the workspace;
    h. x a clone of the sample; i. GN_FUSED 1 -> 0 (a bit-identical form, another workspace layout).  The poison is a
    forward and voids a carry by itself: in b, c and g it follows the intervening forward (at the step's own size, so that
    nothing grows), and a carry taken after all reads NaN; elsewhere it precedes the pair, and a carry taken after all reads the
    old weights' tensor (d, e).  d and e are held to fresh models with the new weights.  (d found one: s3d_unet_film, which a
    step calls before its forward, packed the new weights without dropping the carry; pack_all drops it now.)
    Whether in_conv was launched cannot be seen from here: s3d_unet_profile brackets the convolution classes only and in_conv is
    none of them, so without a new ABI entry there is no assertion that (a) skipped the kernel and the others did not."""
    hs.check_sequence(backend, _cfg(mc), hs.carry_cases(hwd, B)[case], cache)


# ------------------------------------------------------------------ 4
@pytest.mark.parametrize("mc,hwd", [(64, hs.S_EVEN), (128, hs.S_128)])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("name,value", hs.INFERENCE_OPTIONS, ids=[f"{n}={v}" for n, v in hs.INFERENCE_OPTIONS])
def test_options_on_a_live_inference_handle(backend, cache, name, value, mc, hwd, B):
    """default -> option -> default -> option on one handle, as forwards and as carried two-step loops: every result equals a fresh
    handle created under that option, also for the forms whose rounding differs from the default's.  The options decide what the
    forward allocates (VCAT=0 materialises the concat, CONV_IMPL=naive and WINO change the partial-sum records, GN_FUSED=0 adds the
    ahead-of-consumer statistics, RANK1_SLICES the table slices): a handle that kept its measurement across s3d_set_option ran
    past it — by more than the reservation's slack for CONV_IMPL=naive at every width (DESIGN.md has the sizes)."""
    for as_loop in (False, True):
        hs.check_sequence(backend, _cfg(mc), hs.live_option(hwd, B, name, value, as_loop), cache)


# ------------------------------------------------------------------ 5
TRAIN_HWD, TRAIN_B = (9, 13, 7), 2


@pytest.mark.parametrize("mc", [32, 64])
def test_train_then_inference_then_train(backend, cache, mc):
    """A train step, an inference forward at a larger shape (the arena moves), the same train step: the same loss terms and flat
    gradient bits as the first time and as a fresh handle."""
    _, outs = hs.check_sequence(backend, _cfg(mc), hs.train_then_infer_then_train(TRAIN_HWD, TRAIN_B), cache, inference=False)
    assert all(torch.equal(a, b) for a, b in zip(outs[0], outs[2]))


@pytest.mark.parametrize("mc", [32, 64])
def test_sampling_between_two_train_steps(backend, cache, mc):
    """TrainLoop._sample_and_visualize's pattern: a six-step carried sampling loop on the training handle between two train steps.
    The samples equal a fresh inference model's, the second train step equals the first."""
    _, outs = hs.check_sequence(backend, _cfg(mc), hs.sample_between_train_steps(TRAIN_HWD, TRAIN_B), cache, inference=False)
    assert all(torch.equal(a, b) for a, b in zip(outs[0], outs[-1]))


def _train_inputs(mc, seed=51):
    H, W, D = TRAIN_HWD
    dev = torch.device("cuda:0")
    x0 = torch.from_numpy(T.synthetic_noise((TRAIN_B, 12, H + D, W + D), seed)).clamp(-1, 1).to(dev)
    noise = torch.from_numpy(T.synthetic_noise((TRAIN_B, 12, H + D, W + D), seed + 1)).to(dev)
    return x0, noise, torch.tensor([700, 3], device=dev), torch.tensor([1.0, 0.5], device=dev), dict(H=H, W=W, D=D)


@pytest.mark.parametrize("mc", [32, 64])
def test_inference_between_forward_train_and_backward_is_refused(backend, mc):
    """forward_train, an inference forward (it reuses the tape's workspace), backward_flat: refused by message."""
    m = backend.make_model(_cfg(mc), (("seed", 0),))
    x0, noise, t, w, kw = _train_inputs(mc)
    out = m.forward_train(x0, t.float(), **kw)
    with torch.no_grad():
        m(x0, t.float(), **kw)
    with pytest.raises(AssertionError, match="no forward_train activations"):
        m.backward_flat(torch.ones_like(out))


@pytest.mark.parametrize("mc", [32, 64])
def test_inference_after_an_optimizer_step_sees_the_new_weights(backend, mc):
    """FlatAdamW.step writes the flat vector behind the module's back (mark_parameters_changed): inference on the same object —
    forward, forward with host timesteps (FiLM cache filled BEFORE the step), a carried two-step loop — equals a fresh model
    loaded from state_dict()."""
    from sin3dm_amd.diffusion.train_util import FlatAdamW
    m = backend.make_model(_cfg(mc), (("seed", 0),))
    x0, noise, t, w, kw = _train_inputs(mc)
    diff = backend._diffusion(True, "")
    steps = [hs.forward(TRAIN_HWD, TRAIN_B, 71), hs.forward_host_t(TRAIN_HWD, TRAIN_B, 71, (500.0, 500.0)),
             hs.step(TRAIN_HWD, TRAIN_B, 72, 9, carry=hs.CARRY_OUT)]
    for s in steps:
        backend.run(m, s)                                               # (fills the FiLM cache and leaves a carry behind)
    opt = FlatAdamW(m, lr=1e-2, weight_decay=0.01, ema_rates=[0.99])
    _, g = diff.training_losses_and_grads(m, x0, t, w, kw, noise=noise)
    opt.step(g)
    fresh = backend.make_model(_cfg(mc), (("seed", 0),))
    fresh.load_state_dict({k: v.detach().clone() for k, v in m.state_dict().items()})
    assert not torch.equal(dict(m.named_parameters())["out.2.conv_xy.weight"].cpu(),
                           backend.state_dict(_cfg(mc), (("seed", 0),))["out.2.conv_xy.weight"])
    for s in steps:
        a, b = backend.run(m.eval(), s), backend.run(fresh, s)
        assert all(torch.equal(u, v) for u, v in zip(a, b)), s
    a = backend.run(m, dict(steps[2], seed=73, ti=8, carry=hs.CARRY_IN), a[0])
    b = backend.run(fresh, dict(steps[2], seed=73, ti=8, carry=0), b[0])
    assert all(torch.equal(u, v) for u, v in zip(a, b))


@pytest.mark.parametrize("mc", [32, 64])
@pytest.mark.parametrize("name,value", hs.TRAINING_OPTIONS, ids=[f"{n}={v}" for n, v in hs.TRAINING_OPTIONS])
def test_options_on_a_live_training_handle(backend, cache, name, value, mc):
    """default -> option -> default on one attached handle.  GNB_FUSED=0, BWD_SIDE=0, EDGE_SIGNAL=0 and WGRAD_WINO=0 change the
    backward pass's kernels, streams and workspace but read no weight image the repack plan drops: none is refused, and each
    step equals a fresh handle attached under that option, bit for bit (loss terms and flat gradient).  (WINO / CONV_IMPL, which do
    read other images, stay refused: test_a_form_change_after_attach_fails_instead_of_using_stale_weights.)"""
    hs.check_sequence(backend, _cfg(mc), hs.live_training_option(TRAIN_HWD, TRAIN_B, name, value), cache, inference=False)


# ------------------------------------------------------------------ 6
@pytest.mark.parametrize("kind", ["load_state_dict", "inplace", "to_roundtrip", "load_on_lane_2"])
def test_parameter_sync_of_the_python_mirror(backend, cache, kind):
    """The weights of a live model change — load_state_dict of other weights, an in-place update of one FiLM weight, a .to() round
    trip with the edit made on the CPU, load_state_dict while lane 2 is selected — after the FiLM cache was filled and a step
    ran.  forward, forward with HostTimesteps (equal and mixed values) and a carried loop then equal a fresh model's."""
    hs.check_sequence(backend, _cfg(32), hs.parameter_sync(kind), cache)


# ------------------------------------------------------------------ 7: the other handles
def _decoder(variant):
    from sin3dm_amd.encoding.networks import AutoEncoderGroupSkip, AutoEncoderGroupPBR
    import pbr_cases as pc
    kind = {0: "skip", 1: "geo", 2: "pbr"}[variant]
    cls = AutoEncoderGroupPBR if variant == 2 else AutoEncoderGroupSkip
    net = cls(4, 8, 32, 64, 4, use_tex=variant != 1, tex_channels=8 if variant == 2 else 3)
    missing, unexpected = net.load_state_dict(pc.weights(kind, 32, 64, dtype=torch.float32), strict=False)
    assert not unexpected and all(k == "aabb" or "encoder" in k for k in missing), missing
    net = net.to(torch.device("cuda:0"))
    net.reset_aabb(torch.tensor(pc.AABB))
    assert net.variant == variant
    return net


@pytest.mark.parametrize("variant", [0, 1, 2])
def test_decoder_handle_across_triplanes(variant):
    """prepare_triplane with (20, 12, 16) planes, decode 257 points; prepare with (6, 8, 5), decode 33 points, decode_grid at
    reso 12; and back: every output equals a fresh decoder's."""
    import pbr_cases as pc
    dev = torch.device("cuda:0")
    C_in = 4 if variant == 1 else 12
    fms = {hwd: [torch.from_numpy(p).to(dev) for p in pc.synthetic_planes(*hwd, C=C_in, seed=40 + hwd[0])]
           for hwd in ((20, 12, 16), (6, 8, 5))}
    lo, hi = np.asarray(pc.AABB[:3]), np.asarray(pc.AABB[3:])

    def pts(n, seed):
        u = np.random.Generator(np.random.PCG64(seed)).uniform(-1.1, 1.1, size=(n, 3))
        return torch.from_numpy((lo + (u + 1) / 2 * (hi - lo)).astype(np.float32)).to(dev)

    calls = [("decode", (20, 12, 16), pts(257, 1)), ("decode", (6, 8, 5), pts(33, 2)), ("grid", (6, 8, 5), 12),
             ("decode", (20, 12, 16), pts(257, 1)), ("grid", (20, 12, 16), 12)]

    def run(net, call):
        kind, hwd, arg = call
        with torch.no_grad():
            return net.decode(arg, fms[hwd]) if kind == "decode" else net.decode_grid(fms[hwd], arg)

    live = _decoder(variant)
    outs = [run(live, c).clone() for c in calls]
    for c, o in zip(calls, outs):
        assert torch.isfinite(o).all() and torch.equal(o, run(_decoder(variant), c)), (variant, c[0], c[1])
    assert torch.equal(outs[0], outs[3])


def test_marching_cubes_handle_across_grids(oracle):
    """One s3d_mc handle: 33x20x27 noise -> 9x7x5 without a surface -> 14x11x9 noise with three attributes -> the first again,
    each equal to the C restatement; and a count without an extract followed by another count."""
    from sin3dm_amd import _lib
    from sin3dm_amd.encoding.isosurface import marching_cubes
    rng = np.random.Generator(np.random.PCG64(6))
    big = rng.standard_normal((33, 20, 27)).astype(np.float32)
    empty = np.full((9, 7, 5), 2.0, dtype=np.float32)
    att = rng.standard_normal((14, 11, 9, 4)).astype(np.float32)
    for f, n_attr in ((big, 0), (empty, 0), (att, 3), (big, 0)):
        field = f[..., 0] if f.ndim == 4 else f
        v_ref, t_ref = oracle.marching_cubes(np.ascontiguousarray(field), 0.0, 1.0)
        v, t, a = marching_cubes(torch.from_numpy(f).cuda(), 0.0, 1.0, n_attr=n_attr)
        assert np.array_equal(t.cpu().numpy().reshape(-1, 3), t_ref.reshape(-1, 3)) and np.array_equal(v.cpu().numpy().reshape(-1, 3), v_ref.reshape(-1, 3))
        assert (len(t_ref) == 0) == (f is empty)
        if n_attr:
            assert a.shape == (len(v_ref), 3) and torch.isfinite(a).all()
    lib = _lib.load()
    h = C.c_void_p()
    _lib.check(lib.s3d_mc_create(C.byref(h)))
    try:
        counts = []
        for f in (big, att[..., 0].copy(), big):
            g = torch.from_numpy(f).cuda()
            nv, nt = C.c_int64(), C.c_int64()
            _lib.check(lib.s3d_mc_count(h, _lib.ptr(g), *f.shape, 1, 0.0, 1, 1.0, C.byref(nv), C.byref(nt), _lib.stream_ptr()))
            torch.cuda.synchronize()
            counts.append((nv.value, nt.value, len(oracle.marching_cubes(f, 0.0, 1.0)[1])))
        assert all(c[1] == c[2] for c in counts) and counts[0] == counts[2], counts
    finally:
        lib.s3d_mc_destroy(h)


def test_autoencoder_handle_across_volumes():
    """s3d_ae_set_volume large then small on one handle, N 4096 then 130 (test_hip_ae_reference.py changes the batch, not the
    volume): encode, the training forward, losses and flat gradient equal a fresh handle's."""
    from sin3dm_amd.encoding.model import ae_loss_cfg
    from sin3dm_amd.encoding.networks import AutoEncoderGroupSkip
    cfg, aabb, dev = (4, 8, 32, 64, 4, 3), (-0.7, -1.0, -0.45, 0.7, 1.0, 0.45), torch.device("cuda:0")
    sd = T.synthetic_state_dict(T.ae_param_shapes(*cfg, with_encoder=True), 3)
    lc = ae_loss_cfg("weightedl1", "l1", 0.05, 0.999, 1.0, False)

    def net():
        n = AutoEncoderGroupSkip(*cfg[:5], tex_channels=cfg[5]).to(dev)
        n.load_state_dict(sd, strict=False)
        n.reset_aabb(torch.tensor(aabb))
        return n

    def case(hwd, N, seed):
        H, W, D = hwd
        vol = torch.tanh(torch.from_numpy(T.synthetic_noise((1, 4, 2 * H, 2 * W, 2 * D), seed)))
        vol[:, 1:] = 0.5 * vol[:, 1:] + 0.5
        rng = np.random.Generator(np.random.PCG64(seed))
        lo, hi = np.asarray(aabb[:3]), np.asarray(aabb[3:])
        pts = (lo + rng.uniform(-0.075, 1.075, size=(N, 3)) * (hi - lo)).astype(np.float32)
        sdf = rng.normal(0, 0.03, size=(N, 1)).astype(np.float32)
        tex = rng.uniform(0, 1, size=(N, 3)).astype(np.float32)
        return tuple(torch.from_numpy(a).to(dev) if isinstance(a, np.ndarray) else a.to(dev) for a in (vol, pts, sdf, tex))

    def run(n, c):
        vol, pts, sdf, tex = c
        with torch.no_grad():
            fm = n.encode(vol)
            pred = n(vol, pts)
        losses, _, g = n.loss_and_grads(vol, pts, sdf, tex, lc)
        return [f.clone() for f in fm] + [pred.clone(), losses.clone(), g.clone()]

    cases = [case((13, 16, 11), 4096, 81), case((3, 4, 5), 130, 82), case((13, 16, 11), 4096, 81)]
    live = net()
    outs = [run(live, c) for c in cases]
    for i, (c, o) in enumerate(zip(cases, outs)):
        ref = run(net(), c)
        assert all(torch.isfinite(a).all() and torch.equal(a, b) for a, b in zip(o, ref)), i
