"""GPU: torch's CPU noise stream generated on the device (s3d_rng.hip behind sin3dm_amd/diffusion/cpu_stream.py) against live
CPU torch and the recorded draws, and "same seed => same sample": the sampling loops with generator=TorchCpuStream(k) against
SEEDED runs of the reference (tests/golden/seeded.npz: torch.manual_seed(k), then the reference's own loops, nothing patched)."""
import os

import numpy as np
import pytest
import torch

from conftest import golden, relerr
from sin3dm_amd import testing as T
from sin3dm_amd.diffusion.cpu_stream import TorchCpuStream, words_per_call

pytestmark = pytest.mark.gpu

# Derived, not tuned: |z| <= sqrt(-2 ln 2^-24) = 5.77 < 8, one ulp there is 4.77e-7, and the float32 chain log -> mul -> sqrt,
# mul -> cos, mul is allowed 8 ulp of the result (an independent numpy model sits at one ulp against torch)
RANDN_TOL = 4e-6
TRAJ_TOL = 2e-4             # the gate of the stored-noise trajectories (README.md "Parity", test_hip_parity.py)


def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def make_model(mc=32):
    from sin3dm_amd.diffusion.unet_triplane import TriplaneUNetModelSmall
    m = TriplaneUNetModelSmall(12, mc, 12, use_scale_shift_norm=True)
    m.load_state_dict(T.synthetic_state_dict(T.unet_param_shapes(model_channels=mc), 0))
    return m.to(dev()).eval()


def make_diffusion(resp):
    from sin3dm_amd.diffusion.script_util import create_gaussian_diffusion
    return create_gaussian_diffusion(steps=1000, noise_schedule="linear", predict_xstart=True, timestep_respacing=resp)


def check_randn(got, ref, what):
    got, ref = np.asarray(got).reshape(-1), np.asarray(ref).reshape(-1)
    err = float(np.max(np.abs(got - ref)))
    same = float(np.mean(got == ref))
    print(f"{what}: randn max-abs {err:.3e}, bit-equal {same:.4f}")
    assert err <= RANDN_TOL, what
    assert same >= 0.5, what              # a wrong pairing or a wrong tail leaves ~0


# ------------------------------------------------------------------ the stream itself
@pytest.mark.parametrize("n", [16, 3420, 3840, 786432])
def test_rand_is_bit_equal_to_cpu_torch(n):
    torch.manual_seed(11 + n)
    ref = torch.rand(n)
    got = TorchCpuStream(11 + n, device=dev()).rand(n)
    assert got.device.type == "cuda" and got.dtype == torch.float32 and got.shape == (n,)
    assert torch.equal(got.cpu(), ref)


def test_rand_sequence_of_mixed_sizes_is_bit_equal():
    """calls that start mid-block, straddle the 624-word block boundary, end on it, and odd sizes (the scalar stores)"""
    sizes = (5, 600, 19, 624, 1, 1247, 3420, 623, 2, 100000, 7)
    torch.manual_seed(3)
    s = TorchCpuStream(3, device=dev())
    for n in sizes:
        assert torch.equal(s.rand(n).cpu(), torch.rand(n)), n
    key, pos = s.get_state()
    assert pos == (sum(sizes) - 1) % 624 + 1


@pytest.mark.parametrize("n", [16, 20, 1003, 3420, 3840, 786432])
def test_randn_against_cpu_torch(n):
    torch.manual_seed(21 + n)
    ref = torch.randn(n)
    after = torch.rand(4)
    s = TorchCpuStream(21 + n, device=dev())
    got = s.randn((n,))
    check_randn(got.cpu().numpy(), ref.numpy(), f"n={n}")
    assert torch.equal(s.rand(4).cpu(), after)           # n + 16 * (n % 16 != 0) words consumed


def test_randn_against_the_recorded_stream():
    g = golden("seeded")
    for tag, n in (("n3840", 3840), ("n3420", 3420)):
        s = TorchCpuStream(int(g[f"{tag}.seed"]), device=dev())
        check_randn(s.randn((n,)).cpu().numpy(), g[f"{tag}.randn"], f"seeded.npz {tag}")
        assert np.array_equal(s.rand(4).cpu().numpy(), g[f"{tag}.rand_after"])
        s.manual_seed(int(g[f"{tag}.seed"]))             # reuse
        assert np.array_equal(s.rand(n).cpu().numpy(), g[f"{tag}.rand"])


def test_randn_lead_chunks_and_batch_forms():
    """lead=k is k consecutive calls (each 3420-element call has its own tail); [B, ...] is ONE call of B times the elements,
    B x [1, ...] from B streams are B batch-1 calls"""
    from sin3dm_amd.diffusion.gaussian_diffusion import GaussianDiffusion as GD
    shape1, k = (1, 12, 15, 19), 5
    torch.manual_seed(8)
    ref = torch.stack([torch.randn(shape1) for _ in range(k)])
    after = torch.rand(4)
    s = TorchCpuStream(8, device=dev())
    got = s.randn(shape1, lead=k)
    assert got.shape == (k,) + shape1 and got.is_contiguous()
    check_randn(got.cpu().numpy(), ref.numpy(), "lead=5 x 3420")
    assert torch.equal(s.rand(4).cpu(), after)
    # chunked = call by call, bit for bit
    s2 = TorchCpuStream(8, device=dev())
    one_by_one = torch.stack([s2.randn(shape1) for _ in range(k)])
    assert torch.equal(one_by_one, got)
    # one stream, batch 2: one call of the whole tensor
    shape2 = (2, 12, 15, 19)
    torch.manual_seed(9)
    ref2 = torch.randn(shape2)
    got2 = GD._randn(shape2, dev(), TorchCpuStream(9), lead=None)
    check_randn(got2.cpu().numpy(), ref2.numpy(), "[2, ...] as one call")
    # two streams: sample b is the batch-1 call of stream b
    per = GD._randn(shape2, dev(), [TorchCpuStream(9), TorchCpuStream(10)], lead=3)
    assert per.shape == (3,) + shape2 and per.is_contiguous()
    for b, seed in enumerate((9, 10)):
        torch.manual_seed(seed)
        refb = torch.stack([torch.randn(shape1) for _ in range(3)])
        check_randn(per[:, b].cpu().numpy(), refb[:, 0].numpy(), f"per-sample stream {b}")


def test_randn_refuses_fewer_than_16_elements_in_the_library():
    import ctypes as C
    from sin3dm_amd import _lib
    lib = _lib.load()
    h = C.c_void_p()
    assert lib.s3d_rng_create(C.byref(h)) == 0
    out = torch.empty(64, device=dev())
    key = np.zeros(624, dtype=np.uint32)
    assert lib.s3d_rng_randn(h, _lib.ptr(out), 64, 1, None) == _lib.ERR_INVALID            # no state yet
    assert lib.s3d_rng_set_state(h, key.ctypes.data_as(C.POINTER(C.c_uint32)), 625, None) == _lib.ERR_INVALID
    assert lib.s3d_rng_set_state(h, key.ctypes.data_as(C.POINTER(C.c_uint32)), 624, None) == 0
    assert lib.s3d_rng_randn(h, _lib.ptr(out), 64, 1, None) == _lib.ERR_INVALID            # nothing reserved: no allocation in the launch path
    assert b"s3d_rng_reserve" in lib.s3d_last_error()
    assert lib.s3d_rng_reserve(h, 64) == 0
    assert lib.s3d_rng_randn(h, _lib.ptr(out), 15, 1, None) == _lib.ERR_UNSUPPORTED
    assert lib.s3d_rng_randn(h, _lib.ptr(out), 64, 1, None) == 0
    torch.cuda.synchronize()
    lib.s3d_rng_destroy(h)


def test_state_hand_over_to_and_from_torch():
    """TorchCpuStream(seed=None) continues torch's CPU generator where it stands; sync_to_torch() hands the advanced state back."""
    torch.manual_seed(123)
    torch.randn(1000)
    torch.rand(37)
    state = torch.get_rng_state()
    ref = torch.randn(3420)
    ref_after = torch.rand(4)
    torch.set_rng_state(state)
    s = TorchCpuStream(device=dev())
    got = s.randn((3420,))
    check_randn(got.cpu().numpy(), ref.numpy(), "adopted state")
    assert torch.equal(torch.get_rng_state(), state)     # torch's own generator has not moved yet
    s.sync_to_torch()
    assert torch.equal(torch.rand(4), ref_after)


# ------------------------------------------------------------------ same seed => same sample
CASES = ["ddpm20_b2", "ddim10_b1", "ddpm100_b1", "ddpm1000_b1", "ddpm20_b1_s0", "ddpm20_b1_s1"]


def run_case(g, tag, model, generator=None, diff=None, **kw):
    B, H, W, D = (int(v) for v in g[f"{tag}.bhwd"])
    diff = diff or make_diffusion(str(g[f"{tag}.respacing"]))
    gen = generator if generator is not None else TorchCpuStream(int(g[f"{tag}.seed"]))
    fn = diff.ddim_sample_loop if int(g[f"{tag}.ddim"]) else diff.p_sample_loop
    return fn(model, (B, 12, H + D, W + D), model_kwargs=dict(H=H, W=W, D=D), generator=gen, **kw), gen


@pytest.mark.parametrize("tag", CASES)
def test_seeded_trajectory_matches_the_reference(tag):
    g = golden("seeded")
    B, H, W, D = (int(v) for v in g[f"{tag}.bhwd"])
    final, gen = run_case(g, tag, make_model())
    final = final.cpu().numpy()
    e = relerr(final, g[f"{tag}.final"])
    print(f"{tag}: seeded trajectory relerr {e:.3e}")
    assert e <= TRAJ_TOL
    assert np.all(final[..., H:, W:] == 0), "DxD corner must end at exactly 0"
    # the stream stands where the reference's generator stood after its loop: T + 1 calls, DDIM included
    assert np.array_equal(gen.rand(4).cpu().numpy(), g[f"{tag}.rand4"])


def test_seeded_trajectory_per_sample_streams():
    """a list of B streams: sample b is the reference run at batch 1 after manual_seed of ITS seed"""
    g = golden("seeded")
    tags = ("ddpm20_b1_s0", "ddpm20_b1_s1")
    B, H, W, D = (int(v) for v in g["ddpm20_b2.bhwd"])
    gens = [TorchCpuStream(int(g[f"{t}.seed"])) for t in tags]
    diff = make_diffusion("20")
    final = diff.p_sample_loop(make_model(), (B, 12, H + D, W + D), model_kwargs=dict(H=H, W=W, D=D), generator=gens).cpu().numpy()
    for b, t in enumerate(tags):
        e = relerr(final[b:b + 1], g[f"{t}.final"])
        print(f"per-sample stream {t}: relerr {e:.3e}")
        assert e <= TRAJ_TOL
        assert np.array_equal(gens[b].rand(4).cpu().numpy(), g[f"{t}.rand4"])
    assert np.all(final[..., H:, W:] == 0)


def test_sync_to_torch_after_a_loop_continues_the_reference_sequence():
    g = golden("seeded")
    tag = "ddim10_b1"
    _, gen = run_case(g, tag, make_model())
    gen.sync_to_torch()
    assert np.array_equal(torch.rand(4).numpy(), g[f"{tag}.rand4"])


def test_caller_noise_replaces_x_T_and_x_T_is_not_drawn():
    """noise= given: the reference does not draw x_T (:511-514); the stream then holds T calls, not T + 1"""
    g = golden("seeded")
    tag = "ddim10_b1"
    B, H, W, D = (int(v) for v in g[f"{tag}.bhwd"])
    shape = (B, 12, H + D, W + D)
    xT = torch.from_numpy(T.synthetic_noise(shape, 5)).to(dev())
    _, gen = run_case(g, tag, make_model(), noise=xT)
    m = T.TorchCpuStreamModel(int(g[f"{tag}.seed"]))
    m.rand(words_per_call(int(np.prod(shape))) * 10)
    assert np.array_equal(gen.rand(4).cpu().numpy(), m.rand(4))


@pytest.mark.parametrize("tag", ["ddpm20_b2", "ddim10_b1"])
def test_overlap_and_chunk_length_do_not_change_the_bits(tag):
    g = golden("seeded")
    model = make_model()
    finals = {}
    for name, overlap, ahead in (("overlap", True, None), ("inline", False, None), ("chunk1", True, 0), ("chunk1_inline", False, 0),
                                 ("chunk3", True, 3)):
        diff = make_diffusion(str(g[f"{tag}.respacing"]))
        diff._CPU_STREAM_OVERLAP = overlap
        if ahead is not None:
            B, H, W, D = (int(v) for v in g[f"{tag}.bhwd"])
            diff._NOISE_AHEAD_BYTES = ahead * 4 * B * 12 * (H + D) * (W + D)
        finals[name], _ = run_case(g, tag, model, diff=diff)
    torch.cuda.synchronize()
    for name, x in finals.items():
        assert torch.equal(x, finals["overlap"]), name
    assert relerr(finals["overlap"].cpu().numpy(), g[f"{tag}.final"]) <= TRAJ_TOL


def test_chains_with_one_stream_per_run_equal_the_runs_alone():
    g = golden("seeded")
    tag = "ddpm20_b1_s0"
    B, H, W, D = (int(v) for v in g[f"{tag}.bhwd"])
    shape = (B, 12, H + D, W + D)
    model = make_model()
    diff = make_diffusion("20")
    seeds = (1000, 1001, 1002)
    alone = [diff.p_sample_loop(model, shape, model_kwargs=dict(H=H, W=W, D=D), generator=TorchCpuStream(s)) for s in seeds]
    chained = diff.sample_loop_chains(model, shape, len(seeds), chains=2, generators=[TorchCpuStream(s) for s in seeds],
                                      device=dev(), model_kwargs=dict(H=H, W=W, D=D))
    torch.cuda.synchronize()
    for a, c in zip(alone, chained):
        assert torch.equal(a, c)
    assert relerr(chained[0].cpu().numpy(), g["ddpm20_b1_s0.final"]) <= TRAJ_TOL
    assert relerr(chained[1].cpu().numpy(), g["ddpm20_b1_s1.final"]) <= TRAJ_TOL


def test_default_generators_are_untouched_by_the_new_source():
    """generator=None / a torch.Generator still draw the device's Philox stream in the loops' chunks"""
    H, W, D = 10, 14, 6
    shape = (1, 12, H + D, W + D)
    model = make_model()
    diff = make_diffusion("10")
    kw = dict(model_kwargs=dict(H=H, W=W, D=D))
    a = diff.p_sample_loop(model, shape, generator=torch.Generator(device=dev()).manual_seed(5), **kw)
    gen = torch.Generator(device=dev()).manual_seed(5)
    xT = torch.randn(shape, device=dev(), generator=gen)
    eps = iter(torch.randn((10,) + shape, device=dev(), generator=gen))
    diff.noise_fn = lambda z: next(eps)
    b = diff.p_sample_loop(model, shape, noise=xT, **kw)
    assert torch.equal(a, b)


# ------------------------------------------------------------------ the sampling CLI
def test_sample_cli_torch_cpu_noise(tmp_path, monkeypatch):
    """S3D_NOISE=torch_cpu: sample i of the CLI is p_sample_loop(generator=TorchCpuStream(sample_seed(base, i))) — whatever batch
    and chain it ran in — on an experiment directory made of the reference's own files (tests/golden/formats/)."""
    from test_formats import reference_experiment
    from sin3dm_amd import parallel, sample
    from sin3dm_amd.diffusion.script_util import create_model_and_diffusion_from_args
    from sin3dm_amd.utils import parser_util as pu
    from sin3dm_amd.utils.triplane_util import decompose_featmaps, load_triplane_data
    tag = reference_experiment(str(tmp_path))
    argv = ["--tag", tag, "--n_samples", "2", "--timestep_respacing", "10"]
    monkeypatch.setenv("S3D_NOISE", "torch_cpu")
    args = pu.sample_args(argv)
    paths = sample.sample_diffusion(args)
    assert [os.path.relpath(p, tag) for p in paths] == [f"{args.output}/000/feat.npz", f"{args.output}/001/feat.npz"]
    monkeypatch.delenv("S3D_NOISE")
    model, diffusion = create_model_and_diffusion_from_args(args)
    model.load_state_dict(torch.load(pu.diffusion_model_path(tag, args.ema_rate, args.diff_n_iters), map_location="cpu"))
    model.to(dev()).eval()
    _, (H, W, D) = load_triplane_data(pu.encoding_feat_path(tag), device=dev())
    direct = diffusion.p_sample_loop(model, [1, 12, H + D, W + D], model_kwargs=dict(H=H, W=W, D=D),
                                     generator=TorchCpuStream(parallel.sample_seed(1000, 1)))
    xy, xz, yz = (t.cpu().numpy()[0] for t in decompose_featmaps(direct, (H, W, D)))
    d = np.load(paths[1])
    assert np.array_equal(d["feat_xy"], xy) and np.array_equal(d["feat_xz"], xz) and np.array_equal(d["feat_yz"], yz)
    # the keyword selects it too, and the default source gives another sample
    again = sample.sample_diffusion(pu.sample_args(argv + ["--output", "kw"]), noise="torch_cpu")
    assert np.array_equal(np.load(again[1])["feat_xy"], xy)
    default = sample.sample_diffusion(pu.sample_args(argv + ["--output", "dev"]))
    assert not np.array_equal(np.load(default[1])["feat_xy"], xy)
