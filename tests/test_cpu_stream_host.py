"""CPU: the host side of torch's CPU noise stream (sin3dm_amd/diffusion/cpu_stream.py) against LIVE torch — seeding, the
generator-state layout in both directions, words per call and the tail rule (through the numpy model of sin3dm_amd.testing, which
the GPU tests hold the kernels against) — and against the recorded draws of tests/golden/seeded.npz; the noise-source switch of
sin3dm_amd.sample."""
import numpy as np
import pytest
import torch

from conftest import golden
from sin3dm_amd import testing as T
from sin3dm_amd.diffusion import cpu_stream as cs

# |z| <= sqrt(-2 ln 2^-24) = 5.77 < 8, one ulp there is 4.77e-7; the float32 chain log -> mul -> sqrt, mul -> cos, mul is allowed
# 8 ulp of the result (the model's vectorised numpy log / cos against torch's: 1 ulp measured)
RANDN_TOL = 4e-6


@pytest.mark.parametrize("seed", [0, 1, 1000, 2 ** 31 + 5, 2 ** 32 - 1, 2 ** 32 + 7, 2 ** 40 + 12345])
def test_init_genrand_is_the_state_after_manual_seed(seed):
    torch.manual_seed(seed)
    key, pos, seed_field = cs.parse_rng_state(torch.get_rng_state())
    mine, mine_pos = cs.init_genrand(seed)
    assert pos == mine_pos == 624                       # freshly seeded: left = 1, next = 0, the words not yet regenerated
    assert np.array_equal(key, mine)
    assert seed_field == seed
    s = cs.TorchCpuStream(seed)                         # nothing touches a device before the first draw
    k2, p2 = s.get_state()
    assert np.array_equal(k2, key) and p2 == 624 and s.initial_seed() == seed


@pytest.mark.parametrize("draws", [0, 1, 37, 623, 624, 625, 1000, 3 * 624])
def test_parse_advance_set_state_roundtrip(draws):
    """torch -> parse -> host MT continues torch's draws bit for bit; host MT advanced -> pack -> set_rng_state -> torch
    continues the host's.  Positions at, before and after a block boundary and the freshly seeded state."""
    torch.manual_seed(99)
    if draws:
        torch.rand(draws)
    state = torch.get_rng_state()
    key, pos, seed = cs.parse_rng_state(state)
    assert pos == (624 if draws == 0 else (draws - 1) % 624 + 1)
    m = T.TorchCpuStreamModel(key=key, pos=pos)
    assert np.array_equal(torch.rand(2000).numpy(), m.rand(2000))
    # the other direction, from a state torch has not seen
    m.rand(777)
    k2, p2 = m.state()
    torch.set_rng_state(cs.pack_rng_state(k2, p2, seed, template=state))
    assert np.array_equal(torch.rand(1500).numpy(), m.rand(1500))
    # a stream adopted from torch's generator (seed=None) starts exactly there and leaves torch's own generator alone
    torch.set_rng_state(state)
    s = cs.TorchCpuStream()
    k3, p3 = s.get_state()
    assert np.array_equal(k3, key) and p3 == pos
    assert torch.equal(torch.get_rng_state(), state)
    # pack without a template parses back
    k4, p4, s4 = cs.parse_rng_state(cs.pack_rng_state(key, pos, 5))
    assert np.array_equal(k4, key) and p4 == pos and s4 == 5


@pytest.mark.parametrize("n", [16, 17, 31, 32, 1003, 3420, 3840, 786432])
def test_model_words_per_call_and_tail_rule_against_live_torch(n):
    seed = 4242 + n
    torch.manual_seed(seed)
    ref = torch.randn(n).numpy()
    after = torch.rand(8).numpy()
    m = T.TorchCpuStreamModel(seed)
    got = m.randn(n)
    assert m.words == cs.words_per_call(n) == n + (16 if n % 16 else 0)
    assert np.array_equal(m.rand(8), after)              # the stream stands where torch's does: the word count is right
    err = float(np.max(np.abs(got - ref)))
    same = float(np.mean(got == ref))
    print(f"n={n}: model vs torch.randn max-abs {err:.3e}, bit-equal {same:.3f}")
    assert err <= RANDN_TOL
    assert same >= 0.5                                   # a wrong pairing or tail leaves ~0


def test_model_rand_is_bit_equal_and_sequences_of_calls():
    torch.manual_seed(7)
    m = T.TorchCpuStreamModel(7)
    for n in (5, 600, 19, 624, 3420, 1):                 # starts mid-block, straddles and ends on block boundaries
        assert np.array_equal(torch.rand(n).numpy(), m.rand(n))
    for n in (3420, 3420, 16, 3840):                     # consecutive randn calls, each with its own tail
        assert float(np.max(np.abs(torch.randn(n).numpy() - m.randn(n)))) <= RANDN_TOL
    assert np.array_equal(torch.rand(4).numpy(), m.rand(4))


def test_model_agrees_with_the_recorded_stream():
    g = golden("seeded")
    for tag, n in (("n3840", 3840), ("n3420", 3420)):
        seed = int(g[f"{tag}.seed"])
        m = T.TorchCpuStreamModel(seed)
        assert np.array_equal(m.rand(n), g[f"{tag}.rand"])
        m = T.TorchCpuStreamModel(seed)
        got = m.randn(n)
        assert float(np.max(np.abs(got - g[f"{tag}.randn"]))) <= RANDN_TOL
        assert float(np.mean(got == g[f"{tag}.randn"])) >= 0.5
        assert np.array_equal(m.rand(4), g[f"{tag}.rand_after"])


def test_recorded_loops_consumed_one_call_per_step_plus_x_T():
    """The rand4 witness stored after every reference loop is the stream after T + 1 calls of the whole [B, ...] tensor
    (DDIM with eta = 0 and t = 0 included): the sequence TorchCpuStream generators reproduce."""
    g = golden("seeded")
    tags = sorted(k[:-len(".bhwd")] for k in g.files if k.endswith(".bhwd"))
    assert len(tags) == 6
    for tag in tags:
        B, H, W, D = (int(v) for v in g[f"{tag}.bhwd"])
        resp = str(g[f"{tag}.respacing"])
        steps = int(resp) if resp else 1000
        m = T.TorchCpuStreamModel(int(g[f"{tag}.seed"]))
        n = B * 12 * (H + D) * (W + D)
        m.rand(cs.words_per_call(n) * (steps + 1))
        assert np.array_equal(m.rand(4), g[f"{tag}.rand4"]), tag


def test_randn_refuses_fewer_than_16_elements_before_touching_a_device():
    with pytest.raises(NotImplementedError):
        cs.TorchCpuStream(1).randn((3, 5))


def test_noise_source_switch(monkeypatch):
    from sin3dm_amd import parallel, sample
    monkeypatch.delenv("S3D_NOISE", raising=False)
    assert sample.noise_source() == "device" and sample.noise_source("torch_cpu") == "torch_cpu"
    monkeypatch.setenv("S3D_NOISE", "torch_cpu")
    assert sample.noise_source() == "torch_cpu" and sample.noise_source("device") == "device"     # the keyword wins
    gens = sample.sample_generators([[0, 1], [2]], "cpu", base_seed=1000)
    assert [[type(g) for g in b] for b in gens] == [[cs.TorchCpuStream] * 2, [cs.TorchCpuStream]]
    assert [[g.initial_seed() for g in b] for b in gens] == [[parallel.sample_seed(1000, 0), parallel.sample_seed(1000, 1)],
                                                            [parallel.sample_seed(1000, 2)]]
    gens = sample.sample_generators([[0, 1]], "cpu", base_seed=1000, noise="device")
    assert all(isinstance(g, torch.Generator) for g in gens[0])
    assert [g.initial_seed() for g in gens[0]] == [1000, 1001]
    monkeypatch.setenv("S3D_NOISE", "philox")
    with pytest.raises(ValueError, match="philox"):
        sample.noise_source()
    monkeypatch.setenv("S3D_NOISE", "")
    assert sample.noise_source() == "device"


def test_randn_dispatch_and_loop_types_without_a_device(monkeypatch):
    """GaussianDiffusion._randn hands a TorchCpuStream one call of the whole [B, ...] tensor and a list of B of them one
    [1, ...] call each (lead = k consecutive calls), recorded by a stand-in for the device draw."""
    from sin3dm_amd.diffusion.gaussian_diffusion import GaussianDiffusion as GD
    calls = []

    def fake(self, shape, lead=None, device=None):
        calls.append((self.initial_seed(), tuple(shape), lead))
        return torch.full((() if lead is None else (lead,)) + tuple(shape), float(self.initial_seed()))
    monkeypatch.setattr(cs.TorchCpuStream, "randn", fake)
    a, b = cs.TorchCpuStream(1), cs.TorchCpuStream(2)
    x = GD._randn((2, 3, 4, 5), "cpu", a)
    assert x.shape == (2, 3, 4, 5) and calls == [(1, (2, 3, 4, 5), None)]
    calls.clear()
    x = GD._randn((2, 3, 4, 5), "cpu", [a, b], lead=7)
    assert calls == [(1, (1, 3, 4, 5), 7), (2, (1, 3, 4, 5), 7)]
    assert x.shape == (7, 2, 3, 4, 5) and float(x[3, 0, 0, 0, 0]) == 1.0 and float(x[3, 1, 0, 0, 0]) == 2.0
    x = GD._randn((1, 3, 4, 5), "cpu", [b])
    assert x.shape == (1, 3, 4, 5)
    assert cs.is_cpu_stream(a) and cs.is_cpu_stream([a, b]) and not cs.is_cpu_stream([torch.Generator()]) and not cs.is_cpu_stream(None)
