"""CPU side of the handle-state tests: the tables of tests/handle_sequences.py against the library's option list, the sequence
runner's own logic on a stub model, and the option entry points after the generation change."""
import ctypes as C
import os
import re

import pytest

import handle_sequences as hs
from conftest import REPO
from sin3dm_amd import _lib


def _library_options():
    txt = open(os.path.join(REPO, "sin3dm_amd", "csrc", "s3d_common.h")).read()
    body = re.search(r"kOptNames\[\]\s*=\s*\{(.*?)\};", txt, re.S).group(1)
    return re.findall(r'"(\w+)"', body)


def test_every_option_is_switched_live_or_excused():
    """A new option cannot arrive untested: each name of kOptNames is switched on a live inference handle (group 4), on a live
    training handle (group 5), or is listed as not applicable with a reason; and the tables name nothing the library lacks."""
    names = _library_options()
    assert len(names) >= 12 and len(set(names)) == len(names)
    for n in names:
        cls = hs.option_class(n)
        assert cls in ("inference", "training") or (isinstance(cls, tuple) and cls[0] == "n/a" and len(cls[1]) > 10), n
    listed = {n for n, _ in hs.INFERENCE_OPTIONS + hs.TRAINING_OPTIONS} | set(hs.NOT_APPLICABLE)
    assert listed <= set(names), listed - set(names)
    assert not {n for n, _ in hs.INFERENCE_OPTIONS} & {n for n, _ in hs.TRAINING_OPTIONS}


class StubBackend:
    """Records what the runner asks for; a compute step's output is a function of exactly what a fresh handle would see (the
    step, the weights, the options, the input), so a runner that forgot to apply or to clear something compares unequal."""

    def __init__(self):
        self.options, self.made, self.log = {}, 0, []

    def set_option(self, name, value):
        self.log.append(("option", name, value))
        if value is None:
            self.options.pop(name, None)
        else:
            self.options[name] = value

    def clear_options(self):
        self.options.clear()

    def make_model(self, cfg, weights):
        self.made += 1
        return dict(cfg=hs._freeze(cfg), weights=tuple(weights), lane=0, flat=False, runs=0)

    def set_weights(self, model, s):
        model["weights"] = (("seed", s["seed"]),) if s["seed"] is not None else model["weights"] + (("add", s["tensor"], float(s["add"])),)

    def select_lane(self, model, k):
        model["lane"] = k

    def attach_flat(self, model):
        model["flat"] = True

    def poison(self, model, s):
        self.log.append(("poison", s["hwd"], s["B"]))

    def clone(self, x):
        return ("clone", x)

    def run(self, model, s, x=None):
        model["runs"] += 1
        self.log.append(("run", s["op"]))
        if isinstance(x, tuple) and x and x[0] == "clone":
            x = x[1]
        core = hs._freeze(s)
        return ((model["cfg"], model["weights"], tuple(sorted(self.options.items())), core, x), "second output")

    def equal(self, a, b):
        return a == b


def _all_sequences():
    seqs = {"shapes": hs.shapes_and_batches(), "modes32": hs.modes_at_one_shape(32), "modes64": hs.modes_at_one_shape(64)}
    for k, v in hs.carry_cases(hs.S_A, 2).items():
        seqs["carry_" + k] = v
    for name, value in hs.INFERENCE_OPTIONS:
        for loop in (False, True):
            seqs[f"opt_{name}={value}_{loop}"] = hs.live_option(hs.S_EVEN, 3, name, value, loop)
    for kind in ("load_state_dict", "inplace", "to_roundtrip", "load_on_lane_2"):
        seqs["sync_" + kind] = hs.parameter_sync(kind)
    return seqs


TRAINING_SEQUENCES = {"train_infer_train": hs.train_then_infer_then_train((9, 13, 7), 2),
                      "sample_between": hs.sample_between_train_steps((9, 13, 7), 2),
                      **{f"topt_{n}": hs.live_training_option((9, 13, 7), 2, n, v) for n, v in hs.TRAINING_OPTIONS}}


@pytest.mark.parametrize("name", sorted(_all_sequences()))
def test_inference_sequences_have_references_and_a_covering_poison(name):
    """Every compute step gets a signature (so a reference), non-compute steps none; a poison step precedes the last compute step
    (or the carried pair it ends) and is at least as large; the runner on a stub reproduces the fresh references."""
    steps = _all_sequences()[name]
    sigs = hs.plan(dict(mc=64, cm=(1, 2)), steps)
    assert len(sigs) == len(steps)
    for s, sig in zip(steps, sigs):
        assert (sig is not None) == (s["op"] in hs.COMPUTE_OPS), s
    target = hs.poisoned_steps(steps)
    comp = [i for i, s in enumerate(steps) if s["op"] in hs.COMPUTE_OPS]
    assert target and target[-1] == comp[-1]
    p = max(i for i in range(target[0]) if steps[i]["op"] == "poison")
    assert all(steps[i]["op"] not in hs.COMPUTE_OPS for i in range(p, target[0]))
    assert all(steps[p]["B"] >= steps[i]["B"] and all(a >= b for a, b in zip(steps[p]["hwd"], steps[i]["hwd"])) for i in target)
    b = StubBackend()
    cache = {}
    _, outs = hs.check_sequence(b, dict(mc=64, cm=(1, 2)), steps, cache)
    assert b.options == {} and len(cache) == len({s for s in sigs if s is not None})
    assert sum(o is not None for o in outs) == len(comp)
    made = b.made
    hs.check_sequence(b, dict(mc=64, cm=(1, 2)), steps, cache)
    assert b.made == made + 1, "cached references are not recomputed: only the sequence's own model is new"


@pytest.mark.parametrize("name", sorted(TRAINING_SEQUENCES))
def test_training_sequences_on_the_stub(name):
    steps = TRAINING_SEQUENCES[name]
    assert not any(s["op"] == "poison" for s in steps), "the poison is an inference forward: it would discard the tape"
    b = StubBackend()
    hs.check_sequence(b, dict(mc=32, cm=(1, 2)), steps, {}, inference=False)
    assert b.options == {}


def test_the_runner_notices_what_it_should():
    """The stub's outputs depend on weights, options and input: a sequence without its poison is rejected, and a reference that
    ignored an option or a weight change would differ."""
    cfg = dict(mc=64, cm=(1, 2))
    seq = hs.shapes_and_batches()
    with pytest.raises(AssertionError, match="poison"):
        hs.plan(cfg, [s for s in seq if s["op"] != "poison"])
    small = [hs.forward(hs.S_A, 2, 1), hs.poison(hs.S_MIN, 2), hs.forward(hs.S_A, 2, 1)]
    with pytest.raises(AssertionError, match="poison"):
        hs.plan(cfg, small)
    a = hs.plan(cfg, [hs.forward(hs.S_A, 2, 1), hs.option("VCAT", "0"), hs.poison(hs.S_A, 2), hs.forward(hs.S_A, 2, 1)])
    assert a[0] != a[3] and a[0][3] == a[3][3]
    w = hs.plan(cfg, [hs.forward(hs.S_A, 2, 1), hs.set_weights(seed=1), hs.poison(hs.S_A, 2), hs.forward(hs.S_A, 2, 1)])
    assert w[0] != w[3] and w[3][1] == (("seed", 1),)
    c = hs.plan(cfg, hs.carry_cases(hs.S_A, 2)["c_same_shape"])
    last = [s for s in c if s is not None][-1]
    assert last[4] is not None and dict(last[3]).get("carry") is None      # fed by the carry-out step; the flags are not in the signature


def test_option_round_trips_after_the_generation_change():
    """s3d_set_option / s3d_get_option through the CPU-loadable part of the ABI: set, read back, clear, reject."""
    lib = _lib.load()
    names = _library_options()
    try:
        for n in names:
            for v in ({"WINO": ("0", "4", "24"), "CONV_IMPL": ("naive", "mfma")}.get(n, ("0", "1"))):
                _lib.set_option(n, v)
                want = {"naive": 1, "mfma": 0}.get(v, int(v) if v.isdigit() else None)
                assert _lib.get_option(n) == want and _lib.get_option("S3D_" + n) == want, (n, v)
            _lib.set_option(n, None)
            assert _lib.get_option(n) is None
            _lib.set_option(n, "")
            assert _lib.get_option(n) is None
        assert lib.s3d_set_option(b"WINO", b"3") == _lib.ERR_INVALID and b"takes" in lib.s3d_last_error()
        assert _lib.get_option("WINO") is None                       # a rejected value changes nothing
        assert lib.s3d_set_option(b"NO_SUCH_OPTION", b"1") == _lib.ERR_INVALID
        v = C.c_int(7)
        assert lib.s3d_get_option(b"NO_SUCH_OPTION", C.byref(v)) == _lib.ERR_INVALID and v.value == 7
    finally:
        for n in names:
            _lib.set_option(n, None)
