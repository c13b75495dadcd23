"""CPU-only: the host half of SSFID (sin3dm_amd/evaluation/ssfid.py, s3d_ssfid.hip).  The float64 restatement of
tests/ssfid_cases.py is pinned to what the reference's own modules gave (tests/golden/ssfid.npz) at ten times the reference's
float32-versus-float64 gap per statistic, three injected defects each break that bound, the Frechet distance's symmetric form
is held to the reference's scipy.linalg.sqrtm path, and the checkpoint reader, the command line and the ABI are checked."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import ssfid_cases as S
from conftest import REPO, golden
from sin3dm_amd import _lib
from sin3dm_amd.evaluation import ssfid as F

ENTRY_POINTS = ("s3d_ssfid_create", "s3d_ssfid_set_param", "s3d_ssfid_out_dims", "s3d_ssfid_features", "s3d_ssfid_profile",
                "s3d_ssfid_profile_read")
FULL_RANK_PAIRS = tuple(p for p in S.PAIRS if p != "prank")


def test_cases_are_what_the_fixture_was_recorded_on():
    assert os.path.getsize(os.path.join(REPO, "tests", "golden", "ssfid.npz")) < 700 * 1024
    long = S.volume("long")
    assert long.shape == (96, 80, 64) and 0.2 < long.mean() < 0.8
    assert S.restated("long", 1)[0].shape == (61440, 32) and S.restated("long", 2)[0].shape == (7680, 64)
    assert S.volume("free").shape == (32, 26, 20) and not S.volume("free").any()
    assert S.restated("rank_a", 2)[0].shape == (24, 64) and np.linalg.matrix_rank(S.restated("rank_a", 2)[2]) < 64
    assert S.restated("ref40", 1)[0].shape[0] == 20 * 16 * 12 and S.restated("ref40", 2)[0].shape[0] == 10 * 8 * 6
    w = S.weights()
    assert {k: tuple(v.shape) for k, v in w.items()} == S.PARAM_SHAPES and all(v.dtype == torch.float32 for v in w.values())


@pytest.mark.parametrize("layer", S.LAYERS)
def test_restatement_is_pinned_to_the_reference(layer):
    g = golden("ssfid")
    for name in S.volume_names():
        act, mu, sigma = S.restated(name, layer)
        key = f"{name}/{layer}"
        e_mu, e_sigma = np.max(np.abs(mu - g[f"{key}/mu"])), np.max(np.abs(sigma - g[f"{key}/sigma"]))
        print(key, "mu", e_mu, "of", 10 * g[f"{key}/gap_mu"], "sigma", e_sigma, "of", 10 * g[f"{key}/gap_sigma"])
        assert e_mu <= 10 * g[f"{key}/gap_mu"], (key, e_mu)
        assert e_sigma <= 10 * g[f"{key}/gap_sigma"], (key, e_sigma)
        if name == S.ACT_CASE:
            e_act = np.max(np.abs(act - g[f"act/{layer}"]))
            print(key, "act", e_act, "of", 10 * g[f"{key}/gap_act"])
            assert act.shape == g[f"act/{layer}"].shape and e_act <= 10 * g[f"{key}/gap_act"], (key, e_act)
    assert np.max(np.abs(S.restated("free", layer)[0])) < 1e-9              # an empty volume normalises to zero


@pytest.mark.parametrize("fault", ("pad_first", "unbiased_var", "ddof0"))
def test_injected_defects_break_the_bound(fault):
    """Each defect moves mu or sigma of layer 2 past ten times the recorded gap on at least one case."""
    g = golden("ssfid")
    broken = []
    for name in ("ref32", "ref40", "rank_a"):
        _, mu, sigma = S.restate(S.volume(name), S.weights(), 2, fault=fault)
        key = f"{name}/2"
        e_mu, e_sigma = np.max(np.abs(mu - g[f"{key}/mu"])), np.max(np.abs(sigma - g[f"{key}/sigma"]))
        print(fault, key, "mu", e_mu, "bound", 10 * g[f"{key}/gap_mu"], "sigma", e_sigma, "bound", 10 * g[f"{key}/gap_sigma"])
        if e_mu > 10 * g[f"{key}/gap_mu"] or e_sigma > 10 * g[f"{key}/gap_sigma"]:
            broken.append(name)
    assert broken, fault


def _fixture_stats(g, name, layer):
    return g[f"{name}/{layer}/mu"], g[f"{name}/{layer}/sigma"]


@pytest.mark.parametrize("layer", S.LAYERS)
def test_frechet_distance_against_the_sqrtm_path(layer):
    g = golden("ssfid")
    sym_gap = max(float(g[f"{p}/{l}/fd_sym_gap"]) for p in FULL_RANK_PAIRS for l in S.LAYERS)
    assert 0 < sym_gap < 1e-8                                               # what DESIGN.md §21 quotes (4.4e-10)
    for pair in FULL_RANK_PAIRS:
        r, gen = S.PAIRS[pair]
        want = float(g[f"{pair}/{layer}/fd"])
        got = F.frechet_distance(*_fixture_stats(g, r, layer), *_fixture_stats(g, gen, layer))
        print(pair, layer, got, want, abs(got - want) / want)
        assert 0.005 < want < 4.0 and abs(got - want) <= 10 * sym_gap * want, (pair, got, want)
        for name in (r, gen):                                               # identical statistics: zero
            mu, sigma = _fixture_stats(g, name, layer)
            assert abs(F.frechet_distance(mu, sigma, mu, sigma)) <= 1e-12 * 2 * np.trace(sigma), name


def test_rank_deficient_statistics_give_the_symmetric_form():
    """24 rows for 64 channels: the product of the covariances is singular, where sqrtm adds 1e-6 to the diagonals.  The distance
    is finite and is the symmetric form: Tr sqrt(s1^1/2 s2 s1^1/2) is the nuclear norm of s2^1/2 s1^1/2."""
    _, m1, s1 = S.restated("rank_a", 2)
    _, m2, s2 = S.restated("rank_b", 2)
    assert np.linalg.matrix_rank(s1) <= 23 and np.linalg.matrix_rank(s2) <= 23
    d = F.frechet_distance(m1, s1, m2, s2)

    def root(s):
        w, v = np.linalg.eigh(s)
        return (v * np.sqrt(np.clip(w, 0, None))) @ v.T

    nuclear = np.linalg.svd(root(s2) @ root(s1), compute_uv=False).sum()
    want = (m1 - m2).dot(m1 - m2) + np.trace(s1) + np.trace(s2) - 2 * nuclear
    print(d, want)
    assert np.isfinite(d) and d > 0 and abs(d - want) <= 1e-6 * (np.trace(s1) + np.trace(s2))


def test_frechet_distance_needs_no_scipy():
    src = open(os.path.join(REPO, "sin3dm_amd", "evaluation", "ssfid.py")).read()
    assert "scipy" not in src


def test_checkpoint_reader(tmp_path):
    w = S.weights()
    full = dict(w)
    full["conv_3.weight"] = torch.zeros(128, 64, 4, 4, 4)                   # the real file carries conv_3 ... linear1: ignored
    full["linear1.bias"] = torch.zeros(24)
    full["conv_1.bias"] = full["conv_1.bias"].double()                      # returned as float32
    torch.save(full, tmp_path / "ok.pth")
    got = F.load_classifier_weights(str(tmp_path / "ok.pth"))
    assert list(got) == list(S.PARAM_SHAPES)
    for k, v in got.items():
        assert v.dtype == torch.float32 and v.is_contiguous() and torch.equal(v, w[k]), k
    missing = {k: v for k, v in w.items() if k != "conv_2.bias"}
    torch.save(missing, tmp_path / "missing.pth")
    with pytest.raises(KeyError, match="conv_2.bias"):
        F.load_classifier_weights(str(tmp_path / "missing.pth"))
    wrong = dict(w)
    wrong["conv_2.weight"] = torch.zeros(128, 64, 4, 4, 4)                  # an ef_dim = 64 classifier
    torch.save(wrong, tmp_path / "wrong.pth")
    with pytest.raises(ValueError, match=r"conv_2.weight.*\(128, 64, 4, 4, 4\)"):
        F.load_classifier_weights(str(tmp_path / "wrong.pth"))


def test_cli_flags_and_unchanged_message():
    from sin3dm_amd.evaluation import eval_geometry as eg
    a = eg.parse_args(["-s", "gen", "-r", "ref"])
    assert a.ssfid_weights is None and a.ssfid_layer == 2
    b = eg.parse_args(["-s", "gen", "-r", "ref", "--ssfid_weights", "w.pth", "--ssfid_layer", "1"])
    assert b.ssfid_weights == "w.pth" and b.ssfid_layer == 1
    with pytest.raises(SystemExit):
        eg.parse_args(["-s", "gen", "-r", "ref", "--ssfid_layer", "3"])
    assert eg.NOT_COMPUTED == ("eval_geometry: SSFID, SIFID and LPIPS are not computed: they need a 3D classifier checkpoint, Inception and "
                               "VGG weights and rendered views, none of which can be obtained offline")
    assert "SSFID" not in eg.NOT_COMPUTED_WITH_SSFID and "SIFID" in eg.NOT_COMPUTED_WITH_SSFID and "LPIPS" in eg.NOT_COMPUTED_WITH_SSFID
    assert "\n" not in eg.NOT_COMPUTED_WITH_SSFID


def test_header_binding_and_abi_agree():
    import sin3dm_amd.evaluation as ev
    for name in ("VoxelClassifier", "frechet_distance", "load_classifier_weights", "eval_ssfid"):
        assert callable(getattr(ev, name)), name
    lib = _lib.load()
    header = open(os.path.join(REPO, "include", "sin3dm_hip.h")).read()
    for name in ENTRY_POINTS:
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
        decl = re.search(r"S3D_API int " + name + r"\(([^;]*)\);", header)
        assert decl, name
        assert len(decl.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name
    assert "S3D_API void s3d_ssfid_destroy(s3d_ssfid* h);" in header and "s3d_ssfid_destroy" in _lib.SIGNATURES
    assert int(re.search(r"#define S3D_ABI_VERSION (\d+)", header).group(1)) == _lib.ABI_VERSION == lib.s3d_abi_version() == 13


def test_argument_errors_launch_nothing():
    """Validation happens before any launch or allocation, so it can be checked without a GPU."""
    lib = _lib.load()
    h = C.c_void_p()
    assert lib.s3d_ssfid_create(C.byref(h)) == 0
    try:
        dims, od, ch = (C.c_int * 3)(40, 33, 25), (C.c_int * 3)(), C.c_int()
        assert lib.s3d_ssfid_out_dims(dims, 1, od, C.byref(ch)) == 0 and (tuple(od), ch.value) == ((20, 16, 12), 32)
        assert lib.s3d_ssfid_out_dims(dims, 2, od, C.byref(ch)) == 0 and (tuple(od), ch.value) == ((10, 8, 6), 64)
        for layer in (3, 4):
            assert lib.s3d_ssfid_out_dims(dims, layer, od, C.byref(ch)) == _lib.ERR_UNSUPPORTED and b"out_layer" in lib.s3d_last_error()
        assert lib.s3d_ssfid_out_dims(dims, 0, od, C.byref(ch)) == _lib.ERR_INVALID
        assert lib.s3d_ssfid_out_dims((C.c_int * 3)(40, 3, 25), 2, od, C.byref(ch)) == _lib.ERR_INVALID and b"axis 1" in lib.s3d_last_error()
        assert lib.s3d_ssfid_out_dims((C.c_int * 3)(40, 3, 25), 1, od, C.byref(ch)) == 0
        assert lib.s3d_ssfid_out_dims((C.c_int * 3)(40, 1, 25), 1, od, C.byref(ch)) == _lib.ERR_INVALID
        # a wrong shape names itself and is 'unsupported'; an unknown name is invalid
        bad = np.zeros((64, 1, 4, 4, 4), dtype=np.float32)
        shape = (C.c_int64 * 5)(*bad.shape)
        assert lib.s3d_ssfid_set_param(h, b"conv_1.weight", bad.ctypes.data_as(C.c_void_p), shape, 5) == _lib.ERR_UNSUPPORTED
        assert b"conv_1.weight" in lib.s3d_last_error() and b"[64, 1, 4, 4, 4]" in lib.s3d_last_error()
        assert lib.s3d_ssfid_set_param(h, b"conv_3.weight", bad.ctypes.data_as(C.c_void_p), shape, 5) == _lib.ERR_INVALID
        # features before the weights are set: refused by name, nothing touched (the pointers here are never dereferenced)
        w = S.weights(as_torch=False)
        for k in ("conv_1.weight", "conv_1.bias", "conv_2.weight"):
            s = (C.c_int64 * w[k].ndim)(*w[k].shape)
            assert lib.s3d_ssfid_set_param(h, k.encode(), w[k].ctypes.data_as(C.c_void_p), s, w[k].ndim) == 0
        fake = C.c_void_p(256)
        assert lib.s3d_ssfid_features(h, fake, dims, 2, None, fake, fake, None) == _lib.ERR_INVALID
        assert b"conv_2.bias" in lib.s3d_last_error()
        assert lib.s3d_ssfid_features(h, fake, dims, 3, None, fake, fake, None) == _lib.ERR_UNSUPPORTED
        assert lib.s3d_ssfid_features(h, fake, (C.c_int * 3)(40, 1, 25), 1, None, fake, fake, None) == _lib.ERR_INVALID
    finally:
        lib.s3d_ssfid_destroy(h)
