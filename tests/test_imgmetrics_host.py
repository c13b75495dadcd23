"""CPU-only: the host half of SIFID and LPIPS (sin3dm_amd/evaluation/{sifid,lpips,eval_renders,eval_full}.py, s3d_imgfeat.hip).
The float64 restatement of tests/imgmetrics_cases.py is pinned to what the reference's own modules gave
(tests/golden/imgmetrics.npz) at ten times the reference's float32-versus-float64 gap per statistic, the uint8 -> float32 input
maps are held bit for bit, six injected defects each break a bound, and the weight loaders, the command lines and the ABI are
checked."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import imgmetrics_cases as S
from conftest import REPO, golden
from sin3dm_amd import _lib
from sin3dm_amd.evaluation import eval_full, eval_renders, lpips as L, sifid as F
from sin3dm_amd.evaluation.ssfid import frechet_distance

ENTRY_POINTS = ("s3d_imgfeat_create", "s3d_imgfeat_set_param", "s3d_imgfeat_out_dims", "s3d_imgfeat_features", "s3d_imgfeat_stats",
                "s3d_imgfeat_pairs", "s3d_imgfeat_profile", "s3d_imgfeat_profile_read")


def _err(a, b):
    return float(np.max(np.abs(np.asarray(a, dtype=np.float64) - b)))


def test_cases_are_what_the_fixture_was_recorded_on():
    assert os.path.getsize(os.path.join(REPO, "tests", "golden", "imgmetrics.npz")) < 256 * 1024
    g = golden("imgmetrics")
    assert [S.sifid_restated("a0", 192)[0][l].shape for l in range(5)] == [(47, 39, 32), (45, 37, 32), (45, 37, 64), (22, 18, 80), (20, 16, 192)]
    assert S.sifid_restated("b", 64)[0][2].shape == (46, 48, 64) and S.sifid_restated("b", 192)[0][3].shape == (22, 23, 80)
    assert S.sifid_restated("d", 64)[0][2].shape[:2] == (97, 65) and S.sifid_restated("s", 192)[0][4].shape == (6, 6, 192)
    assert [m.shape for m in S.lpips_restated("b", "b1")[2]] == [(23, 24, 64), (11, 11, 192), (5, 5, 384), (5, 5, 256), (5, 5, 256)]
    for name in S.PARITY:                                                    # rows > C and no constant channel
        for dims in S.DIMS:
            rows = S.sifid_restated(name, dims)[0][-1].reshape(-1, dims)
            assert rows.shape[0] > dims and np.all(rows.std(axis=0) > 1e-3), (name, dims)
    assert sum(g[f"lin/{l}"].size for l in range(5)) == 1152 and all(np.all(g[f"lin/{l}"] >= 0) for l in range(5))
    for img in (S.image("a0"), S.image("d1")):
        assert img.dtype == np.uint8 and img.shape[2] == 4 and set(np.unique(img[..., 3])) == {0, 255} and len(np.unique(img[..., :3])) > 200
    for pair in S.SIFID_PAIRS:                                               # condition 2 of the fixture
        for dims in S.DIMS:
            assert 10 * g[f"sifid/{pair}/{dims}/fd_gap"] < 1e-3 * g[f"sifid/{pair}/{dims}/fd"]
    for pair in S.LPIPS_PAIRS:
        assert 10 * g[f"lpips/{pair}/gap_total"] < 1e-3 * g[f"lpips/{pair}/total"]


def test_input_maps_bit_for_bit():
    """All 256 sample values x 3 channels: the restatement's maps are the reference's expressions, and float32 division and the
    float64 forms the kernel may use agree on every value."""
    u = np.repeat(np.arange(256, dtype=np.uint8)[:, None, None], 3, axis=2)              # [256][1][3]
    s = S.sifid_input(u).numpy()[0].transpose(1, 2, 0)
    x32 = u.astype(np.float32) / np.float32(255)
    assert s.dtype == np.float32 and np.array_equal(s, np.float32(2) * x32 - np.float32(1))
    assert np.array_equal(x32, (u / 255.0).astype(np.float32)) and s.min() == -1.0 and s.max() == 1.0
    p = S.lpips_input(u).numpy()[0].transpose(1, 2, 0)
    v = ((u / 255. - 0.5) / 0.5).astype(np.float32)
    want = (v - np.asarray(S.LPIPS_MU, dtype=np.float32)) / np.asarray(S.LPIPS_SIGMA, dtype=np.float32)
    assert p.dtype == np.float32 and np.array_equal(p, want)
    rgba = np.concatenate([u, np.full((256, 1, 1), 7, dtype=np.uint8)], axis=2)           # alpha is read but never applied
    assert np.array_equal(S.sifid_input(rgba).numpy(), S.sifid_input(u).numpy())


@pytest.mark.parametrize("dims", S.DIMS)
def test_sifid_restatement_is_pinned_to_the_reference(dims):
    g = golden("imgmetrics")
    for name in S.IMAGES:
        acts, mu, sigma = S.sifid_restated(name, dims)
        key = f"sifid/{name}/{dims}"
        e_mu = _err(mu, g[f"{key}/mu"])
        e_sigma = max(_err(np.diag(sigma), g[f"{key}/sigma_diag"]), _err(sigma[::8, ::8], g[f"{key}/sigma_sub"]))
        print(key, "mu", e_mu, "of", 10 * g[f"{key}/gap_mu"], "sigma", e_sigma, "of", 10 * g[f"{key}/gap_sigma"])
        assert e_mu <= 10 * g[f"{key}/gap_mu"] and e_sigma <= 10 * g[f"{key}/gap_sigma"], key
        if name == S.ACT_CASE:
            e_act = _err(acts[-1].reshape(-1, dims)[::8], g[f"act/{dims}"])
            print(key, "act", e_act, "of", 10 * g[f"{key}/gap_act"][-1])
            assert e_act <= 10 * g[f"{key}/gap_act"][-1]
    for pair, (r, gen) in S.SIFID_PAIRS.items():
        fd = frechet_distance(*S.sifid_restated(r, dims)[1:], *S.sifid_restated(gen, dims)[1:])
        want, gap = float(g[f"sifid/{pair}/{dims}/fd"]), float(g[f"sifid/{pair}/{dims}/fd_gap"])
        print(pair, dims, fd, want, abs(fd - want), S.bound(gap, want))
        assert abs(fd - want) <= S.bound(gap, want), pair


def test_lpips_restatement_is_pinned_to_the_reference():
    g = golden("imgmetrics")
    for pair, (a, b) in S.LPIPS_PAIRS.items():
        terms, total, _ = S.lpips_restated(a, b)
        key = f"lpips/{pair}"
        print(key, total, float(g[f"{key}/total"]), np.abs(terms - g[f"{key}/terms"]), g[f"{key}/gap_terms"])
        assert abs(total - g[f"{key}/total"]) <= S.bound(g[f"{key}/gap_total"], g[f"{key}/total"])
        assert _err(terms, g[f"{key}/terms"]) <= S.bound(np.max(g[f"{key}/gap_terms"]), g[f"{key}/terms"])
    with pytest.raises(RuntimeError, match="too small"):                     # the reference raises at 40 x 40; so does the restatement
        S.lpips_restate(S.image("s"), S.image("s1"), S.alexnet_weights(), S.lpips_linear())


@pytest.mark.parametrize("fault", ("bn_eps", "ceil_pool", "ddof0", "no_2x1"))
def test_injected_sifid_defects_break_a_bound(fault):
    g = golden("imgmetrics")
    broken = []
    for name in ("a0", "b"):                                                 # b: even pre-pool extents, where ceil mode adds a row and a column
        try:
            _, mu, sigma = S.sifid_restate(S.image(name), S.inception_weights(), 192, fault=fault)
        except Exception as e:                                              # a changed extent downstream is a break as well
            broken.append((name, type(e).__name__))
            continue
        key = f"sifid/{name}/192"
        e_mu = _err(mu, g[f"{key}/mu"]) if mu.shape == g[f"{key}/mu"].shape else np.inf
        e_sigma = _err(np.diag(sigma), g[f"{key}/sigma_diag"])
        print(fault, key, "mu", e_mu, "bound", 10 * g[f"{key}/gap_mu"], "sigma", e_sigma, "bound", 10 * g[f"{key}/gap_sigma"])
        if e_mu > S.bound(g[f"{key}/gap_mu"], g[f"{key}/mu"]) or e_sigma > S.bound(g[f"{key}/gap_sigma"], g[f"{key}/sigma_diag"]):
            broken.append(name)
    assert broken, fault


@pytest.mark.parametrize("fault", ("sqrt_eps", "no_imagenet"))
def test_injected_lpips_defects_break_a_bound(fault):
    g = golden("imgmetrics")
    broken = []
    for pair in ("pa", "pb"):
        a, b = S.LPIPS_PAIRS[pair]
        terms, total, _ = S.lpips_restate(S.image(a), S.image(b), S.alexnet_weights(), S.lpips_linear(), fault=fault)
        key = f"lpips/{pair}"
        e_terms, b_terms = _err(terms, g[f"{key}/terms"]), S.bound(np.max(g[f"{key}/gap_terms"]), g[f"{key}/terms"])
        e_total, b_total = abs(total - float(g[f"{key}/total"])), S.bound(g[f"{key}/gap_total"], g[f"{key}/total"])
        print(fault, key, "terms", e_terms, "bound", b_terms, "total", e_total, "bound", b_total)
        if e_terms > b_terms or e_total > b_total:
            broken.append(pair)
    assert broken, fault


def test_weight_loaders(tmp_path):
    w = dict(S.inception_weights())
    full = dict(w)
    full["Mixed_5b.branch1x1.conv.weight"] = torch.zeros(64, 192, 1, 1)      # the real file carries the whole network: ignored
    full["fc.bias"] = torch.zeros(1000)
    full["Conv2d_1a_3x3.bn.num_batches_tracked"] = torch.tensor(0)
    full["Conv2d_2a_3x3.bn.bias"] = full["Conv2d_2a_3x3.bn.bias"].double()   # returned as float32
    torch.save(full, tmp_path / "inception.pth")
    got = F.check_inception_weights(F.load_state(str(tmp_path / "inception.pth")))
    assert list(got) == list(F.INCEPTION_PARAM_SHAPES) and len(got) == 25
    for k, v in got.items():
        assert v.dtype == torch.float32 and v.is_contiguous() and torch.equal(v, w[k]), k
    with pytest.raises(KeyError, match="Conv2d_4a_3x3.bn.running_var"):
        F.check_inception_weights({k: v for k, v in w.items() if k != "Conv2d_4a_3x3.bn.running_var"})
    wrong = dict(w)
    wrong["Conv2d_3b_1x1.conv.weight"] = torch.zeros(80, 64, 3, 3)
    with pytest.raises(ValueError, match=r"Conv2d_3b_1x1.conv.weight.*\(80, 64, 3, 3\)"):
        F.check_inception_weights(wrong)
    a = dict(S.alexnet_weights())
    a["classifier.1.weight"] = torch.zeros(8, 8)
    assert list(F.check_weights(a, L.ALEXNET_PARAM_SHAPES, "alexnet")) == list(L.ALEXNET_PARAM_SHAPES) and len(L.ALEXNET_PARAM_SHAPES) == 10
    with pytest.raises(KeyError, match="features.10.bias"):
        F.check_weights({k: v for k, v in a.items() if k != "features.10.bias"}, L.ALEXNET_PARAM_SHAPES, "alexnet")
    lin = dict(S.lpips_linear())
    assert {k: tuple(v.shape) for k, v in lin.items()} == L.LPIPS_PARAM_SHAPES
    lin["lpips_weights.2.main.1.weight"] = torch.zeros(1, 256, 1, 1)
    with pytest.raises(ValueError, match=r"lpips_weights.2.main.1.weight"):
        F.check_weights(lin, L.LPIPS_PARAM_SHAPES, "lpips")
    torch.save([1, 2], tmp_path / "list.pth")
    with pytest.raises(ValueError, match="state dict"):
        F.load_state(str(tmp_path / "list.pth"))
    with pytest.raises(_lib.Sin3DMHipError, match="no CPU fallback"):
        F.as_image_batch(torch.zeros(1, 8, 8, 3, dtype=torch.uint8))


def test_cli_parsers_and_key_order():
    from sin3dm_amd.evaluation import eval_geometry as eg
    assert eval_full.KEYS == ("SSFID_avg", "SSFID_std", "LP-IOU-avg", "LP-IOU-percent", "LP-F-score-avg", "LP-F-score-percent", "Div",
                              "mv_sifid_dim64", "mv_sifid_dim192", "mv_lpips")
    assert eval_renders.KEYS == eval_full.KEYS[7:]
    weights = ["--inception_weights", "i.pth", "--alexnet_weights", "a.pth", "--lpips_weights", "l.ckpt"]
    r = eval_renders.parse_args(["-s", "gen", "-r", "ref"] + weights)
    assert (r.src, r.ref, r.inception_weights, r.alexnet_weights, r.lpips_weights, r.output) == ("gen", "ref", "i.pth", "a.pth", "l.ckpt", None)
    f = eval_full.parse_args(["-s", "gen", "-r", "ref", "--ssfid_weights", "c.pth"] + weights)
    g = eg.parse_args(["-s", "gen", "-r", "ref", "--ssfid_weights", "c.pth"])
    for k in ("patch_size", "stride", "patch_num", "ssfid_layer", "ssfid_weights", "output"):      # eval_geometry's flags and defaults
        assert getattr(f, k) == getattr(g, k), k
    for missing in (["-s", "gen", "-r", "ref"], ["-s", "gen", "-r", "ref", "--ssfid_weights", "c.pth"] + weights[:4]):
        with pytest.raises(SystemExit):
            eval_full.parse_args(missing)
    with pytest.raises(SystemExit):
        eval_renders.parse_args(["-s", "gen", "-r", "ref"] + weights[:2])
    assert "not computed" in eg.NOT_COMPUTED and "not computed" in eg.NOT_COMPUTED_WITH_SSFID      # eval_geometry itself is unchanged
    assert F.view_paths("d", 2) == [os.path.join("d", "000.png"), os.path.join("d", "001.png")]


def test_find_renders(tmp_path):
    gen, ref = S.write_tree(str(tmp_path))
    g, r = eval_renders.find_renders(str(tmp_path / "src"), str(tmp_path / "ref"))
    assert g == sorted(gen) and r == ref and len(os.listdir(r)) == S.E2E_VIEWS
    assert np.array_equal(F.read_png(os.path.join(r, "000.png")), S.image(S.E2E_TREE["ref"][0]))
    with pytest.raises(FileNotFoundError):
        eval_renders.find_renders(str(tmp_path / "ref"), str(tmp_path / "ref"))
    with pytest.raises(FileNotFoundError):
        eval_renders.find_renders(str(tmp_path / "src"), str(tmp_path / "src"))


def test_header_binding_and_abi_agree():
    lib = _lib.load()
    header = open(os.path.join(REPO, "include", "sin3dm_hip.h")).read()
    for name in ENTRY_POINTS:
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
        decl = re.search(r"S3D_API int " + name + r"\(([^;]*)\);", header)
        assert decl, name
        assert len(decl.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name
    assert "S3D_API void s3d_imgfeat_destroy(s3d_imgfeat* h);" in header and "s3d_imgfeat_destroy" in _lib.SIGNATURES
    assert (_lib.IMGFEAT_INCEPTION, _lib.IMGFEAT_ALEXNET) == tuple(int(re.search(r"#define S3D_IMGFEAT_" + n + r" (\d+)", header).group(1))
                                                                   for n in ("INCEPTION", "ALEXNET"))


def test_argument_errors_launch_nothing():
    """Validation happens before any launch or allocation, so it can be checked without a GPU."""
    lib = _lib.load()
    nl, hw, ch = C.c_int(), (C.c_int * 10)(), (C.c_int * 5)()

    def dims(net, H, W, d):
        rc = lib.s3d_imgfeat_out_dims(net, H, W, d, C.byref(nl), hw, ch)
        return rc, [(hw[2 * l], hw[2 * l + 1], ch[l]) for l in range(nl.value)] if rc == 0 else None

    assert dims(0, 96, 80, 64) == (0, [(47, 39, 32), (45, 37, 32), (45, 37, 64)])
    assert dims(0, 98, 101, 192) == (0, [(48, 50, 32), (46, 48, 32), (46, 48, 64), (22, 23, 80), (20, 21, 192)])
    assert dims(1, 98, 101, 0) == (0, [(23, 24, 64), (11, 11, 192), (5, 5, 384), (5, 5, 256), (5, 5, 256)])
    assert dims(1, 512, 512, 0)[1][0] == (127, 127, 64) and dims(1, 512, 512, 0)[1][4] == (31, 31, 256)
    assert dims(0, 512, 512, 192)[1][2:] == [(253, 253, 64), (126, 126, 80), (124, 124, 192)]
    for d in (0, 100, 768, 2048):
        assert dims(0, 96, 80, d)[0] == _lib.ERR_UNSUPPORTED and b"dims" in lib.s3d_last_error()
    assert dims(1, 40, 40, 0)[0] == _lib.ERR_INVALID and b"too small" in lib.s3d_last_error() and b"MaxPool2d(3, 2)" in lib.s3d_last_error()
    assert dims(1, 62, 62, 0)[0] == _lib.ERR_INVALID and dims(1, 63, 63, 0)[0] == 0           # the smallest image AlexNet's features take
    assert dims(0, 6, 96, 64)[0] == _lib.ERR_INVALID and dims(0, 7, 7, 64) == (0, [(3, 3, 32), (1, 1, 32), (1, 1, 64)])
    assert dims(0, 7, 7, 192)[0] == _lib.ERR_INVALID and dims(0, 0, 7, 64)[0] == _lib.ERR_INVALID
    assert dims(2, 96, 80, 64)[0] == _lib.ERR_UNSUPPORTED
    h = C.c_void_p()
    assert lib.s3d_imgfeat_create(2, C.byref(h)) == _lib.ERR_UNSUPPORTED
    assert lib.s3d_imgfeat_create(_lib.IMGFEAT_INCEPTION, C.byref(h)) == 0
    try:
        bad = np.zeros((32, 3, 5, 5), dtype=np.float32)
        shape = (C.c_int64 * 4)(*bad.shape)
        assert lib.s3d_imgfeat_set_param(h, b"Conv2d_1a_3x3.conv.weight", bad.ctypes.data_as(C.c_void_p), shape, 4) == _lib.ERR_UNSUPPORTED
        assert b"[32, 3, 5, 5]" in lib.s3d_last_error()
        for name in (b"Mixed_5b.branch1x1.conv.weight", b"features.0.weight", b"Conv2d_1a_3x3.bn.num_batches_tracked"):
            assert lib.s3d_imgfeat_set_param(h, name, bad.ctypes.data_as(C.c_void_p), shape, 4) == _lib.ERR_INVALID, name
        w = S.inception_weights()
        for k, t in w.items():
            if k == "Conv2d_2b_3x3.bn.bias":
                continue
            s = (C.c_int64 * t.dim())(*t.shape)
            assert lib.s3d_imgfeat_set_param(h, k.encode(), C.c_void_p(t.data_ptr()), s, t.dim()) == 0, k
        fake = C.c_void_p(256)                                                # never dereferenced
        assert lib.s3d_imgfeat_features(h, fake, 1, 96, 80, 4, 64, None, None) == _lib.ERR_INVALID and b"Conv2d_2b_3x3.bn.bias" in lib.s3d_last_error()
        assert lib.s3d_imgfeat_features(h, fake, 1, 96, 80, 4, 2048, None, None) == _lib.ERR_UNSUPPORTED
        assert lib.s3d_imgfeat_features(h, fake, 1, 96, 80, 2, 64, None, None) == _lib.ERR_INVALID
        assert lib.s3d_imgfeat_features(h, fake, 0, 96, 80, 4, 64, None, None) == _lib.ERR_INVALID
        assert lib.s3d_imgfeat_stats(h, fake, fake, None) == _lib.ERR_INVALID and b"no features" in lib.s3d_last_error()
        assert lib.s3d_imgfeat_pairs(h, None, fake, None) == _lib.ERR_INVALID
        assert lib.s3d_imgfeat_profile_read(h, (C.c_double * 6)()) == _lib.ERR_INVALID
    finally:
        lib.s3d_imgfeat_destroy(h)
