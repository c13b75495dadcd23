"""GPU: SSFID on the device (sin3dm_amd/evaluation/ssfid.py, s3d_ssfid.hip) against the float64 restatement of
tests/ssfid_cases.py, which tests/test_ssfid_host.py pins to the reference's modules (tests/golden/ssfid.npz).  Every activation,
mean and covariance is held at ten times the reference's own float32-versus-float64 gap on that input, never below one float32
ulp of the statistic's largest magnitude; repeated calls, fresh handles and reused handles give the same bits.

Worst errors measured on an MI355X (each next to its bound) are in DESIGN.md §21."""
import json
import os

import numpy as np
import pytest
import torch

import eval_cases as E
import ssfid_cases as S
from conftest import golden
from sin3dm_amd import evaluation as ev
from sin3dm_amd.evaluation import eval_geometry

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def g():
    return golden("ssfid")


@pytest.fixture(scope="module")
def net():
    return ev.VoxelClassifier(S.weights())


def _vox(name):
    return torch.from_numpy(S.volume(name)).cuda()


@pytest.fixture(scope="module")
def device_stats(net):
    """{(volume, layer): (mu, sigma)} as float64 NumPy, computed once."""
    return {(name, layer): net.features(_vox(name), layer) for name in S.volume_names() for layer in S.LAYERS}


@pytest.mark.parametrize("layer", S.LAYERS)
def test_activations_and_statistics_against_the_restatement(layer, g, net):
    for name in S.volume_names():
        act_r, mu_r, sigma_r = S.restated(name, layer)
        mu, sigma, act = net.features(_vox(name), layer, return_activations=True)
        act = act.cpu().numpy()
        key = f"{name}/{layer}"
        assert act.shape == act_r.shape and act.dtype == np.float32 and mu.dtype == sigma.dtype == np.float64
        assert np.isfinite(act).all() and np.isfinite(mu).all() and np.isfinite(sigma).all(), key
        for what, got, want in (("act", act, act_r), ("mu", mu, mu_r), ("sigma", sigma, sigma_r)):
            err, tol = float(np.max(np.abs(got - want))), S.bound(g[f"{key}/gap_{what}"], want)
            print(f"{key} {what}: err {err:.3e} bound {tol:.3e}")
            assert err <= tol, (key, what, err, tol)
        if name == "free":                                                  # an empty volume: exact zeros, as in exact arithmetic
            assert not act.any() and not mu.any() and not sigma.any()


@pytest.mark.parametrize("layer", S.LAYERS)
def test_statistics_tail_against_the_returned_activations(layer, net):
    """Fewer rows than one 64-row stage (24), exactly one stage (64), a 128-row span plus a full and a partial stage (240), many
    spans (2080, 8640): the Gram and covariance alone, at the bound of tests/ssfid_cases.check_tail."""
    cases = {name: _vox(name) for name in ("rank_a", "ref32", "ref48")}
    if layer == 1:
        cases["ones 16 x 16 x 3"] = torch.ones(16, 16, 3, dtype=torch.bool, device="cuda")
    for name, vox in cases.items():
        mu, sigma, act = net.features(vox, layer, return_activations=True)
        S.check_tail(f"{name}/{layer}", act.cpu().numpy(), mu, sigma)


def test_same_bits_call_after_call_and_handle_after_handle(net):
    vox = _vox("ref40")
    for layer in S.LAYERS:
        a = net.features_device(vox, layer, return_activations=True)
        b = net.features_device(vox, layer, return_activations=True)
        c = ev.VoxelClassifier(S.weights()).features_device(vox, layer, return_activations=True)
        for x, y, z in zip(a, b, c):
            assert torch.equal(x, y) and torch.equal(x, z), layer


def test_one_handle_across_shapes_equals_fresh_handles():
    """large -> small -> large: the workspace is reused, and a value read without being written would differ, because the call
    before the last one left another shape's values there."""
    order = ("long", "rank_a", "ref48", "gen48b", "long")
    reused = ev.VoxelClassifier(S.weights())
    for layer in (2, 1):
        got = [reused.features_device(_vox(n), layer, return_activations=True) for n in order]
        for name, out in zip(order, got):
            fresh = ev.VoxelClassifier(S.weights()).features_device(_vox(name), layer, return_activations=True)
            for x, y in zip(out, fresh):
                assert torch.equal(x, y), (name, layer)
        for x, y in zip(got[0], got[-1]):
            assert torch.equal(x, y), layer


@pytest.mark.parametrize("layer", S.LAYERS)
def test_pair_distances_against_the_fixture(layer, g, device_stats):
    for pair, (r, gen) in S.PAIRS.items():
        d = ev.frechet_distance(*device_stats[(r, layer)], *device_stats[(gen, layer)])
        assert np.isfinite(d), pair
        if pair == "prank" and layer == 2:                                  # singular covariances: no parity with sqrtm is claimed
            continue
        want, tol = float(g[f"{pair}/{layer}/fd"]), max(10 * float(g[f"{pair}/{layer}/fd_gap"]), 1e-9)
        print(f"{pair}/{layer}: {d!r} want {want!r} err {abs(d - want):.3e} bound {tol:.3e}")
        assert abs(d - want) <= tol, (pair, layer, d, want)
        same = ev.frechet_distance(*device_stats[(r, layer)], *device_stats[(r, layer)])
        assert abs(same) <= 1e-12 * 2 * np.trace(device_stats[(r, layer)][1])


@pytest.fixture(scope="module")
def e2e_files(tmp_path_factory):
    d = tmp_path_factory.mktemp("ssfid_e2e")
    paths, ref_path = E.write_case_files(S.E2E_CASE, str(d))
    weights = str(d / "Clsshapenet_128.pth")
    full = dict(S.weights())
    full["conv_3.bias"] = torch.zeros(128)                                  # a key of the real file that is not read
    torch.save(full, weights)
    return paths, ref_path, weights


@pytest.mark.parametrize("layer", S.LAYERS)
def test_eval_ssfid_end_to_end(layer, g, e2e_files):
    paths, ref_path, weights = e2e_files
    res = ev.eval_ssfid(paths, ref_path, weights, out_layer=layer, resolution=S.E2E_RESOLUTION)
    want = g[f"e2e/{layer}"]
    print(layer, res, want.tolist())
    assert list(res) == ["SSFID_avg", "SSFID_std"] and all(isinstance(v, float) for v in res.values())
    assert abs(res["SSFID_avg"] - want[0]) <= 2e-6 and abs(res["SSFID_std"] - want[1]) <= 2e-6
    np.savez(os.path.join(os.path.dirname(paths[0]), "small_voxel.npz"), vox_grid=S.volume("gen32a"))
    with pytest.raises(RuntimeError, match="Generated shape and reference shape shall have equal size."):
        ev.eval_ssfid([os.path.join(os.path.dirname(paths[0]), "small_voxel.npz")], ref_path, weights, resolution=S.E2E_RESOLUTION)


def test_cli_three_ways(e2e_files, tmp_path, capsys):
    """In-process on a temporary tree, at the command line's resolution of 128 (the 32-voxel shapes are pooled up)."""
    _, _, weights = e2e_files
    src, ref = tmp_path / "samples", tmp_path / "ref"
    ref.mkdir()
    np.savez(ref / "shape.npz", sdf_grid=E.sdf("ref32"))
    for i, n in enumerate(("gen32a", "div2")):
        (src / f"s{i}").mkdir(parents=True)
        np.savez(src / f"s{i}" / "voxel.npz", vox_grid=E.generated_occupancy(n, "ref32"))
    gen = [str(src / f"s{i}" / "voxel.npz") for i in range(2)]
    five = ["LP-IOU-avg", "LP-IOU-percent", "LP-F-score-avg", "LP-F-score-percent", "Div"]
    out = tmp_path / "with.json"
    capsys.readouterr()
    res = eval_geometry.main(["-s", str(src), "-r", str(ref), "--patch_num", "50", "--ssfid_weights", weights, "-o", str(out)])
    err = capsys.readouterr().err
    saved = json.load(open(out))
    assert list(saved) == ["SSFID_avg", "SSFID_std"] + five and saved == res
    assert err.count("\n") == 1 and "SIFID" in err and "LPIPS" in err and "SSFID" not in err
    direct = ev.eval_ssfid(gen, str(ref / "shape.npz"), weights)
    assert (saved["SSFID_avg"], saved["SSFID_std"]) == (direct["SSFID_avg"], direct["SSFID_std"]) and saved["SSFID_avg"] > 0

    plain = eval_geometry.main(["-s", str(src), "-r", str(ref), "--patch_num", "50", "-o", str(tmp_path / "without.json")])
    err = capsys.readouterr().err
    assert list(plain) == five == list(json.load(open(tmp_path / "without.json"))) and all(plain[k] == saved[k] for k in five)
    assert err.count("\n") == 1 and err.strip() == eval_geometry.NOT_COMPUTED

    one = eval_geometry.main(["-s", str(src), "-r", str(ref), "--patch_num", "50", "--ssfid_weights", weights, "--ssfid_layer", "1",
                              "-o", str(tmp_path / "layer1.json")])
    direct1 = ev.eval_ssfid(gen, str(ref / "shape.npz"), weights, out_layer=1)
    assert list(one) == ["SSFID_avg", "SSFID_std"] + five and one["SSFID_avg"] == direct1["SSFID_avg"] != saved["SSFID_avg"]


def test_refusals(net):
    vox = _vox("ref32")
    for layer in (3, 4):
        with pytest.raises(NotImplementedError, match="out_layer"):
            net.features(vox, layer)
    with pytest.raises(AssertionError, match="axis 1"):
        net.features(torch.ones(16, 1, 16, dtype=torch.bool, device="cuda"), 1)
    with pytest.raises(AssertionError, match="axis 2"):
        net.features(torch.ones(16, 16, 3, dtype=torch.bool, device="cuda"), 2)
    with pytest.raises(AssertionError, match="has not been set"):
        ev.VoxelClassifier().features(vox, 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        net.features(vox.cpu(), 2)
    mu, sigma = net.features(torch.ones(16, 16, 3, dtype=torch.bool, device="cuda"), 1)      # odd extent: floor(3 / 2) = 1
    assert mu.shape == (32,) and sigma.shape == (32, 32) and np.isfinite(sigma).all()
