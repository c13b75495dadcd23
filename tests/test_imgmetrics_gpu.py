"""MI355X: SIFID and LPIPS on the device (s3d_imgfeat.hip, sin3dm_amd/evaluation/{sifid,lpips,eval_full}.py) against the
reference's own modules as recorded in tests/golden/imgmetrics.npz.  Every tolerance is imgmetrics_cases.bound: ten times the
reference's float32-versus-float64 gap on that input, never below one float32 ulp of the largest magnitude.
Activations, mu and sigma are compared with the float64 restatement, which tests/test_imgmetrics_host.py pins to the fixture;
distances and LPIPS values with the fixture's numbers."""
import json
import os

import numpy as np
import pytest
import torch

import imgmetrics_cases as S
from conftest import golden
from sin3dm_amd import _lib
from sin3dm_amd.evaluation import eval_full, eval_renders, lpips as L, sifid as F
from sin3dm_amd.evaluation.ssfid import frechet_distance

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def stem():
    return F.InceptionStem(S.inception_weights())


@pytest.fixture(scope="module")
def alex():
    return L.AlexNetLpips(S.alexnet_weights(), S.lpips_linear())


@pytest.fixture(scope="module")
def stats(stem):
    """{(image, dims): (mu, sigma)} of every image singly, computed once."""
    out = {}
    for dims in S.DIMS:
        for name in S.IMAGES:
            mu, sigma = stem.statistics(S.image(name), dims)
            out[(name, dims)] = (mu[0], sigma[0])
    return out


def _check(what, got, want, gap):
    err, b = float(np.max(np.abs(np.asarray(got, dtype=np.float64) - want))), S.bound(gap, want)
    print(what, "err", err, "bound", b)
    assert np.all(np.isfinite(got)) and err <= b, (what, err, b)


@pytest.mark.parametrize("dims", S.DIMS)
@pytest.mark.parametrize("name", S.PARITY)
def test_sifid_activations_and_statistics(stem, name, dims):
    g = golden("imgmetrics")
    key = f"sifid/{name}/{dims}"
    mu, sigma, acts = stem.statistics(S.image(name), dims, return_activations=True)
    r_acts, r_mu, r_sigma = S.sifid_restated(name, dims)
    assert len(acts) == len(r_acts) == (3 if dims == 64 else 5)
    for l, (a, r) in enumerate(zip(acts, r_acts)):
        assert tuple(a.shape[1:]) == r.shape
        _check(f"{key} unit {l}", a[0].cpu().numpy(), r, g[f"{key}/gap_act"][l])
    _check(f"{key} mu", mu[0], r_mu, g[f"{key}/gap_mu"])
    _check(f"{key} sigma", sigma[0], r_sigma, g[f"{key}/gap_sigma"])
    _check(f"{key} mu (fixture)", mu[0], g[f"{key}/mu"].astype(np.float64), g[f"{key}/gap_mu"])


@pytest.mark.parametrize("dims", S.DIMS)
def test_sifid_pair_distances(stats, dims):
    g = golden("imgmetrics")
    for pair, (r, gen) in S.SIFID_PAIRS.items():
        fd = frechet_distance(*stats[(r, dims)], *stats[(gen, dims)])
        _check(f"sifid/{pair}/{dims}", fd, float(g[f"sifid/{pair}/{dims}/fd"]), g[f"sifid/{pair}/{dims}/fd_gap"])
        same = frechet_distance(*stats[(r, dims)], *stats[(r, dims)])
        assert abs(same) < 1e-6 * max(1.0, fd), (pair, same)


def test_singular_covariance_is_finite(stats):
    """36 rows for 192 channels: no parity is claimed (DESIGN.md §21's `prank`), everything stays finite."""
    (m0, s0), (m1, s1) = (stats[(n, 192)] for n in S.SINGULAR_PAIR)
    assert np.all(np.isfinite(s0)) and np.all(np.isfinite(s1)) and np.linalg.matrix_rank(s0) < 192
    assert np.isfinite(frechet_distance(m0, s0, m1, s1))


@pytest.mark.parametrize("dims", S.DIMS)
def test_batch_of_three_is_the_images_singly(stem, stats, dims):
    g = golden("imgmetrics")
    batch = np.stack([S.image(n) for n in S.BATCH])
    mu, sigma, acts = stem.statistics(batch, dims, return_activations=True)
    for k, name in enumerate(S.BATCH):
        key = f"sifid/{name}/{dims}"
        r_acts, r_mu, r_sigma = S.sifid_restated(name, dims)
        _check(f"{key} batched last unit", acts[-1][k].cpu().numpy(), r_acts[-1], g[f"{key}/gap_act"][-1])
        _check(f"{key} batched mu", mu[k], r_mu, g[f"{key}/gap_mu"])
        _check(f"{key} batched sigma", sigma[k], r_sigma, g[f"{key}/gap_sigma"])
        # a tile never straddles two images and every sum has its image's own order: the same bits
        assert np.array_equal(mu[k], stats[(name, dims)][0]) and np.array_equal(sigma[k], stats[(name, dims)][1])


@pytest.mark.parametrize("names, dims", [(("a0",), 64), (("a0",), 192), (("d",), 64), (S.BATCH, 64), (S.BATCH, 192)])
def test_statistics_tail_against_the_returned_activations(stem, names, dims):
    """320 rows at dims 192, 6305 rows (six spans of 1024 and a ragged seventh) and a batch: the Gram and covariance alone, at the
    bound of tests/ssfid_cases.check_tail."""
    mu, sigma, acts = stem.statistics(np.stack([S.image(n) for n in names]), dims, return_activations=True)
    rows = acts[-1].cpu().numpy()
    for k, name in enumerate(names):
        S.check_tail(f"{name}/{dims}", rows[k].reshape(-1, dims), mu[k], sigma[k])


def test_same_bits_call_after_call_on_reused_and_fresh_handles(stem, stats):
    fresh = F.InceptionStem(S.inception_weights())
    for name in ("d", "s", "d"):                                            # one handle large -> small -> large
        for net in (stem, fresh):
            mu, sigma = net.statistics(S.image(name), 192)
            assert np.array_equal(mu[0], stats[(name, 192)][0]) and np.array_equal(sigma[0], stats[(name, 192)][1]), name
    mu, sigma = fresh.statistics(S.image("d"), 64)
    assert np.array_equal(mu[0], stats[("d", 64)][0]) and np.array_equal(sigma[0], stats[("d", 64)][1])
    fresh.close()


def test_input_forms_agree(stem, stats, tmp_path):
    """A device tensor, a NumPy array, RGB without alpha and a PNG path give the same bits: alpha is read but never applied."""
    from sin3dm_amd.encoding.isosurface import png_bytes
    img = S.image("a0")
    p = tmp_path / "000.png"
    p.write_bytes(png_bytes(img))
    for form in (torch.from_numpy(img.copy()).cuda(), img[..., :3], [str(p)]):
        mu, sigma = stem.statistics(form, 64)
        assert np.array_equal(mu[0], stats[("a0", 64)][0]) and np.array_equal(sigma[0], stats[("a0", 64)][1])


@pytest.mark.parametrize("pair", tuple(S.LPIPS_PAIRS))
def test_lpips_maps_terms_and_total(alex, pair):
    g = golden("imgmetrics")
    a, b = S.LPIPS_PAIRS[pair]
    total, layers, acts = alex.pair_matrix_device(np.stack([S.image(a)[..., :3], S.image(b)[..., :3]]), return_layers=True, return_activations=True)
    total, layers = total.cpu().numpy(), layers.cpu().numpy()
    r_terms, r_total, r_maps = S.lpips_restated(a, b)
    key = f"lpips/{pair}"
    for l in range(5):
        _check(f"{key} map {l}", acts[l][0].cpu().numpy(), r_maps[l], g[f"{key}/gap_act"][l])
    _check(f"{key} terms", layers[:, 0, 1], g[f"{key}/terms"], np.max(g[f"{key}/gap_terms"]))
    _check(f"{key} total", total[0, 1], float(g[f"{key}/total"]), g[f"{key}/gap_total"])
    _check(f"{key} total (restated)", total[0, 1], r_total, g[f"{key}/gap_total"])


def test_lpips_matrix_of_the_batch(alex):
    g = golden("imgmetrics")
    batch = np.stack([S.image(n) for n in S.BATCH])                         # RGBA: the fourth channel is not read
    m = alex.pair_matrix(batch)
    assert m.shape == (3, 3) and np.array_equal(m, m.T) and np.all(np.diag(m) == 0.0)
    for pair, (i, j) in (("pa", (0, 1)), ("pa2", (0, 2)), ("pa12", (1, 2))):
        _check(f"lpips/{pair} in the batch", m[i, j], float(g[f"lpips/{pair}/total"]), g[f"lpips/{pair}/gap_total"])
    two = alex.pair_matrix(batch[:2])
    assert np.array_equal(two, m[:2, :2])                                   # the same bits whatever the batch
    fresh = L.AlexNetLpips(S.alexnet_weights(), S.lpips_linear())
    big = fresh.pair_matrix(np.stack([S.image("d"), S.image("d1")]))
    assert np.array_equal(fresh.pair_matrix(batch), m)                      # large -> small on a fresh handle
    assert np.array_equal(fresh.pair_matrix(np.stack([S.image("d"), S.image("d1")])), big)
    fresh.close()


def test_refusals(stem, alex):
    with pytest.raises(NotImplementedError):
        stem.statistics(S.image("a0"), 2048)
    with pytest.raises(NotImplementedError):
        stem.statistics(S.image("a0"), 100)
    with pytest.raises(ValueError, match="too small"):
        alex.pair_matrix(np.stack([S.image("s"), S.image("s1")]))
    with pytest.raises(ValueError, match="too small"):
        stem.statistics(np.zeros((2, 2, 3), dtype=np.uint8), 64)
    with pytest.raises(_lib.Sin3DMHipError, match="no CPU fallback"):
        stem.statistics(torch.from_numpy(S.image("a0").copy()), 64)
    with pytest.raises(ValueError):
        stem.statistics(S.image("a0").astype(np.float32), 64)
    empty = F.InceptionStem()
    with pytest.raises(AssertionError, match="has not been set"):
        empty.statistics(S.image("a0"), 64)
    with pytest.raises(AssertionError, match="no features"):
        _lib.check(empty._lib.s3d_imgfeat_stats(empty._h, _lib.ptr(torch.zeros(1, device="cuda")), _lib.ptr(torch.zeros(1, device="cuda")), None))
    no_lin = L.AlexNetLpips(S.alexnet_weights())
    with pytest.raises(AssertionError, match="lpips_weights.0.main.1.weight"):
        no_lin.pair_matrix(np.stack([S.image("a0"), S.image("a1")]))


def test_end_to_end_dicts(stem, alex, tmp_path):
    g = golden("imgmetrics")
    gen, ref = S.write_tree(str(tmp_path))
    for dims in S.DIMS:
        res = F.eval_sifid(gen, ref, stem, dims)
        assert list(res) == [f"mv_sifid_dim{dims}"]
        _check(f"e2e sifid {dims}", res[f"mv_sifid_dim{dims}"], float(g[f"e2e/sifid{dims}"]), g[f"e2e/sifid{dims}/gap"])
    res = L.eval_lpips(gen, alex)
    assert list(res) == ["mv_lpips"]
    _check("e2e lpips", res["mv_lpips"], float(g["e2e/lpips"]), g["e2e/lpips/gap"])


def test_eval_full_writes_the_ten_keys(tmp_path):
    """eval_full on a temporary tree: the ten keys in eval_full.py's order, the first seven equal to eval_geometry's."""
    import eval_cases as E
    import ssfid_cases as SS
    from sin3dm_amd.evaluation import eval_geometry
    g = golden("imgmetrics")
    root = str(tmp_path)
    gen_dirs, ref_dir = S.write_tree(root)
    src, ref = os.path.join(root, "src"), os.path.join(root, "ref")
    np.savez(os.path.join(ref, "shape.npz"), sdf_grid=E.sdf("ref32"))
    for j, n in enumerate(("gen32a", "div2", "gen32a")):
        np.savez(os.path.join(src, f"sample_{j}", "voxel.npz"), vox_grid=E.generated_occupancy(n, "ref32"))
    ck = {k: os.path.join(root, k + ".pth") for k in ("ssfid", "inception", "alexnet", "lpips")}
    torch.save(SS.weights(), ck["ssfid"])
    torch.save(S.inception_weights(), ck["inception"])
    torch.save(S.alexnet_weights(), ck["alexnet"])
    torch.save(S.lpips_linear(), ck["lpips"])
    common = ["-s", src, "-r", ref, "--patch_num", "50", "--ssfid_weights", ck["ssfid"]]
    weights = ["--inception_weights", ck["inception"], "--alexnet_weights", ck["alexnet"], "--lpips_weights", ck["lpips"]]
    full = eval_full.main(common + weights + ["-o", os.path.join(root, "full.json")])
    geo = eval_geometry.main(common + ["-o", os.path.join(root, "geo.json")])
    assert list(full) == list(eval_full.KEYS) and len(full) == 10
    assert list(geo) == list(full)[:7] and all(full[k] == geo[k] for k in geo)
    assert json.load(open(os.path.join(root, "full.json"))) == full
    renders = eval_renders.main(["-s", src, "-r", ref] + weights + ["-o", os.path.join(root, "renders.json")])
    assert list(renders) == list(eval_full.KEYS[7:]) and all(renders[k] == full[k] for k in renders)
    _check("eval_full lpips", full["mv_lpips"], float(g["e2e/lpips"]), g["e2e/lpips/gap"])
    _check("eval_full sifid 64", full["mv_sifid_dim64"], float(g["e2e/sifid64"]), g["e2e/sifid64/gap"])
