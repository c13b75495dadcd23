"""GPU: the geometry evaluation (sin3dm_amd/evaluation, s3d_eval.hip) against tests/golden/eval_geometry.npz, which
tests/golden/make_golden_eval.py recorded from the reference's evaluation/patch_utils.py on the CPU.  The volumes are procedural
(tests/eval_cases.py).  Integers (occupancy, validity, order, choice, bits, counts) and the per-patch maxima are compared exactly;
only the means, which torch adds in its own order on the device, get a tolerance."""
import json
import random

import numpy as np
import pytest
import torch

import eval_cases as E
from conftest import golden
from sin3dm_amd import evaluation as ev
from sin3dm_amd.evaluation import eval_geometry

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def g():
    return golden("eval_geometry")


@pytest.fixture(scope="module")
def case_files(tmp_path_factory):
    d = tmp_path_factory.mktemp("eval_cases")
    return {case: E.write_case_files(case, str(d)) for case in E.LP_CASES}


def _same_after_round6(a, b):
    """abs <= 1e-6 between two numbers rounded to six places, taken on the integers so that 0.123457 - 0.123456 does not depend on
    how the two decimals are represented."""
    return abs(round(float(a) * 1e6) - round(float(b) * 1e6)) <= 1


def _packbits_words(vox, positions, patch_size, stride):
    """NumPy restatement of the packing: the patch's voxels in row-major order, np.packbits little-endian, as uint64 words."""
    stride = patch_size // 2 if stride is None else stride
    p = patch_size // 2
    padded = np.pad(vox, p)
    nb, nc = ((n + 2 * p - patch_size) // stride + 1 for n in vox.shape[1:])
    nw = (patch_size ** 3 + 63) // 64
    words = np.zeros((len(positions), nw), dtype=np.uint64)
    counts = np.zeros(len(positions), dtype=np.int32)
    for i, t in enumerate(positions):
        a, b, c = t // (nb * nc), (t // nc) % nb, t % nc
        patch = padded[a * stride:a * stride + patch_size, b * stride:b * stride + patch_size, c * stride:c * stride + patch_size]
        by = np.zeros(nw * 8, dtype=np.uint8)
        packed = np.packbits(patch.reshape(-1), bitorder="little")
        by[:len(packed)] = packed
        words[i] = by.view("<u8")
        counts[i] = patch.sum()
    return words, counts


def _load_case(case, case_files):
    ref_name, gens, ps, stride, patch_num, reso = E.LP_CASES[case]
    paths, ref_path = case_files[case]
    ref = ev.load_sdfgrid2vox(ref_path, resolution=reso)
    return ref, [ev.load_voxgrid(p, resolution=reso) for p in paths], ps, stride, patch_num


@pytest.mark.parametrize("case", list(E.LP_CASES))
def test_loaders_and_pooling(case, g, case_files):
    ref, gens, *_ = _load_case(case, case_files)
    for tag, vox in [("ref", ref)] + [(f"gen{i}", v) for i, v in enumerate(gens)]:
        assert vox.dtype == torch.bool and vox.is_cuda
        assert tuple(vox.shape) == tuple(g[f"{case}/{tag}/shape"]), (case, tag)
        assert int(vox.sum()) == int(g[f"{case}/{tag}/count"]), (case, tag)
        if f"{case}/{tag}/bits" in g.files:
            assert np.array_equal(np.packbits(vox.cpu().numpy().reshape(-1)), g[f"{case}/{tag}/bits"]), (case, tag)
    if case == "p11_pool":
        assert tuple(ref.shape) == (32, 26, 20) and f"{case}/gen1/bits" in g.files        # pooled, both keys read


def test_pooling_to_a_finer_grid(g, tmp_path):
    path = str(tmp_path / "up.npz")
    np.savez(path, sdf_grid=E.sdf(E.POOL_UP[0]), voxel=E.generated_occupancy(E.POOL_UP[0]))
    for tag, vox in (("ref", ev.load_sdfgrid2vox(path, resolution=E.POOL_UP[1])), ("gen", ev.load_voxgrid(path, resolution=E.POOL_UP[1]))):
        assert tuple(vox.shape) == tuple(g[f"pool_up/{tag}/shape"]) == (40, 32, 25)
        assert np.array_equal(np.packbits(vox.cpu().numpy().reshape(-1)), g[f"pool_up/{tag}/bits"]), tag


@pytest.mark.parametrize("case", list(E.LP_CASES))
def test_validity_order_and_packed_bits(case, g, case_files):
    ref, gens, ps, stride, _ = _load_case(case, case_files)
    for tag, vox in [("ref", ref)] + [(f"gen{i}", v) for i, v in enumerate(gens)]:
        want = g[f"{case}/{tag}/valid"].astype(np.int64)
        flags = ev.patch_validity(vox, ps, stride).cpu().numpy()
        na, nb, nc = (ev.patch_utils.candidate_counts(vox.shape, ps, stride))
        assert flags.shape == (na * nb * nc,) and set(np.unique(flags)) <= {0, 1}
        assert np.array_equal(np.nonzero(flags)[0], want), (case, tag)
        for word_major in (False, True):
            pt = ev.extract_valid_patches(vox, ps, stride, word_major=word_major)
            assert np.array_equal(pt.indices.cpu().numpy(), want) and len(pt) == len(want)
            words, counts = _packbits_words(vox.cpu().numpy(), want, ps, stride)
            got = pt.words.cpu().numpy().view(np.uint64)
            assert np.array_equal(got.T if word_major else got, words), (case, tag, word_major)
            assert np.array_equal(pt.counts.cpu().numpy(), counts), (case, tag, word_major)
            assert (counts >= 1).all()


@pytest.mark.parametrize("case", list(E.LP_CASES))
def test_lp_maxima_are_the_references_bits(case, g, case_files):
    """Per-patch maxima bitwise equal to the reference's; percents exactly equal; the averages and the driver's four numbers within
    1e-6 after round(6): the device's torch.mean may add in another order than the CPU's, bound (n - 1) 2^-24 mean <= 6e-5 for
    n = 1000.  Measured on an MI355X: every maximum bit-identical; the largest gap of an average 1.2e-7 (p11_pool), of Div 1.2e-8."""
    ref_vox, gens, ps, stride, patch_num = _load_case(case, case_files)
    ref = ev.extract_valid_patches(ref_vox, ps, stride, word_major=True)
    rng = random.Random(1234)
    worst = 0.0
    for i, vox in enumerate(gens):
        gen = ev.extract_valid_patches(vox, ps, stride)
        chosen = ev.shuffled_choice(rng, len(gen), patch_num)
        assert np.array_equal(chosen, g[f"{case}/gen{i}/chosen"]), (case, i)
        m = ev.lp_metrics(gen.select(chosen), ref)
        want_iou, want_f = g[f"{case}/gen{i}/max_iou"], g[f"{case}/gen{i}/max_f"]
        got_iou, got_f = m["max_iou"].cpu().numpy(), m["max_f"].cpu().numpy()
        assert got_iou.dtype == np.float32 and got_f.dtype == np.float32
        print(case, i, "n", len(chosen), "iou bits differ", int((got_iou.view(np.uint32) != want_iou.view(np.uint32)).sum()),
              "f bits differ", int((got_f.view(np.uint32) != want_f.view(np.uint32)).sum()))
        assert np.array_equal(got_iou.view(np.uint32), want_iou.view(np.uint32)), (case, i)
        assert np.array_equal(got_f.view(np.uint32), want_f.view(np.uint32)), (case, i)
        lp = g[f"{case}/gen{i}/lp"]
        gaps = (abs(m["iou_avg"] - lp[0]), abs(m["f_avg"] - lp[2]))
        worst = max(worst, *gaps)
        print(case, i, "avg gaps", gaps)
        assert m["iou_percent"] == lp[1] and m["f_percent"] == lp[3], (case, i)
        assert _same_after_round6(round(m["iou_avg"], 6), round(lp[0], 6)) and _same_after_round6(round(m["f_avg"], 6), round(lp[2], 6))
        # the other layouts of the same patches give the same bits
        m2 = ev.lp_maxima(gen.select(chosen).to_layout(True), ref.to_layout(False))
        assert torch.equal(m2[0], m["max_iou"]) and torch.equal(m2[1], m["max_f"])
    if case == "p11_32":
        assert 0 < g[f"{case}/gen0/lp"][1] < 1 and 0 < g[f"{case}/gen0/lp"][3] < 1            # a percent strictly inside (0, 1)
        assert (got_iou == 1).all() and (got_f == 1).all() and m["iou_avg"] == 1 and m["f_avg"] == 1 and m["iou_percent"] == 1
    print(case, "worst average gap", worst)


@pytest.mark.parametrize("case", list(E.LP_CASES))
def test_eval_lp_driver(case, g, case_files):
    _, _, ps, stride, patch_num, reso = E.LP_CASES[case]
    paths, ref_path = case_files[case]
    state = random.getstate()
    res = ev.eval_lp(paths, ref_path, ps, stride if stride is not None else ps // 2, patch_num, resolution=reso)
    assert random.getstate() == state                                          # the caller's global stream is untouched
    assert list(res) == ["LP-IOU-avg", "LP-IOU-percent", "LP-F-score-avg", "LP-F-score-percent"]
    want = g[f"{case}/result"]
    print(case, {k: (v, w) for (k, v), w in zip(res.items(), want)})
    for (k, v), w in zip(res.items(), want):
        assert _same_after_round6(v, w), (case, k, v, w)
    assert res["LP-IOU-percent"] == want[1] and res["LP-F-score-percent"] == want[3]


def test_pairwise_counts_and_div(g, tmp_path):
    vols = torch.stack([torch.from_numpy(E.generated_occupancy(n)) for n in E.DIV_CASE]).cuda()
    inter, union = ev.pairwise_counts(vols)
    assert inter.dtype == torch.int64 and np.array_equal(inter.cpu().numpy(), g["div/inter"])
    assert np.array_equal(union.cpu().numpy(), g["div/union"])
    assert np.array_equal(torch.diagonal(inter).cpu().numpy(), g["div/counts"])
    div = ev.pairwise_iou_dist(vols)
    print("Div", div, "reference", float(g["div/value"]), "gap", abs(div - float(g["div/value"])))
    assert _same_after_round6(round(div, 6), round(float(g["div/value"]), 6))
    paths = []
    for i, n in enumerate(E.DIV_CASE):
        paths.append(str(tmp_path / f"{i}_voxel.npz"))
        np.savez(paths[-1], **{"voxel" if i % 2 else "vox_grid": E.generated_occupancy(n)})
    res = ev.eval_div(paths, resolution=E.DIV_RESOLUTION)
    assert list(res) == ["Div"] and _same_after_round6(res["Div"], float(g["div/result"]))
    # a ragged last word: 1000 voxels are 15 words and 40 bits
    v = (torch.arange(3 * 1000, device="cuda").view(3, 10, 10, 10) % 3 == 0)
    inter, union = ev.pairwise_counts(v)
    f = v.view(3, -1)
    assert torch.equal(inter, (f[:, None] & f[None]).sum(dim=2)) and torch.equal(union, (f[:, None] | f[None]).sum(dim=2))


def test_degenerate_volumes_and_bad_arguments():
    """An empty volume has no valid patch.  A full one has those whose centre cube straddles the zero padding: the reference's
    extract_valid_patches_unfold gives 30 (patch 11, stride 5) and 90 (patch 6) on a full (20, 17, 13) volume."""
    ref = ev.extract_valid_patches(torch.from_numpy(E.reference_occupancy("ref32")).cuda(), 11, 5, word_major=True)
    for fill, n11, n6 in ((False, 0, 0), (True, 30, 90)):
        vox = torch.full((20, 17, 13), fill, dtype=torch.bool, device="cuda")
        pt = ev.extract_valid_patches(vox, 11, 5)
        assert len(pt) == n11 and pt.words.shape == (n11, 21) and pt.indices.numel() == n11
        assert int(ev.patch_validity(vox, 6).sum()) == n6
        m = ev.lp_metrics(pt, ref)
        assert m["max_iou"].shape == (n11,) and m["max_f"].shape == (n11,)
        if not fill:
            assert np.isnan(m["iou_avg"]) and np.isnan(m["f_percent"])           # n_gen == 0: nothing to average
            a, b = ev.lp_maxima(ref, pt)                                         # n_ref == 0
            assert a.shape == (len(ref),) and not a.any() and not b.any()
    torch.cuda.synchronize()
    vox = torch.zeros((20, 17, 13), dtype=torch.bool, device="cuda")
    for ps in (1, 33, 0):
        with pytest.raises(AssertionError, match="patch_size"):
            ev.patch_validity(vox, ps, 1)
    with pytest.raises(AssertionError, match="stride"):
        ev.patch_validity(vox, 11, 0)
    occ = torch.from_numpy(E.reference_occupancy("ref32")).cuda()
    for ps, stride in ((2, 2), (3, 2), (32, 4)):                                 # the ends of the supported range
        pt = ev.extract_valid_patches(occ, ps, stride)
        words, counts = _packbits_words(occ.cpu().numpy(), pt.indices.cpu().numpy(), ps, stride)
        assert len(pt) > 0 and np.array_equal(pt.words.cpu().numpy().view(np.uint64), words)
        assert np.array_equal(pt.counts.cpu().numpy(), counts)
        m = ev.lp_metrics(pt, pt)
        assert (m["max_iou"] == 1).all() and (m["max_f"] == 1).all()


def test_cli_writes_the_five_keys(g, case_files, tmp_path, capsys):
    """The command line on a temporary tree (run in-process: resolution 128 pools the 48-voxel shapes up, like any other input)."""
    src, ref = tmp_path / "samples", tmp_path / "ref"
    ref.mkdir()
    np.savez(ref / "shape.npz", sdf_grid=E.sdf("ref32"))
    for i, n in enumerate(("gen32a", "ref32", "div2")):
        (src / f"s{i}").mkdir(parents=True)
        np.savez(src / f"s{i}" / ("r128_voxel.npz" if i else "voxel.npz"), **{"voxel" if i else "vox_grid": E.generated_occupancy(n, "ref32")})
    out = tmp_path / "result.json"
    res = eval_geometry.main(["-s", str(src), "-r", str(ref), "--patch_num", "50", "-o", str(out)])
    saved = json.load(open(out))
    keys = ["LP-IOU-avg", "LP-IOU-percent", "LP-F-score-avg", "LP-F-score-percent", "Div"]
    assert list(saved) == keys and saved == res
    assert all(isinstance(saved[k], float) and 0 <= saved[k] <= 1 for k in keys), saved
    err = capsys.readouterr().err
    assert err.count("\n") == 1 and all(w in err for w in ("SSFID", "SIFID", "LPIPS", "offline"))
    eval_geometry.main(["-s", str(src), "-r", str(ref), "--patch_num", "50"])
    assert json.load(open(str(src) + "_eval.json")) == saved
