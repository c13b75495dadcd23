"""Writes tests/golden/imgmetrics.npz from the reference's evaluation/sifid.py, evaluation/inception.py and evaluation/lpips.py on
the CPU:

    python tests/golden/make_golden_imgmetrics.py /path/to/reference

torchvision is not needed and nothing is fetched: stub `torchvision` / `torchvision.models` modules are put into sys.modules
before the reference's modules are imported, whose `inception_v3` and `alexnet` return hand-built stacks (torchvision's
BasicConv2d units and AlexNet `features`) carrying the procedural weights of tests/imgmetrics_cases.py.  The reference's LPIPS
reads lpips_weights.ckpt from the working directory: a temporary one that holds a copy.

The fixture stores results only, plus the 1152 linear LPIPS weights as plain arrays (lin/0..4).  Per image `v` and dims `D`:
  sifid/v/D/mu                         calculate_activation_statistics of the float32 modules (float32)
  sifid/v/D/sigma_diag, /sigma_sub     the diagonal and every eighth row and column of its float64 covariance
  sifid/v/D/gap_act [units], /gap_mu, /gap_sigma
                                       the reference's own float32-versus-float64 gap on this input: the largest absolute
                                       difference to the same modules in .double() on the same float32 input
per pair `p` of imgmetrics_cases.SIFID_PAIRS and dims: sifid/p/D/fd, /fd_gap (calculate_frechet_distance of the float32 and of
the float64 statistics); act/D: every eighth row of the last unit's float32 activations of imgmetrics_cases.ACT_CASE;
per pair of LPIPS_PAIRS: lpips/p/terms [5], /total, /gap_terms [5], /gap_total, /gap_act [5] (first image's maps);
e2e/sifid64, e2e/sifid192, e2e/lpips: the reference's calculate_multiview_* over imgmetrics_cases.write_tree, each with /gap.
"""
import os
import shutil
import sys
import tempfile
import types

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))                     # tests/
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))    # the repository

import imgmetrics_cases as S  # noqa: E402


class BasicConv2d(nn.Module):
    """torchvision.models.inception.BasicConv2d"""

    def __init__(self, cin, cout, **kw):
        super().__init__()
        self.conv = nn.Conv2d(cin, cout, bias=False, **kw)
        self.bn = nn.BatchNorm2d(cout, eps=0.001)

    def forward(self, x):
        return F.relu(self.bn(self.conv(x)), inplace=True)


def stub_inception(**_):
    m = nn.Module()
    for name, cin, cout, k, stride, pad, _ in S.STEM:
        setattr(m, name, BasicConv2d(cin, cout, kernel_size=k, stride=stride, padding=pad))
    m.load_state_dict(S.inception_weights(), strict=False)
    return m


def stub_alexnet(**_):
    m = nn.Module()
    m.features = nn.Sequential(
        nn.Conv2d(3, 64, 11, 4, 2), nn.ReLU(inplace=True), nn.MaxPool2d(3, 2), nn.Conv2d(64, 192, 5, padding=2), nn.ReLU(inplace=True),
        nn.MaxPool2d(3, 2), nn.Conv2d(192, 384, 3, padding=1), nn.ReLU(inplace=True), nn.Conv2d(384, 256, 3, padding=1), nn.ReLU(inplace=True),
        nn.Conv2d(256, 256, 3, padding=1), nn.ReLU(inplace=True), nn.MaxPool2d(3, 2))
    m.load_state_dict(S.alexnet_weights())
    return m


def install_stubs():
    tv, models = types.ModuleType("torchvision"), types.ModuleType("torchvision.models")
    models.inception_v3, models.alexnet = stub_inception, stub_alexnet
    models.Inception_V3_Weights = types.SimpleNamespace(IMAGENET1K_V1=None)
    models.AlexNet_Weights = types.SimpleNamespace(IMAGENET1K_V1=None)
    tv.models = models
    sys.modules["torchvision"], sys.modules["torchvision.models"] = tv, models


def main(ref_root):
    install_stubs()
    sys.path.insert(0, os.path.join(ref_root, "evaluation"))
    cwd = os.getcwd()
    tmp = tempfile.mkdtemp()
    shutil.copy(os.path.join(ref_root, "evaluation", "lpips_weights.ckpt"), tmp)
    os.chdir(tmp)
    try:
        out = run()
    finally:
        os.chdir(cwd)
        shutil.rmtree(tmp)
    path = os.path.join(HERE, "imgmetrics.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 1024 * 1024


def run():
    import sifid as RS
    import lpips as RL
    from inception import InceptionV3
    from sin3dm_amd.encoding.isosurface import png_bytes

    out = {}
    lin_state = torch.load("lpips_weights.ckpt", map_location="cpu")
    for l in range(5):
        out[f"lin/{l}"] = lin_state[f"lpips_weights.{l}.main.1.weight"].numpy().reshape(-1).astype(np.float32)
    assert sum(out[f"lin/{l}"].size for l in range(5)) == 1152
    lin = {k: v for k, v in lin_state.items() if k.startswith("lpips_weights.")}

    def png(name):
        p = os.path.join(os.getcwd(), name + ".png")
        if not os.path.exists(p):
            with open(p, "wb") as fh:
                fh.write(png_bytes(S.image(name)))
        return p

    # ---------------------------------------------------------------- SIFID
    stats32, stats64, worst = {}, {}, {}
    for dims in S.DIMS:
        model = InceptionV3([InceptionV3.BLOCK_INDEX_BY_DIM[dims]]).eval()
        model64 = InceptionV3([InceptionV3.BLOCK_INDEX_BY_DIM[dims]], normalize_input=False).double().eval()
        for name in S.IMAGES:
            mu32, sigma32 = RS.calculate_activation_statistics([png(name)], model, 1, dims, "cpu")
            assert mu32.dtype == np.float32 and sigma32.dtype == np.float64
            x = torch.from_numpy(RS.imread(png(name)).astype(np.float32)[None, :, :, 0:3].transpose(0, 3, 1, 2))
            assert torch.equal(2 * x - 1, S.sifid_input(S.image(name)))          # imread's samples are the restatement's
            a32, a64 = [], []
            with torch.no_grad():
                y32, y64 = 2 * x - 1, (2 * x - 1).double()
                for b32, b64 in zip(model.blocks, model64.blocks):
                    for m32, m64 in zip(b32, b64):
                        y32, y64 = m32(y32), m64(y64)
                        if not isinstance(m32, nn.MaxPool2d):
                            a32.append(y32[0].permute(1, 2, 0).numpy().copy())
                            a64.append(y64[0].permute(1, 2, 0).numpy().copy())
            rows32, rows64 = a32[-1].reshape(-1, dims), a64[-1].reshape(-1, dims)
            assert np.array_equal(mu32, np.mean(rows32, axis=0)) and np.array_equal(sigma32, np.cov(rows32, rowvar=False))
            mu64, sigma64 = np.mean(rows64, axis=0), np.cov(rows64, rowvar=False)
            r_acts, r_mu, r_sigma = S.sifid_restated(name, dims)                  # the restatement is the .double() modules to round-off
            assert all(np.max(np.abs(a - b)) < 1e-11 for a, b in zip(a64, r_acts)), (name, dims)
            assert np.max(np.abs(mu64 - r_mu)) < 1e-11 and np.max(np.abs(sigma64 - r_sigma)) < 1e-11, (name, dims)
            if name in S.PARITY:                                                  # condition 1: rows > C, no constant channel
                assert rows64.shape[0] > dims and np.all(rows64.std(axis=0) > 1e-3), (name, dims, rows64.shape, rows64.std(axis=0).min())
            key = f"sifid/{name}/{dims}"
            out[f"{key}/mu"] = mu32
            out[f"{key}/sigma_diag"], out[f"{key}/sigma_sub"] = np.diag(sigma32).copy(), sigma32[::8, ::8].copy()
            gaps = dict(act=np.asarray([np.max(np.abs(a - b)) for a, b in zip(a32, a64)]), mu=np.max(np.abs(mu32 - mu64)),
                        sigma=np.max(np.abs(sigma32 - sigma64)))
            for k, v in gaps.items():
                out[f"{key}/gap_{k}"] = np.asarray(v, dtype=np.float64)
                worst[(dims, k)] = max(worst.get((dims, k), 0.0), float(np.max(v)))
            stats32[(name, dims)], stats64[(name, dims)] = (mu32, sigma32), (mu64, sigma64)
            if name == S.ACT_CASE:
                out[f"act/{dims}"] = rows32[::8].copy()
            print(key, "rows", rows64.shape[0], "max|act|", float(np.max(a64[-1])), "max|sigma|", float(np.max(np.abs(sigma64))),
                  {k: np.asarray(v).tolist() for k, v in gaps.items()})
        for pair, (r, g) in list(S.SIFID_PAIRS.items()) + [("psing", S.SINGULAR_PAIR)]:
            fd32 = float(np.real(RS.calculate_frechet_distance(*stats32[(r, dims)], *stats32[(g, dims)])))
            fd64 = float(np.real(RS.calculate_frechet_distance(*stats64[(r, dims)], *stats64[(g, dims)])))
            out[f"sifid/{pair}/{dims}/fd"], out[f"sifid/{pair}/{dims}/fd_gap"] = np.float64(fd32), np.float64(abs(fd32 - fd64))
            print("sifid", pair, dims, "fd", fd32, "gap", abs(fd32 - fd64))
            if pair != "psing":                                                   # condition 2
                assert 10 * abs(fd32 - fd64) < 1e-3 * fd32, (pair, dims, fd32, fd64)
    print("worst sifid gaps", worst)

    # ---------------------------------------------------------------- LPIPS
    lp32 = RL.LPIPS().eval()
    lp64 = RL.LPIPS().double().eval()
    aw = S.alexnet_weights()

    def lpips64(xa, xb):
        """The reference's LPIPS.forward body on the .double() modules, fed the float32-normalised input."""
        fa, fb = lp64.alexnet(xa), lp64.alexnet(xb)
        terms = [float(torch.mean(c(((RL.normalize(a) - RL.normalize(b)) ** 2)))) for a, b, c in zip(fa, fb, lp64.lpips_weights)]
        return np.asarray(terms), fa

    with torch.no_grad():
        for pair, (a, b) in S.LPIPS_PAIRS.items():
            ia, ib = ((torch.from_numpy(((np.asarray(S.image(n))[..., :3] / 255.)[None] - 0.5) / 0.5).permute(0, 3, 1, 2)).type(torch.FloatTensor)
                      for n in (a, b))
            total32 = float(lp32(ia, ib))
            xa, xb = ((i - lp32.mu) / lp32.sigma for i in (ia, ib))
            assert torch.equal(xa, S.lpips_input(S.image(a)))
            fa, fb = lp32.alexnet(xa), lp32.alexnet(xb)
            terms32 = np.asarray([float(torch.mean(c((RL.normalize(p) - RL.normalize(q)) ** 2))) for p, q, c in zip(fa, fb, lp32.lpips_weights)])
            terms64, fa64 = lpips64(xa.double(), xb.double())
            r_terms, r_total, r_maps = S.lpips_restate(S.image(a), S.image(b), aw, lin)
            assert np.max(np.abs(r_terms - terms64)) < 1e-13 and abs(r_total - terms64.sum()) < 1e-13, (pair, r_terms, terms64)
            assert abs(np.float32(terms32.sum()) - total32) <= 2e-7 * total32
            key = f"lpips/{pair}"
            out[f"{key}/terms"], out[f"{key}/total"] = terms32, np.float64(total32)
            out[f"{key}/gap_terms"], out[f"{key}/gap_total"] = np.abs(terms32 - terms64), np.float64(abs(total32 - terms64.sum()))
            out[f"{key}/gap_act"] = np.asarray([float((p.double() - q).abs().max()) for p, q in zip(fa, fa64)])
            print(key, "total", total32, "gap", out[f"{key}/gap_total"], "terms", terms32, "act gaps", out[f"{key}/gap_act"])
            assert 10 * out[f"{key}/gap_total"] < 1e-3 * total32, pair
        small = torch.zeros(1, 3, 40, 40)
        try:
            lp32(small, small)
            raise AssertionError("the reference accepts a 40 x 40 image")
        except RuntimeError as e:
            print("40 x 40:", str(e)[:100])

    # ---------------------------------------------------------------- end to end
    root = os.path.join(os.getcwd(), "tree")
    gen, ref = S.write_tree(root)
    from sin3dm_amd.evaluation.ssfid import frechet_distance
    for dims in S.DIMS:
        res = RS.calculate_multiview_sifid_given_paths(gen, ref, device="cpu", dims=dims)
        views = []
        for i in range(S.E2E_VIEWS):
            _, mr, sr = S.sifid_restated(S.E2E_TREE["ref"][i], dims)
            views.append(np.mean([frechet_distance(mr, sr, *S.sifid_restated(names[i], dims)[1:]) for names in S.E2E_TREE["gen"]]))
        out[f"e2e/sifid{dims}"] = np.float64(res[f"mv_sifid_dim{dims}"])
        out[f"e2e/sifid{dims}/gap"] = np.float64(abs(res[f"mv_sifid_dim{dims}"] - np.mean(views)))
        print("e2e", res, "gap", out[f"e2e/sifid{dims}/gap"])
    res = RL.calculate_multiview_lpips_given_paths(gen, device="cpu")
    views = []
    for i in range(S.E2E_VIEWS):
        names = [g[i] for g in S.E2E_TREE["gen"]]
        views.append(np.mean([S.lpips_restate(S.image(names[p]), S.image(names[q]), aw, lin)[1] for p in range(3) for q in range(p + 1, 3)]))
    out["e2e/lpips"], out["e2e/lpips/gap"] = np.float64(res["mv_lpips"]), np.float64(abs(res["mv_lpips"] - np.mean(views)))
    print("e2e", res, "gap", out["e2e/lpips/gap"])
    return out


if __name__ == "__main__":
    main(sys.argv[1])
