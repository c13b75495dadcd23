"""Writes tests/golden/ssfid.npz from the reference's evaluation/ssfid.py and evaluation/classifier3D.py on the CPU:

    python tests/golden/make_golden_ssfid.py /path/to/reference

Weights and volumes are procedural (tests/ssfid_cases.py); the fixture stores results only.  Per volume `v` and layer `L`:
  v/L/mu, v/L/sigma                       calculate_activation_statistics of the float32 classifier (mu float32, sigma float64)
  v/L/gap_act, /gap_mu, /gap_sigma        the reference's own float32-versus-float64 gap on this input: the largest absolute
                                          difference to the same module run in .double()
per pair `p` of ssfid_cases.PAIRS and layer:
  p/L/fd                                  calculate_frechet_distance (scipy sqrtm) of the float32 statistics
  p/L/fd_gap                              |that - the same function of the .double() statistics|
  p/L/fd_sym_gap                          |symmetric eigh form - sqrtm form| / |sqrtm form| on the float32 statistics
act/L                                     the float32 activations of ssfid_cases.ACT_CASE, rows in [X'][Y'][Z'] order
e2e/L                                     [SSFID_avg, SSFID_std] of eval_SSFID_given_paths over the two generated shapes of
                                          ssfid_cases.E2E_CASE, the loaders' resolution patched to ssfid_cases.E2E_RESOLUTION
e2e/L/gap                                 the largest per-shape |float32 - float64| distance gap of that run
The classifier's other layers keep their default initialisation: the procedural weights are loaded with strict=False and the
whole state dict is written as Clsshapenet_128.pth into a temporary working directory for the end-to-end run.
"""
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))                     # tests/
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))    # the repository

import eval_cases as E  # noqa: E402
import ssfid_cases as S  # noqa: E402


def main(ref_root):
    sys.path.insert(0, os.path.join(ref_root, "evaluation"))
    import ssfid as R
    from classifier3D import classifier
    from sin3dm_amd.evaluation.ssfid import frechet_distance

    torch.manual_seed(0)
    model = classifier()
    missing = model.load_state_dict(S.weights(), strict=False)
    assert not missing.unexpected_keys and not any(k.startswith(("conv_1", "conv_2.")) for k in missing.missing_keys), missing
    model.eval()
    model64 = classifier().double()
    model64.load_state_dict({k: v.double() for k, v in model.state_dict().items()})
    model64.eval()

    def stats(m, vox, layer):
        with torch.no_grad():
            act = m(vox[None, None], out_layer=layer)
        act = act.permute(0, 2, 3, 4, 1).reshape(-1, act.shape[1]).numpy()
        mu, sigma = R.calculate_activation_statistics(vox, m, layer)
        assert np.array_equal(mu, np.mean(act, axis=0)) and np.array_equal(sigma, np.cov(act, rowvar=False))
        return act, mu, sigma

    out, both = {}, {}
    worst = {}
    for name in S.volume_names():
        vox = torch.from_numpy(S.volume(name))
        for layer in S.LAYERS:
            a32, m32, s32 = stats(model, vox.float(), layer)
            a64, m64, s64 = stats(model64, vox.double(), layer)
            assert a32.dtype == np.float32 and a64.dtype == np.float64
            _, mu_r, sigma_r = S.restated(name, layer)                 # the restatement is the .double() module to round-off
            assert np.max(np.abs(m64 - mu_r)) < 1e-12 and np.max(np.abs(s64 - sigma_r)) < 1e-12, (name, layer)
            key = f"{name}/{layer}"
            out[f"{key}/mu"], out[f"{key}/sigma"] = m32, s32
            gaps = dict(act=np.max(np.abs(a32 - a64)), mu=np.max(np.abs(m32 - m64)), sigma=np.max(np.abs(s32 - s64)))
            for k, v in gaps.items():
                out[f"{key}/gap_{k}"] = np.float64(v)
                worst[(layer, k)] = max(worst.get((layer, k), 0.0), float(v))
            both[(name, layer)] = ((m32, s32), (m64, s64))
            if name == S.ACT_CASE:
                out[f"act/{layer}"] = a32
            print(key, "rows", a32.shape[0], "max|act|", float(np.max(np.abs(a64))), "max|sigma|", float(np.max(np.abs(s64))),
                  {k: float(v) for k, v in gaps.items()})
    worst_sym = 0.0
    for pair, (r, g) in S.PAIRS.items():
        for layer in S.LAYERS:
            (r32, r64), (g32, g64) = both[(r, layer)], both[(g, layer)]
            fd32 = float(R.calculate_frechet_distance(*r32, *g32))
            fd64 = float(R.calculate_frechet_distance(*r64, *g64))
            sym = frechet_distance(*r32, *g32)
            out[f"{pair}/{layer}/fd"] = np.float64(fd32)
            out[f"{pair}/{layer}/fd_gap"] = np.float64(abs(fd32 - fd64))
            out[f"{pair}/{layer}/fd_sym_gap"] = np.float64(abs(sym - fd32) / abs(fd32))
            if pair != "prank":
                worst_sym = max(worst_sym, abs(sym - fd32) / abs(fd32))
            print(pair, layer, "fd", fd32, "f32-f64 gap", abs(fd32 - fd64), "sym gap (rel)", abs(sym - fd32) / abs(fd32),
                  "same", frechet_distance(*r32, *r32))
    print("worst gaps", worst, "worst symmetric-form gap (full-rank pairs)", worst_sym)

    # end to end: eval_SSFID_given_paths reads Clsshapenet_128.pth from the working directory and loads at resolution 128
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        torch.save(model.state_dict(), os.path.join(tmp, "Clsshapenet_128.pth"))
        paths, ref_path = E.write_case_files(S.E2E_CASE, tmp)
        old = R.load_voxgrid, R.load_sdfgrid2vox
        R.load_voxgrid = lambda path, resolution=128, device="cpu": old[0](path, resolution=S.E2E_RESOLUTION, device=device)
        R.load_sdfgrid2vox = lambda path, resolution=128, device="cpu": old[1](path, resolution=S.E2E_RESOLUTION, device=device)
        os.chdir(tmp)
        try:
            for layer in S.LAYERS:
                res = R.eval_SSFID_given_paths(paths, ref_path, model_out_layer=layer)
                out[f"e2e/{layer}"] = np.asarray([res["SSFID_avg"], res["SSFID_std"]], dtype=np.float64)
                ref = R.load_sdfgrid2vox(ref_path)
                gap = 0.0
                for p in paths:
                    gen = R.load_voxgrid(p)
                    d32 = R.calculate_frechet_distance(*R.calculate_activation_statistics(ref.float(), model, layer),
                                                       *R.calculate_activation_statistics(gen.float(), model, layer))
                    d64 = R.calculate_frechet_distance(*R.calculate_activation_statistics(ref.double(), model64, layer),
                                                       *R.calculate_activation_statistics(gen.double(), model64, layer))
                    gap = max(gap, abs(float(d32) - float(d64)))
                out[f"e2e/{layer}/gap"] = np.float64(gap)
                print("e2e", layer, res, "gap", gap)
        finally:
            os.chdir(cwd)
            R.load_voxgrid, R.load_sdfgrid2vox = old

    path = os.path.join(HERE, "ssfid.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
