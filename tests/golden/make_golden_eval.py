"""Writes tests/golden/eval_geometry.npz from the reference's evaluation/patch_utils.py on the CPU:

    python tests/golden/make_golden_eval.py /path/to/reference

The volumes are procedural (tests/eval_cases.py); the fixture stores results only.  Per LP case `c`, reference `ref` and generated
shape `gen{i}`:
  c/{ref,gen{i}}/shape, /count      the loaded (pooled) occupancy's shape and number of occupied voxels
  c/{ref,gen{i}}/bits               pooled cases only: np.packbits of the loaded occupancy
  c/{ref,gen{i}}/valid              the valid candidates' positions in the row-major candidate grid, in order
  c/gen{i}/chosen                   positions in `valid` after the shuffle (random.seed(1234), one stream over the shapes)
  c/gen{i}/max_iou, /max_f          per chosen patch, float32: the reference's loop body, patch by patch
  c/gen{i}/lp                       [iou_avg, iou_percent, f_avg, f_percent] as eval_LP_IoU / eval_LP_Fscore return them
  c/result                          the four numbers of eval_LP_given_paths' dictionary (means over the shapes, round(6))
pool_up/{ref,gen}/shape, /bits: one volume pooled to a finer grid by both loaders; and for the diversity: div/counts, div/inter, div/union ([N][N]), div/result.
The reference returns patches, not their positions: the positions are restated here and the patches they select are checked
against the patches the reference returns.
"""
import os
import random
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))                     # tests/
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))    # the repository

import eval_cases as E  # noqa: E402


def valid_positions(vox, patch_size, stride):
    """Positions of the candidates whose centre cube is mixed, and all candidates as [n][ps][ps][ps]."""
    stride = patch_size // 2 if stride is None else stride
    p = patch_size // 2
    padded = np.pad(vox, p)
    win = np.lib.stride_tricks.sliding_window_view(padded, (patch_size,) * 3)[::stride, ::stride, ::stride]
    win = win.reshape(-1, patch_size, patch_size, patch_size)
    o, l = patch_size // 2 - 1, (2 if patch_size % 2 == 0 else 3)
    occ = win[:, o:o + l, o:o + l, o:o + l].reshape(len(win), -1).sum(axis=1)
    return np.nonzero((occ > 0) & (occ < l ** 3))[0], win


def main(ref_root):
    sys.path.insert(0, os.path.join(ref_root, "evaluation"))
    import patch_utils as P
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for case, (ref_name, gens, ps, stride, patch_num, reso) in E.LP_CASES.items():
            ref_path = os.path.join(tmp, "ref.npz")
            np.savez(ref_path, sdf_grid=E.sdf(ref_name))
            ref_vox = P.load_sdfgrid2vox(ref_path, resolution=reso)
            pooled = tuple(ref_vox.shape) != E.VOLUMES[ref_name][0]

            def record(tag, vox):
                v = vox.numpy()
                out[f"{case}/{tag}/shape"] = np.asarray(v.shape, dtype=np.int32)
                out[f"{case}/{tag}/count"] = np.int64(v.sum())
                if pooled:
                    out[f"{case}/{tag}/bits"] = np.packbits(v.reshape(-1))
                pos, win = valid_positions(v, ps, stride)
                patches = P.extract_valid_patches_unfold(vox, ps, stride)
                assert np.array_equal(win[pos], patches.numpy()), (case, tag)
                out[f"{case}/{tag}/valid"] = pos.astype(np.int32)
                return patches

            ref_patches = record("ref", ref_vox)
            random.seed(1234)
            rows = []
            for i, g in enumerate(gens):
                path = os.path.join(tmp, "gen.npz")
                np.savez(path, vox_grid=E.generated_occupancy(g, ref_name))
                gen_vox = P.load_voxgrid(path, resolution=reso)
                assert gen_vox.shape == ref_vox.shape
                gen_patches = record(f"gen{i}", gen_vox)
                indices = list(range(gen_patches.shape[0]))
                random.shuffle(indices)
                indices = indices[:patch_num]
                gen_patches = gen_patches[indices]
                out[f"{case}/gen{i}/chosen"] = np.asarray(indices, dtype=np.int32)
                max_iou, max_f = [], []
                ref_sum = ref_patches.sum(dim=(1, 2, 3))
                for k in range(gen_patches.shape[0]):
                    one = gen_patches[k:k + 1]
                    inter = torch.logical_and(ref_patches, one).sum(dim=(1, 2, 3))
                    union = torch.logical_or(ref_patches, one).sum(dim=(1, 2, 3))
                    max_iou.append(torch.max(inter / union))
                    precision, recall = inter / one.sum(), inter / ref_sum
                    max_f.append(torch.max(2 * precision * recall / (precision + recall + 1e-8)))
                max_iou, max_f = torch.stack(max_iou), torch.stack(max_f)
                assert max_iou.dtype == torch.float32 and max_f.dtype == torch.float32
                iou_avg, iou_percent = P.eval_LP_IoU(gen_patches, ref_patches)
                f_avg, f_percent = P.eval_LP_Fscore(gen_patches, ref_patches)
                assert iou_avg == torch.mean(max_iou).item() and f_avg == torch.mean(max_f).item()
                assert iou_percent == (max_iou > 0.95).sum().item() / len(max_iou) and f_percent == (max_f > 0.95).sum().item() / len(max_f)
                out[f"{case}/gen{i}/max_iou"] = max_iou.numpy()
                out[f"{case}/gen{i}/max_f"] = max_f.numpy()
                out[f"{case}/gen{i}/lp"] = np.asarray([iou_avg, iou_percent, f_avg, f_percent], dtype=np.float64)
                rows.append((iou_avg, iou_percent, f_avg, f_percent))
                print(case, g, "ref", ref_patches.shape[0], "gen", len(indices), "lp", rows[-1])
            out[f"{case}/result"] = np.asarray([np.mean(c).round(6) for c in zip(*rows)], dtype=np.float64)

        # the issue's requirements on the cases: a percent strictly inside (0, 1) for both metrics, and an identical shape at exactly 1
        lp = out["p11_32/gen0/lp"]
        assert 0 < lp[1] < 1 and 0 < lp[3] < 1, lp
        assert np.all(out["p11_32/gen1/max_iou"] == 1) and np.all(out["p11_32/gen1/max_f"] == 1) and np.all(out["p11_32/gen1/lp"] == 1)

        # pooling to a finer grid (windows of one or two voxels): (32, 26, 20) -> (40, 32, 25), both loaders
        up = os.path.join(tmp, "up.npz")
        np.savez(up, sdf_grid=E.sdf(E.POOL_UP[0]), vox_grid=E.generated_occupancy(E.POOL_UP[0]))
        for tag, vox in (("ref", P.load_sdfgrid2vox(up, resolution=E.POOL_UP[1])), ("gen", P.load_voxgrid(up, resolution=E.POOL_UP[1]))):
            out[f"pool_up/{tag}/shape"] = np.asarray(vox.shape, dtype=np.int32)
            out[f"pool_up/{tag}/bits"] = np.packbits(vox.numpy().reshape(-1))

        paths = []
        for i, name in enumerate(E.DIV_CASE):
            paths.append(os.path.join(tmp, f"div{i}.npz"))
            np.savez(paths[-1], vox_grid=E.generated_occupancy(name))
        vols = torch.stack([P.load_voxgrid(p, resolution=E.DIV_RESOLUTION) for p in paths])
        flat = vols.reshape(len(paths), -1).numpy()
        out["div/counts"] = flat.sum(axis=1).astype(np.int64)
        out["div/inter"] = (flat[:, None] & flat[None]).sum(axis=2).astype(np.int64)
        out["div/union"] = (flat[:, None] | flat[None]).sum(axis=2).astype(np.int64)
        out["div/value"] = np.float64(P.pairwise_IoU_dist(vols))
        old = P.load_voxgrid                  # eval_Div_given_paths fixes resolution=128: run it at the case's resolution
        P.load_voxgrid = lambda path, resolution=128, device="cpu": old(path, resolution=E.DIV_RESOLUTION, device=device)
        try:
            out["div/result"] = np.float64(P.eval_Div_given_paths(paths)["Div"])
        finally:
            P.load_voxgrid = old
        print("div", out["div/value"], out["div/result"])

    # the procedural volumes themselves: what tests/test_eval_host.py regenerates
    for name in E.VOLUMES:
        out[f"volumes/{name}"] = np.asarray([E.reference_occupancy(name).sum(), (E.sdf(name) < 0).sum()], dtype=np.int64)
    path = os.path.join(HERE, "eval_geometry.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
