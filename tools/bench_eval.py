#!/usr/bin/env python3
"""Per-stage times of the geometry evaluation (sin3dm_amd.evaluation) on one MI355X: procedural gyroid shapes at 128 x 104 x 88
(tests: sin3dm_amd.testing.gyroid_sdf), 16 generated shapes against one training shape, 1000 sampled patches of 11^3, stride 5.
Every stage ends in a device synchronise, so host work inside it (file reading, the shuffle, torch's compaction) is included;
median of the repeats after one warm-up run.  Next to the two counting stages, the same numbers from a dense torch formulation
on the same GPU: a float32 matmul of the flattened patches (volumes) gives the intersections, exactly, and the same float32
expression follows.  The two paths are compared bit for bit before they are timed, and timed alternately in one process.

    python tools/bench_eval.py [--shapes 16 --patch_num 1000 --repeats 5 --inner 50] > profiles/eval.txt
"""
import argparse
import os
import random
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from sin3dm_amd import _lib
from sin3dm_amd import evaluation as ev
from sin3dm_amd.testing import gyroid_sdf

ap = argparse.ArgumentParser()
ap.add_argument("--shape", type=int, nargs=3, default=(128, 104, 88))
ap.add_argument("--shapes", type=int, default=16)
ap.add_argument("--patch_size", type=int, default=11)
ap.add_argument("--stride", type=int, default=5)
ap.add_argument("--patch_num", type=int, default=1000)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--inner", type=int, default=50, help="back-to-back launches per timed window of the kernel / torch comparison")
args = ap.parse_args()

_lib.require_gpu()                                   # no GPU: fail, there is nothing to measure
PS, STRIDE, SHAPE = args.patch_size, args.stride, tuple(args.shape)
RESO = max(SHAPE)


def sync_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def unpack(words, n_bits):
    """int64 words [n][n_words] -> float32 [n][n_bits] of 0 / 1 (for the dense formulation)."""
    shifts = torch.arange(64, device=words.device, dtype=torch.int64)
    return ((words[:, :, None] >> shifts) & 1).reshape(words.shape[0], -1)[:, :n_bits].float()


def dense_lp_maxima(gen_bits, gen_counts, ref_bits, ref_counts):
    inter = gen_bits @ ref_bits.t()                                  # exact: 0 / 1 products, sums below 2^24
    ng, nr = gen_counts.float()[:, None], ref_counts.float()[None, :]
    iou = inter / (ng + nr - inter)
    p, r = inter / ng, inter / nr
    f = 2 * p * r / (p + r + 1e-8)
    return iou.max(dim=1).values, f.max(dim=1).values


def dense_div_counts(vols):
    flat = vols.reshape(vols.shape[0], -1).float()
    inter = flat @ flat.t()
    count = flat.sum(dim=1)
    return inter.long(), (count[:, None] + count[None, :] - inter).long()


with tempfile.TemporaryDirectory() as tmp:
    ref_path = os.path.join(tmp, "ref.npz")
    np.savez_compressed(ref_path, sdf_grid=gyroid_sdf(SHAPE, 3.0))
    paths = []
    for i in range(args.shapes):
        paths.append(os.path.join(tmp, f"s{i:02d}_voxel.npz"))
        np.savez_compressed(paths[-1], vox_grid=gyroid_sdf(SHAPE, 3.0, (0.05 + 0.04 * i, -0.03 * i, 0.02 * i)) < 0)

    def run():
        t = {}
        rng = random.Random(ev.patch_utils.SEED)
        t["load / pool"], (ref_vox, gens) = sync_ms(lambda: (ev.load_sdfgrid2vox(ref_path, RESO), [ev.load_voxgrid(p, RESO) for p in paths]))
        occ = [ref_vox.to(torch.uint8)] + [v.to(torch.uint8) for v in gens]
        t["validity + compaction"], idx = sync_ms(lambda: [torch.nonzero(ev.patch_validity(v, PS, STRIDE)).view(-1) for v in occ])
        chosen = [idx[0]] + [ix[torch.as_tensor(ev.shuffled_choice(rng, len(ix), args.patch_num), device=ix.device)] for ix in idx[1:]]
        t["packing"], packed = sync_ms(lambda: [ev.pack_patches(v, PS, STRIDE, ix, word_major=(k == 0)) for k, (v, ix) in enumerate(zip(occ, chosen))])
        pts = [ev.Patches(w, c, ix, PS, k == 0) for k, ((w, c), ix) in enumerate(zip(packed, chosen))]
        t["LP maxima"], maxima = sync_ms(lambda: [ev.lp_maxima(g, pts[0]) for g in pts[1:]])
        t["means and percents"], rows = sync_ms(lambda: [torch.stack([a.mean(), (a > 0.95).sum().float(), b.mean(), (b > 0.95).sum().float()]).tolist()
                                                         for a, b in maxima])
        t["Div (pack + pairwise counts + means)"], div = sync_ms(lambda: ev.pairwise_iou_dist(torch.stack(gens)))
        t["TOTAL"] = sum(t.values())
        return t, pts, maxima, gens, div, rows

    run()                                                # warm-up: allocations, code objects
    runs = [run() for _ in range(args.repeats)]
    _, pts, maxima, gens, div, rows = runs[-1]
    t_drivers, res = sync_ms(lambda: dict(ev.eval_lp(paths, ref_path, PS, STRIDE, args.patch_num, RESO), **ev.eval_div(paths, RESO)))

ref = pts[0]
n_bits = PS ** 3
print(f"geometry evaluation per stage, one MI355X: {args.shapes} generated shapes of {SHAPE[0]} x {SHAPE[1]} x {SHAPE[2]}, patch {PS}, stride {STRIDE}, "
      f"{len(ref)} reference patches, {len(pts[1])} sampled patches per shape ({ev.patch_utils.n_words(PS)} words each); "
      f"median of {args.repeats} runs after one warm-up [min .. max], ms for all {args.shapes} shapes")
for label in runs[0][0]:
    v = [r[0][label] for r in runs]
    print(f"  {label:40s} {statistics.median(v):9.3f}  [{min(v):.3f} .. {max(v):.3f}]")
print(f"  eval_lp + eval_div from the files, one call each: {t_drivers:.3f} ms -> {res}")

# ---- the counting kernels against the dense torch formulation: same inputs, same bits, alternating windows
gen = pts[1].to_layout(False)
ref_wm, ref_pm = ref.to_layout(True), ref.to_layout(False)
gen_bits, ref_bits = unpack(gen.words, n_bits), unpack(ref_pm.words, n_bits)
k_iou, k_f = ev.lp_maxima(gen, ref_wm)
d_iou, d_f = dense_lp_maxima(gen_bits, gen.counts, ref_bits, ref_pm.counts)
print(f"LP maxima, one shape ({len(gen)} x {len(ref)} pairs): kernel == dense torch bit for bit: iou {torch.equal(k_iou, d_iou)}, f {torch.equal(k_f, d_f)}"
      f" (differing: {int((k_iou != d_iou).sum())}, {int((k_f != d_f).sum())})")
vols = torch.stack(gens)
ki, ku = ev.pairwise_counts(vols)
di, du = dense_div_counts(vols)
print(f"pairwise counts ({vols.shape[0]} volumes): kernel == dense torch: inter {torch.equal(ki, di)}, union {torch.equal(ku, du)}")


def window(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(args.inner):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1e3 / args.inner


pairs = (("LP maxima", lambda: ev.lp_maxima(gen, ref_wm), lambda: dense_lp_maxima(gen_bits, gen.counts, ref_bits, ref_pm.counts)),
         ("LP maxima incl. unpacking for torch", lambda: ev.lp_maxima(gen, ref_wm),
          lambda: dense_lp_maxima(unpack(gen.words, n_bits), gen.counts, unpack(ref_pm.words, n_bits), ref_pm.counts)),
         ("pairwise counts incl. packing", lambda: ev.pairwise_counts(vols), lambda: dense_div_counts(vols)))
print(f"device-event time per call, us: {args.inner} back-to-back calls per window, {args.repeats} alternating windows each, median [min .. max]")
for label, kern, dense in pairs:
    kern(), dense()
    tk, td = [], []
    for _ in range(args.repeats):
        tk.append(window(kern))
        td.append(window(dense))
    mk, md = statistics.median(tk), statistics.median(td)
    print(f"  {label:38s} kernels {mk:9.1f} [{min(tk):.1f} .. {max(tk):.1f}]   dense torch {md:9.1f} [{min(td):.1f} .. {max(td):.1f}]   torch / kernels {md / mk:.2f}x")
