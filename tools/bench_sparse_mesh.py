#!/usr/bin/env python3
"""The narrow-band iso-surface extraction (isosurface.marching_cubes_sparse) beside the dense path on one MI355X, in
one process, by device events.

  fields      "torus": an analytic torus as a torch expression (the field costs almost nothing: this row is the extraction itself);
              "decoder": the skip net with texture at full width (up 64, hidden 256) with synthetic weights on a 128^3 triplane
              (same arithmetic as a trained one, but a rougher field: more surface per volume than a trained shape has)
  256^3 and 512x512x256   dense (decode_grid + marching_cubes, or the expression on the whole grid) against sparse, the two
              alternating round by round after a warm-up round; medians and the spread (min .. max)
  1024^3 and 2048^3       sparse alone: the dense path refuses 3 (N + 2)^3 >= 2^31 edges, so there is no dense time to compare
              against at these sizes, and none is extrapolated
  per stage   the lattice, the band decode per round, the boundary pass per round (grow), count (flags twice + the two key sorts),
              extract (vertices, triangles), occupancy; n_samples / N^3, the rounds, the peak device memory of the call
A field the band cannot hold (S3D_MCS_MAX_SAMPLES) is reported as refused, not skipped silently.

    python tools/bench_sparse_mesh.py [--repeats 3] [--block 8] > profiles/sparse_mesh.txt
"""
import argparse
import os
import statistics
import sys
import tempfile
from types import SimpleNamespace

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO]
import numpy as np
import torch

from sin3dm_amd import _lib, testing as T
from sin3dm_amd.encoding import isosurface as iso
from sin3dm_amd.encoding.model import ShapeAutoEncoder

ap = argparse.ArgumentParser()
ap.add_argument("--fm", type=int, default=128, help="feature-map side of the decoder's triplane (H = W = D)")
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--block", type=int, default=8)
ap.add_argument("--large_block", type=int, default=16, help="brick size of the 1024^3 / 2048^3 rows")
ap.add_argument("--skip_2048", action="store_true")
args = ap.parse_args()

_lib.require_gpu()                                   # no GPU: fail, there is nothing to measure
dev = torch.device("cuda:0")


def med(xs):
    return f"{statistics.median(xs):9.2f} ms ({min(xs):.2f} .. {max(xs):.2f})"


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


# ------------------------------------------------------------------ the two fields
def torus_field(dims):
    c = [(d - 1) / 2.0 for d in dims]
    s = float(min(dims))

    def sdf(p):
        q = torch.sqrt((p[:, 0] - c[0]) ** 2 + (p[:, 1] - c[1]) ** 2) - 0.30 * s
        return (torch.sqrt(q * q + (p[:, 2] - c[2]) ** 2) - 0.10 * s)[:, None]

    def dense():
        ax = [torch.arange(d, dtype=torch.float32, device=dev) for d in dims]
        q = torch.sqrt((ax[0][:, None, None] - c[0]) ** 2 + (ax[1][None, :, None] - c[1]) ** 2) - 0.30 * s
        return torch.sqrt(q * q + (ax[2][None, None, :] - c[2]) ** 2) - 0.10 * s
    return sdf, dense, 0


cfg = SimpleNamespace(enc_net_type="skip", fdim_geo=4, fdim_tex=8, fdim_up=64, hidden_dim=256, n_hidden_layers=4, data_type="sdftex", gpu_id=0)
ae = ShapeAutoEncoder(tempfile.mkdtemp(prefix="sparse_mesh_"), cfg, device=dev)
ae.net.load_state_dict(T.synthetic_state_dict(T.ae_param_shapes(), 5), strict=False)
ae.net.to(dev).eval()
FM = [torch.from_numpy(np.tanh(T.synthetic_noise((1, 12, args.fm, args.fm), s))).to(dev) for s in (1, 2, 3)]


def decoder_field(dims):
    big = max(dims)
    aabb = torch.tensor([-d / big for d in dims] + [d / big for d in dims], device=dev)
    ae.aabb = aabb
    ae.net.reset_aabb(aabb)
    ae.featmap_size = (args.fm,) * 3
    fn, got = ae.index_sampler(FM, aabb, big)
    assert tuple(got) == tuple(dims), (got, dims)
    return fn, (lambda: ae.decode_grid(FM, big, aabb=aabb)), 3


FIELDS = {"torus": torus_field, "decoder": decoder_field}


def sparse_run(fn, dims, n_attr, block, occupancy=True):
    stages = []
    torch.cuda.reset_peak_memory_stats()
    ms, out = event_ms(lambda: iso.marching_cubes_sparse(fn, dims, n_attr=n_attr, block=block, return_info=True, occupancy=occupancy, stages=stages))
    return ms, out, stages, torch.cuda.max_memory_allocated()


def dense_run(dense, n_attr):
    torch.cuda.reset_peak_memory_stats()

    def run():
        g = dense()
        occ = (g[..., 0] if g.dim() == 4 else g) < 0
        return iso.marching_cubes(g, 0.0, 1.0, n_attr=n_attr), occ
    ms, out = event_ms(run)
    return ms, out, torch.cuda.max_memory_allocated()


def report_stages(all_stages):
    names = [n for n, _ in all_stages[0]]
    for i, n in enumerate(names):
        print(f"      {n:12s} {med([s[i][1] for s in all_stages if len(s) == len(names)])}")


print(f"# narrow-band iso-surface extraction: {torch.cuda.get_device_name(0)}, brick {args.block} (large sizes {args.large_block}), "
      f"{args.repeats} timed rounds after one warm-up, dense and sparse alternating")
for dims in ((256, 256, 256), (512, 512, 256)):
    for name, make in FIELDS.items():
        fn, dense, n_attr = make(dims)
        d_ms, s_ms, s_stages = [], [], []
        for rnd in range(args.repeats + 1):
            dm, (dmesh, docc), dmem = dense_run(dense, n_attr)
            sm, smesh, stages, smem = sparse_run(fn, dims, n_attr, args.block)
            if rnd:
                d_ms.append(dm); s_ms.append(sm); s_stages.append(stages)
        info = smesh[3]
        N = dims[0] * dims[1] * dims[2]
        same = smesh[0].shape == dmesh[0].shape and torch.equal(smesh[0], dmesh[0]) and torch.equal(smesh[1], dmesh[1])
        same_l = all(torch.equal(a, b) for a, b in zip(iso.largest_component(*smesh[:2])[:2], iso.largest_component(*dmesh[:2])[:2]))
        print(f"\n{name} {dims[0]}x{dims[1]}x{dims[2]}: {dmesh[1].shape[0]} triangles dense, {smesh[1].shape[0]} sparse (whole mesh identical: {same}; "
              f"largest component identical: {same_l}; occupancy identical: {torch.equal(info['occupancy'].bool(), docc)})")
        print(f"    dense   {med(d_ms)}   peak memory {dmem / 2 ** 30:.2f} GiB   {N} evaluations")
        print(f"    sparse  {med(s_ms)}   peak memory {smem / 2 ** 30:.2f} GiB   {info['n_samples']} evaluations = {info['n_samples'] / N:.4f} N^3, "
              f"{info['n_active']} of {info['n_bricks']} bricks ({info['n_seed']} seeds), {info['rounds']} rounds, closed {info['closed']}")
        print(f"    dense / sparse (medians) {statistics.median(d_ms) / statistics.median(s_ms):.2f}")
        report_stages(s_stages)
        del dmesh, docc, smesh, info
        torch.cuda.empty_cache()

for n in (1024,) + (() if args.skip_2048 else (2048,)):
    dims = (n, n, n)
    for name, make in FIELDS.items():
        fn, _, n_attr = make(dims)
        try:
            sparse_run(fn, dims, n_attr, args.large_block, occupancy=n <= 1024)          # warm-up
            ms, smesh, stages, smem = sparse_run(fn, dims, n_attr, args.large_block, occupancy=n <= 1024)
        except (NotImplementedError, torch.OutOfMemoryError) as e:
            print(f"\n{name} {n}^3 (sparse alone, brick {args.large_block}): refused: {str(e)[:200]}")
            torch.cuda.empty_cache()
            continue
        info = smesh[3]
        print(f"\n{name} {n}^3 (sparse alone, brick {args.large_block}; the dense path refuses this size, so there is no dense time): "
              f"{smesh[1].shape[0]} triangles")
        print(f"    sparse  {ms:9.2f} ms (one timed run)   peak memory {smem / 2 ** 30:.2f} GiB   {info['n_samples']} evaluations = "
              f"{info['n_samples'] / n ** 3:.4f} N^3, {info['n_active']} of {info['n_bricks']} bricks ({info['n_seed']} seeds), {info['rounds']} rounds, "
              f"closed {info['closed']}" + ("" if n <= 1024 else "   (occupancy not written at this size: 8 GiB of uint8)"))
        report_stages([stages])
        del smesh, info
        torch.cuda.empty_cache()
