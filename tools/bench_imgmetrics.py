"""SIFID and LPIPS per stage on one MI355X (s3d_imgfeat.hip), next to PyTorch-ROCm eager on the same GPU:

    python tools/bench_imgmetrics.py [--size 512] [--generated 16] [--views 8] [--runs 5] [--out profiles/imgmetrics.txt]

Per view: SIFID takes the 16 generated renders and the reference render in one batch of 17 per dims, LPIPS the 16 generated ones
and all 120 pairs.  Stage times are device events inside the library (s3d_imgfeat_profile) and torch events around the
statistics and pair calls; medians over the runs after one warm-up, the two implementations alternating in one process.
The eager comparator runs the same layers with F.conv2d / F.batch_norm / F.max_pool2d in float32, torch.cov in float64, and
the LPIPS features once per image and its head per image against all later ones.  Weights and images are procedural.
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import imgmetrics_cases as S  # noqa: E402
from sin3dm_amd import _lib  # noqa: E402
from sin3dm_amd.evaluation import lpips as L, sifid as SF  # noqa: E402

PEAK_TF, DECODER_TF = 155.0, 121.0       # measured float32-MFMA peak and the decoder's rate on it


def images(n, size, seed):
    rng = np.random.Generator(np.random.PCG64([seed, 0xBE7C]))
    base = rng.integers(0, 256, size=(n, size // 8, size // 8, 4), dtype=np.uint8)
    img = np.repeat(np.repeat(base, 8, axis=1), 8, axis=2)
    return torch.from_numpy(np.ascontiguousarray((img.astype(np.int32) + rng.integers(-8, 9, size=img.shape)).clip(0, 255).astype(np.uint8))).cuda()


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def eager_stem(x_u8, w, dims):
    x = 2 * (x_u8[..., :3].permute(0, 3, 1, 2).float() / 255) - 1
    for name, _, _, _, stride, pad, pool in S.STEM[:3 if dims == 64 else 5]:
        if pool:
            x = F.max_pool2d(x, 3, 2)
        x = F.conv2d(x, w[name + ".conv.weight"], stride=stride, padding=pad)
        x = F.relu(F.batch_norm(x, w[name + ".bn.running_mean"], w[name + ".bn.running_var"], w[name + ".bn.weight"], w[name + ".bn.bias"], False, 0.0, 1e-3))
    rows = x.permute(0, 2, 3, 1).reshape(x.shape[0], -1, x.shape[1]).double()
    return rows.mean(dim=1), torch.stack([torch.cov(r.T) for r in rows])


def eager_lpips(x_u8, w, lin, mu, sigma):
    x = ((x_u8[..., :3].permute(0, 3, 1, 2).double() / 255. - 0.5) / 0.5).float()
    x = (x - mu) / sigma
    maps = []
    for name, _, _, _, stride, pad, pool in S.ALEX:
        if pool:
            x = F.max_pool2d(x, 3, 2)
        x = F.relu(F.conv2d(x, w[name + ".weight"], w[name + ".bias"], stride=stride, padding=pad))
        maps.append(x * torch.rsqrt(torch.sum(x ** 2, dim=1, keepdim=True) + 1e-10))
    n = x.shape[0]
    out = torch.zeros((n, n), device=x.device)
    for i in range(n - 1):                # features once per image (the reference recomputes them per pair), the head per pair
        for l, m in enumerate(maps):
            out[i, i + 1:] += torch.mean(F.conv2d((m[i:i + 1] - m[i + 1:]) ** 2, lin[l]), dim=(1, 2, 3))
    return out


def flops(units, H, W, n):
    out, e = [], [H, W]
    for _, cin, cout, k, stride, pad, pool in units:
        if pool:
            e = [(v - 3) // 2 + 1 for v in e]
        e = [(v + 2 * pad - k) // stride + 1 for v in e]
        out.append(2.0 * n * e[0] * e[1] * cout * cin * k * k)
    return out


def med(v):
    return f"{statistics.median(v):9.3f}  [{min(v):.3f} .. {max(v):.3f}]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--generated", type=int, default=16)
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    dev = torch.device("cuda")
    n, size = a.generated, a.size
    wi = {k: v.to(dev) for k, v in S.inception_weights().items()}
    wa = {k: v.to(dev) for k, v in S.alexnet_weights().items()}
    lin = [v.to(dev) for v in S.lpips_linear().values()]
    mu, sigma = torch.tensor(S.LPIPS_MU, device=dev).view(1, 3, 1, 1), torch.tensor(S.LPIPS_SIGMA, device=dev).view(1, 3, 1, 1)
    stem, alex = SF.InceptionStem(S.inception_weights()), L.AlexNetLpips(S.alexnet_weights(), S.lpips_linear())
    stem.profile(True)
    alex.profile(True)
    batch = images(n + 1, size, 1)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    lines = [f"SIFID and LPIPS per stage, one MI355X ({cus} CUs): per view {n} generated renders + the reference render of {size} x {size}; "
             f"median of {a.runs} runs after one warm-up [min .. max], ms per VIEW (x {a.views} views for an evaluation)"]

    # agreement of the two implementations on this input
    m64, s64 = stem.statistics_device(batch[:2], 64)
    em, es = eager_stem(batch[:2], wi, 64)
    lp = alex.pair_matrix_device(batch[:3])
    le = eager_lpips(batch[:3], wa, lin, mu, sigma)
    lines.append(f"  kernels vs eager torch: dims 64 mu {float((m64 - em).abs().max()):.2e}, sigma {float((s64 - es).abs().max()):.2e}; "
                 f"LPIPS {float((lp - le.double()).abs()[0, 1:].max()):.2e} on {float(lp[0, 1]):.4f}")

    res = {}
    for run in range(a.runs + 1):
        cur = {}
        for dims in (64, 192):
            t_feat, _ = timed(lambda: stem._features(batch, dims, False))
            cur[f"sifid{dims} units"] = stem.stage_ms()[:5]
            mu_d = torch.empty((n + 1, dims), dtype=torch.float64, device=dev)
            sg_d = torch.empty((n + 1, dims, dims), dtype=torch.float64, device=dev)
            cur[f"sifid{dims} statistics"], _ = timed(lambda: _lib.check(stem._lib.s3d_imgfeat_stats(stem._h, _lib.ptr(mu_d), _lib.ptr(sg_d), _lib.stream_ptr())))
            cur[f"sifid{dims} all"] = t_feat + cur[f"sifid{dims} statistics"]
            cur[f"sifid{dims} eager"], _ = timed(lambda: eager_stem(batch, wi, dims))
        t_feat, _ = timed(lambda: alex._features(batch[:n], 0, False))
        ms = alex.stage_ms()
        cur["lpips units"], cur["lpips normalise"] = ms[:5], ms[5]
        total = torch.empty((n, n), dtype=torch.float64, device=dev)
        cur["lpips pairs"], _ = timed(lambda: _lib.check(alex._lib.s3d_imgfeat_pairs(alex._h, None, _lib.ptr(total), _lib.stream_ptr())))
        cur["lpips all"] = t_feat + cur["lpips pairs"]
        cur["lpips eager"], _ = timed(lambda: eager_lpips(batch[:n], wa, lin, mu, sigma))
        if run:
            for k, v in cur.items():
                res.setdefault(k, []).append(v)

    def unit_lines(tag, key, units, count):
        fl = flops(units, size, size, count)
        for l, (name, cin, cout, k, stride, pad, pool) in enumerate(units):
            v = [r[l] for r in res[key]]
            t = statistics.median(v)
            e = [size, size]
            for u in units[:l + 1]:
                if u[6]:
                    e = [(x - 3) // 2 + 1 for x in e]
                e = [(x + 2 * u[5] - u[3]) // u[4] + 1 for x in e]
            blocks = count * ((e[0] * e[1] + 127) // 128) * ((cout + 63) // 64)
            lines.append(f"  {tag} {name:<14} {cin:>3}->{cout:<3} k{k} s{stride}{' pool+' if pool else '      '} {med(v)}   {fl[l] / 1e9:7.2f} GFLOP "
                         f"{fl[l] / t / 1e9:6.1f} TFLOP/s ({100 * fl[l] / t / 1e9 / PEAK_TF:4.1f} % of {PEAK_TF:.0f}; decoder {DECODER_TF:.0f})   "
                         f"{blocks} blocks = {blocks / (2.0 * cus):.1f} rounds of 2 per CU")

    for dims in (64, 192):
        unit_lines(f"sifid{dims}", f"sifid{dims} units", S.STEM[:3 if dims == 64 else 5], n + 1)
        lines.append(f"  sifid{dims} statistics (Gram + covariance, {n + 1} images)   {med(res[f'sifid{dims} statistics'])}")
        k, e = statistics.median(res[f"sifid{dims} all"]), statistics.median(res[f"sifid{dims} eager"])
        lines.append(f"  sifid{dims} features + statistics                      {med(res[f'sifid{dims} all'])}")
        lines.append(f"  sifid{dims} eager torch (conv2d, batch_norm, cov f64)  {med(res[f'sifid{dims} eager'])}     torch / kernels {e / k:.2f}x")
    unit_lines("lpips", "lpips units", S.ALEX, n)
    lines.append(f"  lpips unit normalisation (5 maps, {n} images)           {med(res['lpips normalise'])}")
    lines.append(f"  lpips pairs ({n * n} ordered pairs, 5 launches + 1)       {med(res['lpips pairs'])}")
    k, e = statistics.median(res["lpips all"]), statistics.median(res["lpips eager"])
    lines.append(f"  lpips features + pairs                                {med(res['lpips all'])}")
    lines.append(f"  lpips eager torch (features once per image)           {med(res['lpips eager'])}     torch / kernels {e / k:.2f}x")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
