#!/usr/bin/env python3
"""What seed-level parity costs: the headline workload (BASELINE configs[1]: 128-ch UNet, 128^3 triplane, batch 1, DDPM) with
three noise sources, interleaved in one process and timed with device events:

  (a) device   the default: the device's Philox generator, drawn in chunks of steps
  (b) stream   generator=TorchCpuStream(k): torch's CPU stream generated on the device (s3d_rng.hip)
  (c) host     the host recipe  noise_fn = lambda x: th.randn(x.shape).to(x.device)

plus the two kernels alone: the state walker (one workgroup) and the transform, per step's worth of noise.

    python tools/bench_cpu_stream.py [--steps 200] [--rounds 3] > profiles/cpu_stream.txt
"""
import argparse
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--kernels-only", action="store_true", help="only the walker / transform timings")
    args = ap.parse_args()

    import ctypes as C
    import torch
    from sin3dm_amd import _lib, testing as T
    from sin3dm_amd.diffusion.cpu_stream import TorchCpuStream, words_per_call
    from sin3dm_amd.diffusion.script_util import create_gaussian_diffusion
    from sin3dm_amd.diffusion.unet_triplane import TriplaneUNetModelSmall

    _lib.require_gpu()
    dev = torch.device("cuda:0")
    H = W = D = 128
    mc = 128
    model = TriplaneUNetModelSmall(12, mc, 12, num_res_blocks=1, channel_mult=(1, 2), use_scale_shift_norm=True)
    model.load_state_dict(T.synthetic_state_dict(T.unet_param_shapes(model_channels=mc), 0))
    model.to(dev).eval()
    kw = dict(H=H, W=W, D=D)
    shape = (1, 12, H + D, W + D)
    numel = 12 * (H + D) * (W + D)

    def run(kind, steps, overlap=True):
        """ms per step of `steps` steps of p_sample_loop_progressive (the first step, which holds the set-up, is left out)"""
        diff = create_gaussian_diffusion(steps=1000, predict_xstart=True)
        diff._CPU_STREAM_OVERLAP = overlap
        gen = None
        if kind == "stream":
            gen = TorchCpuStream(1000)
        elif kind == "host":
            torch.manual_seed(1000)
            diff.noise_fn = lambda x: torch.randn(x.shape).to(x.device)
        else:
            gen = torch.Generator(device=dev).manual_seed(1000)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        it = diff.p_sample_loop_progressive(model, shape, model_kwargs=kw, generator=gen)
        for n, _ in enumerate(it):
            if n == 0:
                e0.record()
            if n == steps:
                e1.record()
                break
        it.close()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / steps

    print(f"# tools/bench_cpu_stream.py --steps {args.steps} --rounds {args.rounds}: {torch.cuda.get_device_name(0)}, torch {torch.__version__}, "
          f"host threads {torch.get_num_threads()}")
    print(f"# workload: {mc}-ch UNet, {H}^3 triplane, batch 1, DDPM-1000 schedule, {args.steps} steps per leg; {numel} noise elements per step")
    if not args.kernels_only:
        legs_report(args, run)
    kernels_report(torch, C, _lib, TorchCpuStream, words_per_call, dev, shape, numel)


def legs_report(args, run):
    for kind in ("device", "stream", "host"):
        run(kind, args.warmup)
    legs = {"device": [], "stream": [], "stream_inline": [], "host": []}
    for r in range(args.rounds):
        for kind in legs:
            ms = run("stream" if kind.startswith("stream") else kind, args.steps, overlap=kind != "stream_inline")
            legs[kind].append(ms)
            print(f"round {r} {kind:14s} {ms * 1000:9.1f} us/step")
    med = {k: statistics.median(v) for k, v in legs.items()}
    print()
    print(f"(a) device generator            median {med['device'] * 1000:8.1f} us/step   spread {(max(legs['device']) - min(legs['device'])) * 1000:.1f} us")
    print(f"(b) TorchCpuStream (side stream) median {med['stream'] * 1000:8.1f} us/step   = (a) x {med['stream'] / med['device']:.3f}")
    print(f"(b') TorchCpuStream (in line)    median {med['stream_inline'] * 1000:8.1f} us/step   = (a) x {med['stream_inline'] / med['device']:.3f}")
    print(f"(c) host randn + upload          median {med['host'] * 1000:8.1f} us/step   = (a) x {med['host'] / med['device']:.3f}   (b) is {med['host'] / med['stream']:.2f}x faster")


def kernels_report(torch, C, _lib, TorchCpuStream, words_per_call, dev, shape, numel):
    """the two kernels alone, on one step's worth of noise (k calls in one launch pair, so the launch overhead is spread)"""
    lib = _lib.load()
    s = TorchCpuStream(1, device=dev)
    k = 16
    s.randn(shape, lead=k)                       # warm: handle, workspace
    out = torch.empty((k,) + shape, device=dev)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def timed(fn, reps=5):
        ts = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
        return statistics.median(ts)
    both = timed(lambda: _lib.check(lib.s3d_rng_randn(s._handle, _lib.ptr(out), numel, k, st)))
    # rand of the same word count runs the same walk followed by the (cheaper) uniform transform: the walk dominates it
    words = words_per_call(numel) * k
    flat = torch.empty(words, device=dev)
    walk_u = timed(lambda: _lib.check(lib.s3d_rng_rand(s._handle, _lib.ptr(flat), words, st)))
    philox = timed(lambda: torch.randn((k,) + shape, device=dev))
    flat2 = torch.empty_like(flat)
    stream_op = timed(lambda: torch.mul(flat, 2.0, out=flat2))      # 4 B in, 4 B out per word: what the uniform transform moves
    print()
    print(f"kernels alone, {k} steps' noise per call ({words} words):")
    print(f"  walker + normal transform   {both / k * 1000:8.1f} us per step's noise")
    print(f"  walker + uniform transform  {walk_u / k * 1000:8.1f} us per step's noise   ({words / (walk_u * 1000):.0f} words/us: the walker bounds it)")
    print(f"  normal transform - uniform  {(both - walk_u) / k * 1000:8.1f} us per step's noise (difference of the two lines above)")
    print(f"  an elementwise pass alone   {stream_op / k * 1000:8.1f} us per step's noise (torch.mul over the same words: the uniform transform's traffic)")
    print(f"  torch.randn on the device   {philox / k * 1000:8.1f} us per step's noise (Philox, for scale)")
    print(f"  walker: {words / 624 / k:.0f} state regenerations per step's noise, three barrier-separated phases each -> "
          f"{(walk_u - stream_op) * 1e6 / (words / 624 * 3):.0f} ns per phase")


if __name__ == "__main__":
    main()
