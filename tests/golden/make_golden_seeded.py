#!/usr/bin/env python3
"""Generate tests/golden/seeded.npz: SEEDED runs of the reference (PyTorch-CPU), nothing patched.

Each trajectory case is `torch.manual_seed(k)` followed by the reference's own p_sample_loop / ddim_sample_loop, which draw
x_T and every step's eps from torch's default CPU generator; stored are only k, (B, H, W, D), the respacing, the final
sample and `torch.rand(4)` drawn right after the loop (a witness of the stream position).  Two bare calls pin the stream
itself: the full `torch.randn(n)` and `torch.rand(n)` outputs after `torch.manual_seed`.  Like make_golden.py this runs only
where the reference is present; what is committed is data.

    python tests/golden/make_golden_seeded.py      # rewrites tests/golden/seeded.npz
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_golden import make_diffusion, make_unet, save  # noqa: E402  (sets the thread count, disables grad)

# tag -> (seed, (B, H, W, D), respacing, ddim)
CASES = {
    "ddpm20_b2": (1234, (2, 10, 14, 6), "20", False),
    "ddpm20_b1_s0": (1000, (1, 10, 14, 6), "20", False),      # the batch-1 runs the per-sample form of the B=2 shape reproduces
    "ddpm20_b1_s1": (1001, (1, 10, 14, 6), "20", False),
    "ddim10_b1": (77, (1, 9, 13, 6), "10", True),             # 12 * 15 * 19 = 3420 elements per call: the tail rule
    "ddpm100_b1": (5, (1, 9, 13, 6), "100", False),
    "ddpm1000_b1": (2024, (1, 10, 14, 6), "", False),
}
# tag -> (seed, n): bare torch.randn(n) / torch.rand(n) after manual_seed
STREAMS = {"n3840": (31, 3840), "n3420": (32, 3420)}


def main():
    out = {}
    model = make_unet(32)
    for tag, (seed, (B, H, W, D), resp, ddim) in CASES.items():
        diff = make_diffusion(resp)
        shape = (B, 12, H + D, W + D)
        torch.manual_seed(seed)
        fn = diff.ddim_sample_loop if ddim else diff.p_sample_loop
        final = fn(model, shape, model_kwargs=dict(H=H, W=W, D=D))
        rand4 = torch.rand(4)
        assert float(final[..., H:, W:].abs().max()) == 0.0, "DxD corner must end at exactly 0"
        out[f"{tag}.seed"] = np.asarray(seed, dtype=np.int64)
        out[f"{tag}.bhwd"] = np.asarray([B, H, W, D], dtype=np.int64)
        out[f"{tag}.respacing"] = np.asarray(resp)
        out[f"{tag}.ddim"] = np.asarray(int(ddim), dtype=np.int64)
        out[f"{tag}.final"] = final
        out[f"{tag}.rand4"] = rand4
    for tag, (seed, n) in STREAMS.items():
        out[f"{tag}.seed"] = np.asarray(seed, dtype=np.int64)
        torch.manual_seed(seed)
        out[f"{tag}.randn"] = torch.randn(n)
        out[f"{tag}.rand_after"] = torch.rand(4)
        torch.manual_seed(seed)
        out[f"{tag}.rand"] = torch.rand(n)
    save("seeded", **out)


if __name__ == "__main__":
    main()
