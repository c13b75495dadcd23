#!/usr/bin/env python3
"""Bits of the auto-encoder training iteration, for comparing two builds of the library (tools/lib_ab.sh swaps them): per
network variant (sdftex, geo, skip8, pbr) two consecutive iterations on fixed seeds in this process, one sha256 per variant,
BWD_SIDE setting and quantity (losses, pred, flat gradient; both iterations hashed together).  --save keeps the tensors
themselves, so that two runs can be compared with torch.equal on the CPU afterwards.

    python tools/ae_bits.py [--fm 10 14 6] [--points 257] [--side 0] [--save FILE.pt]"""
import argparse
import hashlib
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import torch  # noqa: E402

from sin3dm_amd import _lib, testing as T  # noqa: E402
from sin3dm_amd.encoding.model import ae_loss_cfg  # noqa: E402
from sin3dm_amd.encoding.networks import AutoEncoderGroupPBR, AutoEncoderGroupSkip  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--fm", type=int, nargs=3, default=(10, 14, 6))
ap.add_argument("--points", type=int, default=257)
ap.add_argument("--side", type=int, default=None, help="0: BWD_SIDE off (everything in line on one stream); default: the library's default")
ap.add_argument("--save", default=None)
args = ap.parse_args()
(H, W, D), N, dev = args.fm, args.points, torch.device("cuda:0")
VARIANTS = {"sdftex": dict(use_tex=True, tc=3), "geo": dict(use_tex=False, tc=0), "skip8": dict(use_tex=True, tc=8),
            "pbr": dict(use_tex=True, tc=8, pbr=True)}
if args.side is not None:
    _lib.set_option("BWD_SIDE", args.side)
tag = "inline" if args.side == 0 else "side"
kept = {}
for name, v in VARIANTS.items():
    if v.get("pbr"):
        shapes = T.pbr_param_shapes(4, 8, 64, 256, 4, 8, with_encoder=True)
        net = AutoEncoderGroupPBR(4, 8, 64, 256, 4, tex_channels=8)
    else:
        shapes = (T.ae_param_shapes(4, 8, 64, 256, 4, v["tc"], with_encoder=True) if v["use_tex"]
                  else T.geo_only_param_shapes(4, 64, 256, 4, with_encoder=True))
        net = AutoEncoderGroupSkip(4, 8, 64, 256, 4, use_tex=v["use_tex"], tex_channels=max(v["tc"], 1))
    net.load_state_dict(T.synthetic_state_dict(shapes, 5), strict=False)
    net.to(dev).build_training_tier(**({"material_heads": True} if v.get("pbr") else {}))
    g = torch.Generator().manual_seed(1200)
    vol = torch.rand((1, 1 + v["tc"], 2 * H, 2 * W, 2 * D), generator=g)
    vol[:, :1] = vol[:, :1] * 0.2 - 0.1
    vol = vol.to(dev)
    net.set_volume(vol)
    out = {"losses": [], "pred": [], "grads": []}
    for it in range(2):
        g = torch.Generator().manual_seed(50 + it)
        pts = (torch.rand((N, 3), generator=g) * 2.2 - 1.1).to(dev)          # past the box: the border clamp is taken
        sdf = (torch.rand((N, 1), generator=g) * 0.1 - 0.05).to(dev)
        tex = torch.rand((N, v["tc"]), generator=g).to(dev) if v["tc"] else None
        losses, pred, grads = net.loss_and_grads(vol, pts, sdf, tex, ae_loss_cfg("weightedl1", "l1", 0.05), want_pred=True)
        torch.cuda.synchronize()
        for k, t in zip(("losses", "pred", "grads"), (losses, pred, grads)):
            out[k].append(t.detach().cpu().clone())
    for k, ts in out.items():
        assert all(torch.isfinite(t).all() for t in ts), (name, k)
        kept[f"{name}.{tag}.{k}"] = torch.cat([t.reshape(-1) for t in ts])
        print(f"{name} {tag} {k} {hashlib.sha256(kept[f'{name}.{tag}.{k}'].numpy().tobytes()).hexdigest()}", flush=True)
if args.save:
    torch.save(kept, args.save)
