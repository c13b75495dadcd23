#!/usr/bin/env python3
"""Bits of the auto-encoder training iteration, for comparing two builds of the library (tools/lib_ab.sh swaps them): per
network variant (sdftex, geo, skip8, pbr) two consecutive iterations on fixed seeds in this process, one sha256 per variant,
BWD_SIDE setting and quantity (losses, pred, flat gradient; both iterations hashed together).  --save keeps the tensors
themselves, so that two runs can be compared with torch.equal on the CPU afterwards.  --decode hashes the inference handle instead:
decode, decode_grid at resolution 12, sdf_and_grad, project_to_surface(iters=2) and every group's plane_features of the same four
variants on the same planes and points, and of one geometry-only net of widths (16, 32), which the handle pads to 32.

    python tools/ae_bits.py [--decode] [--fm 10 14 6] [--points 257] [--side 0] [--save FILE.pt]"""
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
ap.add_argument("--decode", action="store_true", help="the inference handle's outputs instead of the training iteration's")
args = ap.parse_args()
(H, W, D), N, dev = args.fm, args.points, torch.device("cuda:0")
VARIANTS = {"sdftex": dict(use_tex=True, tc=3), "geo": dict(use_tex=False, tc=0), "skip8": dict(use_tex=True, tc=8),
            "pbr": dict(use_tex=True, tc=8, pbr=True)}
if args.side is not None:
    _lib.set_option("BWD_SIDE", args.side)
tag = "inline" if args.side == 0 else "side"
kept = {}


def make_net(v, up=64, hid=256):
    if v.get("pbr"):
        shapes = T.pbr_param_shapes(4, 8, up, hid, 4, 8, with_encoder=True)
        net = AutoEncoderGroupPBR(4, 8, up, hid, 4, tex_channels=8)
    else:
        shapes = (T.ae_param_shapes(4, 8, up, hid, 4, v["tc"], with_encoder=True) if v["use_tex"]
                  else T.geo_only_param_shapes(4, up, hid, 4, with_encoder=True))
        net = AutoEncoderGroupSkip(4, 8, up, hid, 4, use_tex=v["use_tex"], tex_channels=max(v["tc"], 1))
    net.load_state_dict(T.synthetic_state_dict(shapes, 5), strict=False)
    return net.to(dev)


def keep(key, t):
    assert torch.isfinite(t).all(), key
    kept[key] = t.detach().cpu().reshape(-1).clone()
    print(f"{key.replace('.', ' ')} {hashlib.sha256(kept[key].numpy().tobytes()).hexdigest()}", flush=True)


def decode_bits(name, v):
    """the inference handle: every entry point that reads the prepared planes"""
    net = make_net(v, *v.get("widths", (64, 256)))
    net.reset_aabb([-1.0, -0.9, -0.8, 1.0, 0.9, 0.8])
    g = torch.Generator().manual_seed(1300)
    fm = [(torch.rand((1, net.in_feat_channels, a, b), generator=g) * 2 - 1).to(dev) for a, b in ((H, W), (H, D), (W, D))]
    pts = (torch.rand((N, 3), generator=g) * 2.2 - 1.1).to(dev)              # past the box: the border clamp is taken
    keep(f"{name}.decode", net.decode(pts, fm))
    keep(f"{name}.decode_grid", net.decode_grid(fm, 12))
    for what, res in (("sdf_and_grad", net.sdf_and_grad(pts, fm)), ("project_to_surface", net.project_to_surface(pts, fm, iters=2))):
        keep(f"{name}.{what}", torch.cat([t.reshape(-1) for t in res]))
    for group in ("geo",) + (("tex",) if v["use_tex"] else ()) + (("tex0",) if v.get("pbr") else ()):
        keep(f"{name}.plane_features_{group}", torch.cat([t.reshape(-1) for t in net.plane_features(fm, group)]))


def train_bits(name, v):
    """two consecutive training iterations"""
    net = make_net(v)
    net.build_training_tier(**({"material_heads": True} if v.get("pbr") else {}))
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


if args.decode:
    for name, v in dict(VARIANTS, geo16x32=dict(use_tex=False, tc=0, widths=(16, 32))).items():
        decode_bits(name, v)
else:
    for name, v in VARIANTS.items():
        train_bits(name, v)
if args.save:
    torch.save(kept, args.save)
