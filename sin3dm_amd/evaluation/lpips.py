"""LPIPS of the reference's evaluation/lpips.py over multi-view renders (s3d_imgfeat.hip): AlexNet's `features`
on the device, once per image, the unit-normalised maps kept, and every pair of a view's renders in one launch per map.

Two outside inputs: torchvision's alexnet state dict and the reference's lpips_weights.ckpt; pass their paths.  No CPU fallback.
"""
from __future__ import annotations

import os

import numpy as np
import torch

from .. import _lib
from .sifid import ImageFeatureNet, load_state, read_png

_CONVS = (("features.0", 3, 64, 11), ("features.3", 64, 192, 5), ("features.6", 192, 384, 3), ("features.8", 384, 256, 3),
          ("features.10", 256, 256, 3))
ALEXNET_PARAM_SHAPES = {}
LPIPS_PARAM_SHAPES = {}
for _l, (_n, _ci, _co, _k) in enumerate(_CONVS):
    ALEXNET_PARAM_SHAPES[f"{_n}.weight"] = (_co, _ci, _k, _k)
    ALEXNET_PARAM_SHAPES[f"{_n}.bias"] = (_co,)
    LPIPS_PARAM_SHAPES[f"lpips_weights.{_l}.main.1.weight"] = (1, _co, 1, 1)


class AlexNetLpips(ImageFeatureNet):
    """The reference's LPIPS module on the device.  alexnet_weights: a path or a state dict of torchvision's alexnet (the
    classifier's keys are ignored); lpips_weights: the reference's lpips_weights.ckpt or its state dict."""
    NET = _lib.IMGFEAT_ALEXNET
    SHAPES = ALEXNET_PARAM_SHAPES
    WHAT = "alexnet"

    def __init__(self, alexnet_weights=None, lpips_weights=None):
        super().__init__(alexnet_weights)
        if lpips_weights is not None:
            self.load_lpips_weights(lpips_weights)

    def load_lpips_weights(self, weights):
        self.load_weights(weights, LPIPS_PARAM_SHAPES, "lpips")

    def pair_matrix_device(self, images, return_layers=False, return_activations=False):
        """total [n][n] float64 on the device: LPIPS(image i, image j); with return_layers also the five per-map terms [5][n][n],
        with return_activations also the five post-ReLU maps [n][H'][W'][C]."""
        t, _, acts = self._features(images, 0, return_activations)
        n = t.shape[0]
        total = torch.empty((n, n), dtype=torch.float64, device=t.device)
        layers = torch.empty((5, n, n), dtype=torch.float64, device=t.device) if return_layers else None
        _lib.check(self._lib.s3d_imgfeat_pairs(self._h, _lib.ptr(layers), _lib.ptr(total), _lib.stream_ptr()))
        out = (total,)
        if return_layers:
            out += (layers,)
        if return_activations:
            out += (acts,)
        return out if len(out) > 1 else total

    def pair_matrix(self, images, return_layers=False):
        out = self.pair_matrix_device(images, return_layers)
        return tuple(o.cpu().numpy() for o in out) if return_layers else out.cpu().numpy()


def lpips_values(gen_render_dirs, alexnet_weights, lpips_weights=None):
    """Per view, the mean over all unordered pairs of generated renders (calculate_lpips_given_images)."""
    gen_render_dirs = list(gen_render_dirs)
    net = alexnet_weights if isinstance(alexnet_weights, AlexNetLpips) else AlexNetLpips(alexnet_weights, lpips_weights)
    n_views = len(os.listdir(gen_render_dirs[0]))
    iu = np.triu_indices(len(gen_render_dirs), 1)
    values = []
    for i in range(n_views):
        imgs = np.stack([read_png(os.path.join(d, f"{i:03d}.png"))[..., :3] for d in gen_render_dirs])
        values.append(float(np.mean(net.pair_matrix(imgs)[iu])))
    return values


def eval_lpips(gen_render_dirs, alexnet_weights, lpips_weights=None):
    """calculate_multiview_lpips_given_paths: the mean over views."""
    return {"mv_lpips": float(np.mean(lpips_values(gen_render_dirs, alexnet_weights, lpips_weights)))}
