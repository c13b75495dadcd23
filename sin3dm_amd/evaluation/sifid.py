"""SIFID of the reference's evaluation/sifid.py over multi-view renders (s3d_imgfeat.hip): the stem of
torchvision's Inception-v3 on the device, the mean and covariance of its rows per image, and the Frechet distance between a
generated render's statistics and the reference render's.

The Inception checkpoint (torchvision's inception_v3 state dict) is the only outside input: pass its path.  The features have
no CPU fallback; the Frechet distance is float64 NumPy on the host (ssfid.frechet_distance).
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np
import torch

from .. import _lib
from ._weights import FeatureHandle, check_weights, load_state  # noqa: F401  (lpips.py and the tests take them from here)
from .ssfid import frechet_distance

SIFID_DIMS = (64, 192)
_UNITS = (("Conv2d_1a_3x3", 3, 32, 3), ("Conv2d_2a_3x3", 32, 32, 3), ("Conv2d_2b_3x3", 32, 64, 3), ("Conv2d_3b_1x1", 64, 80, 1),
          ("Conv2d_4a_3x3", 80, 192, 3))
INCEPTION_PARAM_SHAPES = {}
for _n, _ci, _co, _k in _UNITS:
    INCEPTION_PARAM_SHAPES[f"{_n}.conv.weight"] = (_co, _ci, _k, _k)
    for _s in ("weight", "bias", "running_mean", "running_var"):
        INCEPTION_PARAM_SHAPES[f"{_n}.bn.{_s}"] = (_co,)


def check_inception_weights(state):
    return check_weights(state, INCEPTION_PARAM_SHAPES, "inception_v3")


def read_png(path):
    """uint8 [H][W][3|4] of a PNG, read with PIL as data/obj_io.py reads textures: the samples matplotlib's imread divides by 255."""
    from PIL import Image
    with Image.open(path) as im:
        if im.mode not in ("RGB", "RGBA"):
            im = im.convert("RGBA" if "A" in im.getbands() or "transparency" in im.info else "RGB")
        return np.asarray(im, dtype=np.uint8).copy()


def as_image_batch(images):
    """uint8 device tensor [n][H][W][3|4] of: a device tensor, a NumPy array ([H][W][c] or [n][H][W][c]), or a list of PNG paths.
    A host torch tensor is refused: there is no CPU fallback, and a silent upload would hide one."""
    if isinstance(images, torch.Tensor):
        if not images.is_cuda:
            raise _lib.Sin3DMHipError("image features run on an MI355X: the tensor is on the host and there is no CPU fallback")
        t = images
    else:
        _lib.require_gpu()
        if isinstance(images, (list, tuple)) and images and isinstance(images[0], (str, bytes, os.PathLike)):
            arrs = [read_png(p) for p in images]
            if any(a.shape != arrs[0].shape for a in arrs):
                raise ValueError("images of one batch must have equal size and channels: " + ", ".join(str(a.shape) for a in arrs))
            images = np.stack(arrs)
        t = torch.from_numpy(np.array(images, copy=True, order="C")).to("cuda")
    if t.dtype != torch.uint8:
        raise ValueError(f"images are uint8 samples, got {t.dtype}")
    if t.dim() == 3:
        t = t[None]
    if t.dim() != 4 or t.shape[-1] not in (3, 4):
        raise ValueError(f"images are [n][H][W][3|4], got {tuple(t.shape)}")
    return t.contiguous()


class ImageFeatureNet(FeatureHandle):
    """A handle of s3d_imgfeat: parameters by name, the features call, the stage timing."""
    PREFIX, STAGES = "imgfeat", 6
    NET = None
    CREATE_ARGS = property(lambda self: (self.NET,))

    def out_dims(self, H, W, dims=0):
        """[(rows, columns, channels)] per unit.  NotImplementedError for dims the stem does not have, ValueError for an image
        too small for the network."""
        nl, hw, ch = C.c_int(0), (C.c_int * 10)(), (C.c_int * 5)()
        rc = self._lib.s3d_imgfeat_out_dims(self.NET, int(H), int(W), int(dims), C.byref(nl), hw, ch)
        if rc == _lib.ERR_INVALID:
            raise ValueError(_lib.last_error())
        _lib.check(rc)
        return [(hw[2 * l], hw[2 * l + 1], ch[l]) for l in range(nl.value)]

    def _features(self, images, dims, return_activations):
        t = as_image_batch(images)
        n, H, W, c = t.shape
        layers = self.out_dims(H, W, dims)
        acts, ptrs = None, None
        if return_activations:
            acts = [torch.empty((n, h, w, ch), dtype=torch.float32, device=t.device) for h, w, ch in layers]
            ptrs = (C.c_void_p * len(acts))(*[a.data_ptr() for a in acts])
        _lib.check(self._lib.s3d_imgfeat_features(self._h, _lib.ptr(t), n, H, W, c, int(dims), ptrs, _lib.stream_ptr()))
        return t, layers, acts

    def profile(self, on=True):
        """Record device events between the units of every following features call (tools/bench_imgmetrics.py)."""
        super().profile(on)

    def stage_ms(self):
        """Milliseconds of the last timed features call: units 1..5 (a pool counts with the unit it feeds), the unit normalisation."""
        return super().stage_ms()


class InceptionStem(ImageFeatureNet):
    """Blocks 0 and 1 of the reference's InceptionV3 wrapper on the device.  weights: a path or a state dict of torchvision's
    inception_v3; its other keys are ignored."""
    NET = _lib.IMGFEAT_INCEPTION
    SHAPES = INCEPTION_PARAM_SHAPES
    WHAT = "inception_v3"

    def statistics_device(self, images, dims=64, return_activations=False):
        """(mu [n][C], sigma [n][C][C]) as float64 device tensors, and the per-unit activations [n][H'][W'][C] when asked for."""
        t, layers, acts = self._features(images, dims, return_activations)
        n, c = t.shape[0], layers[-1][2]
        mu = torch.empty((n, c), dtype=torch.float64, device=t.device)
        sigma = torch.empty((n, c, c), dtype=torch.float64, device=t.device)
        _lib.check(self._lib.s3d_imgfeat_stats(self._h, _lib.ptr(mu), _lib.ptr(sigma), _lib.stream_ptr()))
        return (mu, sigma, acts) if return_activations else (mu, sigma)

    def statistics(self, images, dims=64, return_activations=False):
        """calculate_activation_statistics (sifid.py) per image: float64 NumPy mu [n][C], sigma [n][C][C]."""
        out = self.statistics_device(images, dims, return_activations)
        mu, sigma = out[0].cpu().numpy(), out[1].cpu().numpy()
        return (mu, sigma, out[2]) if return_activations else (mu, sigma)


def view_paths(render_dir, n_views):
    return [os.path.join(render_dir, f"{i:03d}.png") for i in range(n_views)]


def sifid_values(gen_render_dirs, ref_render_dir, weights, dims=64):
    """[n_views][n generated] distances of calculate_multiview_sifid_given_paths; one batch per view holds the reference render and
    every generated one when their sizes agree."""
    if dims not in SIFID_DIMS:
        raise NotImplementedError(f"sifid: dims {dims} is not built; {SIFID_DIMS} are")
    gen_render_dirs = list(gen_render_dirs)
    assert len(gen_render_dirs) > 0
    net = weights if isinstance(weights, InceptionStem) else InceptionStem(weights)
    n_views = len(os.listdir(ref_render_dir))
    values = []
    for i in range(n_views):
        name = f"{i:03d}.png"
        imgs = [read_png(os.path.join(ref_render_dir, name))] + [read_png(os.path.join(d, name)) for d in gen_render_dirs]
        if all(a.shape == imgs[0].shape for a in imgs):
            mu, sigma = net.statistics(np.stack(imgs), dims)
        else:
            stats = [net.statistics(a, dims) for a in imgs]
            mu, sigma = np.concatenate([s[0] for s in stats]), np.concatenate([s[1] for s in stats])
        values.append([frechet_distance(mu[0], sigma[0], mu[k], sigma[k]) for k in range(1, len(imgs))])
    return values


def eval_sifid(gen_render_dirs, ref_render_dir, weights, dims=64):
    """calculate_multiview_sifid_given_paths: the mean over views of the mean over the generated renders."""
    values = sifid_values(gen_render_dirs, ref_render_dir, weights, dims)
    return {f"mv_sifid_dim{dims}": float(np.mean([np.mean(v) for v in values]))}
