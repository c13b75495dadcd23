"""SSFID of the reference's evaluation/ssfid.py (s3d_ssfid.hip): the first two layers of the 3-D voxel classifier
on the device, the mean and covariance of their activations, and the Frechet distance between a generated shape's statistics and
the training shape's.

The classifier checkpoint (`Clsshapenet_128.pth`) is the only outside input: pass its path.  The features have no CPU fallback;
the Frechet distance is float64 NumPy on the host.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from .. import _lib
from ._weights import FeatureHandle, check_weights, load_state
from .patch_utils import _as_occupancy, _dims, load_sdfgrid2vox, load_voxgrid

PARAM_SHAPES = {"conv_1.weight": (32, 1, 4, 4, 4), "conv_1.bias": (32,), "conv_2.weight": (64, 32, 4, 4, 4), "conv_2.bias": (64,)}
_HINT = " (the classifier of ef_dim = 32)"


def check_classifier_weights(state):
    """The four tensors of PARAM_SHAPES out of a state dict of the reference's `classifier`, as contiguous float32 on the host;
    every other key (conv_3 ... linear1) is ignored.  KeyError names a missing key, ValueError a wrong shape."""
    return check_weights(state, PARAM_SHAPES, "classifier", _HINT)


def load_classifier_weights(path):
    """torch.load of the reference's Clsshapenet_128.pth (a state dict), reduced to the two layers SSFID reads."""
    return check_classifier_weights(load_state(path))


class VoxelClassifier(FeatureHandle):
    """Layers 1 and 2 of the reference's classifier on the device.  weights: a path or a state dict."""
    PREFIX, STAGES = "ssfid", 5
    SHAPES, WHAT, HINT = PARAM_SHAPES, "classifier", _HINT

    def features_device(self, vox, out_layer=2, return_activations=False):
        """(mu [C], sigma [C][C]) as float64 device tensors, and the activations [rows][C] (float32) when asked for."""
        vox = _as_occupancy(vox)
        dims, od, ch = _dims(vox.shape), (C.c_int * 3)(), C.c_int(0)
        _lib.check(self._lib.s3d_ssfid_out_dims(dims, int(out_layer), od, C.byref(ch)))
        c = ch.value
        mu = torch.empty(c, dtype=torch.float64, device=vox.device)
        sigma = torch.empty((c, c), dtype=torch.float64, device=vox.device)
        act = torch.empty((od[0] * od[1] * od[2], c), dtype=torch.float32, device=vox.device) if return_activations else None
        _lib.check(self._lib.s3d_ssfid_features(self._h, _lib.ptr(vox), dims, int(out_layer), _lib.ptr(act), _lib.ptr(mu), _lib.ptr(sigma),
                                                _lib.stream_ptr()))
        return (mu, sigma, act) if return_activations else (mu, sigma)

    def profile(self, on=True):
        """Record device events between the stages of every following call (tools/bench_ssfid.py)."""
        super().profile(on)

    def stage_ms(self):
        """Milliseconds of the last timed call: layer 1, its statistics, layer 2, its statistics, the covariance."""
        return super().stage_ms()

    def features(self, vox, out_layer=2, return_activations=False):
        """calculate_activation_statistics (:65): (mu, sigma) as float64 NumPy; with return_activations also the activations, rows
        in [X'][Y'][Z'] order, as a device tensor."""
        out = self.features_device(vox, out_layer, return_activations)
        mu, sigma = out[0].cpu().numpy(), out[1].cpu().numpy()
        return (mu, sigma, out[2]) if return_activations else (mu, sigma)


def _sqrt_psd(s):
    """The symmetric square root of a symmetric positive semi-definite matrix: eigh, eigenvalues clipped at 0."""
    w, v = np.linalg.eigh((s + s.T) * 0.5)
    return (v * np.sqrt(np.clip(w, 0.0, None))) @ v.T


def frechet_distance(mu1, sigma1, mu2, sigma2):
    """|mu1 - mu2|^2 + Tr s1 + Tr s2 - 2 Tr sqrt(s1 s2) (calculate_frechet_distance :11) in float64.  s1 s2 is similar to the
    symmetric positive semi-definite s1^(1/2) s2 s1^(1/2), so the trace of its square root is the sum of the square roots of that
    matrix's eigenvalues: no square root of a non-symmetric matrix, nothing imaginary, finite for rank-deficient inputs."""
    mu1, mu2 = np.atleast_1d(np.asarray(mu1, dtype=np.float64)), np.atleast_1d(np.asarray(mu2, dtype=np.float64))
    s1, s2 = np.atleast_2d(np.asarray(sigma1, dtype=np.float64)), np.atleast_2d(np.asarray(sigma2, dtype=np.float64))
    assert mu1.shape == mu2.shape, "Training and test mean vectors have different lengths"
    assert s1.shape == s2.shape, "Training and test covariances have different dimensions"
    r = _sqrt_psd(s1)
    m = r @ s2 @ r
    w = np.linalg.eigvalsh((m + m.T) * 0.5)
    tr_covmean = float(np.sum(np.sqrt(np.clip(w, 0.0, None))))
    diff = mu1 - mu2
    return float(diff.dot(diff) + np.trace(s1) + np.trace(s2) - 2.0 * tr_covmean)


def ssfid_values(paths, ref_path, weights, out_layer=2, resolution=128):
    """The per-shape distances of eval_SSFID_given_paths (:81); the reference shape's statistics are computed once."""
    net = weights if isinstance(weights, VoxelClassifier) else VoxelClassifier(weights)
    ref = load_sdfgrid2vox(ref_path, resolution=resolution)
    mu_r, sigma_r = net.features(ref, out_layer)
    values = []
    for path in paths:
        gen = load_voxgrid(path, resolution=resolution)
        if gen.shape != ref.shape:
            raise RuntimeError("Generated shape and reference shape shall have equal size.")
        mu_f, sigma_f = net.features(gen, out_layer)
        values.append(frechet_distance(mu_r, sigma_r, mu_f, sigma_f))
    return values


def eval_ssfid(paths, ref_path, weights, out_layer=2, resolution=128):
    """eval_SSFID_given_paths (:81): the mean and the (population) standard deviation of the distances, round(6)."""
    values = ssfid_values(paths, ref_path, weights, out_layer, resolution)
    return {"SSFID_avg": float(np.mean(values).round(6)), "SSFID_std": float(np.std(values).round(6))}
