"""The cases of the SSFID tests and a float64 restatement of the reference's computation, shared by tests/test_ssfid_host.py,
tests/test_ssfid_gpu.py and the fixture generator tests/golden/make_golden_ssfid.py.  Nothing is stored: the weights come from a
seed, the volumes from formulas.

The restatement is written from the module definitions of evaluation/classifier3D.py and evaluation/ssfid.py:65-77
(F.conv3d, F.instance_norm, F.leaky_relu, np.cov); tests/golden/ssfid.npz pins it to the reference's own modules.
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

import eval_cases as E
from sin3dm_amd.testing import gyroid_sdf, synthetic_state_dict

WEIGHT_SEED = 7
PARAM_SHAPES = {"conv_1.weight": (32, 1, 4, 4, 4), "conv_1.bias": (32,), "conv_2.weight": (64, 32, 4, 4, 4), "conv_2.bias": (64,)}
LAYERS = (1, 2)

# (reference volume, generated volume): reference_occupancy (sdf <= 0) against generated_occupancy (sdf < 0) of tests/eval_cases.py
PAIRS = {
    "p32": ("ref32", "gen32a"),          # (32, 26, 20): layer 2 extents (8, 6, 5)
    "p40": ("ref40", "gen40a"),          # (40, 33, 25): odd extents, (20, 16, 12) then (10, 8, 6)
    "p48": ("ref48", "gen48b"),          # (48, 40, 36): more than one layer-2 tile along every axis
    "pdiv": ("div0", "div4"),
    "prank": ("rank_a", "rank_b"),       # (16, 12, 8): 24 rows for 64 channels at layer 2, rank-deficient covariances
}
LONG_SHAPE, FREE_SHAPE, RANK_SHAPE = (96, 80, 64), (32, 26, 20), (16, 12, 8)
ACT_CASE = "ref32"                       # the volume whose activations the fixture stores
E2E_CASE = "p11_48"                      # the eval_cases.LP_CASES entry the end-to-end value is recorded on (two generated shapes)
E2E_RESOLUTION = 48


def weights(as_torch=True):
    return synthetic_state_dict(PARAM_SHAPES, WEIGHT_SEED, as_torch=as_torch)


@functools.lru_cache(maxsize=None)
def volume(name):
    """bool [X][Y][Z].  Names of eval_cases.VOLUMES: 'ref*' and 'div0' by the training shape's rule, the others by the decoders'."""
    if name == "long":                   # 61 440 rows at layer 1, 7 680 at layer 2
        return gyroid_sdf(LONG_SHAPE, 3.0, (0.2, -0.1, 0.3), thickness=0.6) < 0
    if name == "free":
        return np.zeros(FREE_SHAPE, dtype=bool)
    if name == "rank_a":
        return gyroid_sdf(RANK_SHAPE, 1.0, (0.0, 0.0, 0.0), thickness=0.6) < 0
    if name == "rank_b":
        return gyroid_sdf(RANK_SHAPE, 1.0, (0.5, -0.3, 0.2), thickness=0.6) < 0
    ref_names = {r for r, _ in PAIRS.values()}
    return E.reference_occupancy(name) if name in ref_names else E.generated_occupancy(name)


def volume_names():
    names = []
    for r, g in PAIRS.values():
        names += [r, g]
    return names + ["long", "free"]


def restate(vox, w, layer, fault=None):
    """Float64: (activations [rows][C], mu [C], sigma [C][C]) of one occupancy grid.  fault: None, or one of the three defects the
    host test injects: 'pad_first' (the second convolution's out-of-range taps read leaky(norm(0)) instead of 0), 'unbiased_var'
    (InstanceNorm with the unbiased variance), 'ddof0' (the population covariance)."""
    w = {k: torch.as_tensor(v).double() for k, v in w.items()}
    x = torch.as_tensor(np.asarray(vox)).double()[None, None]

    def norm_act(y):
        if fault == "unbiased_var":
            mean = y.mean(dim=(2, 3, 4), keepdim=True)
            y = (y - mean) / torch.sqrt(y.var(dim=(2, 3, 4), keepdim=True, unbiased=True) + 1e-5)
        else:
            y = F.instance_norm(y, eps=1e-5)
        return F.leaky_relu(y, 0.01)

    y1 = F.conv3d(x, w["conv_1.weight"], w["conv_1.bias"], stride=2, padding=1)
    a = norm_act(y1)
    if layer == 2:
        if fault == "pad_first":
            mean = y1.mean(dim=(2, 3, 4), keepdim=True)
            fill = F.leaky_relu((0.0 - mean) / torch.sqrt(y1.var(dim=(2, 3, 4), keepdim=True, unbiased=False) + 1e-5), 0.01)
            padded = fill.expand(-1, -1, *(s + 2 for s in a.shape[2:])).clone()
            padded[:, :, 1:-1, 1:-1, 1:-1] = a
            a = norm_act(F.conv3d(padded, w["conv_2.weight"], w["conv_2.bias"], stride=2, padding=0))
        else:
            a = norm_act(F.conv3d(a, w["conv_2.weight"], w["conv_2.bias"], stride=2, padding=1))
    act = a.permute(0, 2, 3, 4, 1).reshape(-1, a.shape[1]).numpy()
    mu = np.mean(act, axis=0)
    sigma = np.cov(act, rowvar=False, ddof=0 if fault == "ddof0" else 1)
    return act, mu, sigma


@functools.lru_cache(maxsize=None)
def restated(name, layer):
    """The unfaulted restatement of a named volume, computed once per process and shared; do not write to the arrays."""
    out = restate(volume(name), weights(), layer)
    for a in out:
        a.setflags(write=False)
    return out


def bound(gap, value):
    """The tolerance of DESIGN.md §21: ten times the reference's own float32-versus-float64 gap on this input, and never below one
    float32 ulp of the statistic's largest magnitude."""
    return max(10.0 * float(gap), 2.0 ** -23 * float(np.max(np.abs(value))) if np.size(value) else 0.0)


def check_tail(what, rows, mu, sigma):
    """The statistics tail on its own (s3d_rowstats.h): a device mean and ddof = 1 covariance against np.mean / np.cov of the
    float32 rows [R][C] the device itself returned, so that no convolution error enters.  The tolerance is the forward-error bound
    of a float64 sum of R terms in any order, 8 R 2^-53 sum |terms|: for sigma[i][j] over the products and the product of the
    column sums, (sum_r |a_ri a_rj| + |sum_r a_ri| |sum_r a_rj| / R) / (R - 1); for mu[i] over sum_r |a_ri| / R."""
    a = np.asarray(rows, dtype=np.float64)
    R = a.shape[0]
    u, s, ab = 8.0 * R * 2.0 ** -53, np.abs(a.sum(axis=0)), np.abs(a)
    mu_b, sigma_b = u * ab.sum(axis=0) / R, u * (ab.T @ ab + np.outer(s, s) / R) / (R - 1)
    mu_e, sigma_e = np.abs(mu - a.mean(axis=0)), np.abs(sigma - np.cov(a, rowvar=False))
    print(f"{what}: {R} rows, mu err {mu_e.max():.3e} bound there {mu_b.flat[mu_e.argmax()]:.3e}, "
          f"sigma err {sigma_e.max():.3e} bound there {sigma_b.flat[sigma_e.argmax()]:.3e}")
    assert mu.shape == mu_b.shape and sigma.shape == sigma_b.shape and np.all(mu_e <= mu_b) and np.all(sigma_e <= sigma_b), what
