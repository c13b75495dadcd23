"""The grid of cases that holds the auto-encoder training step of the geometry-only net (variant 1), the skip net with 8 material
channels and its three grouped losses (variant 0), the skip net at other texture widths and the PBR net (variant 2) to float64
autograd: shapes, configs, point counts, placements, aabbs and loss modes (tests/test_hip_ae_variants_f64.py on the device,
tests/test_ae_variants_f64_host.py without one, tools/ae_variants_f64_report.py for the figures).

The reference is the restatement of tests/ae_variants_cases.py / tests/ae_pbr_cases.py, which reproduces the vectors captured
from the reference implementation (tests/golden/ae_variants.npz, ae_pbr.npz) and runs in the dtype of its inputs.  Weights are
sin3dm_amd.testing.synthetic_state_dict, volumes and batches are seeded; nothing is stored.

Batches are drawn as tests/test_hip_ae_reference.py draws them (its placements), and a row is redrawn until in float64 nothing
lies within KINK of a kink: every hidden ReLU pre-activation of every MLP the network runs, the sdf residual, the sdf sample
itself under weightedl1 (sign(sdf)), and every material residual.  N stays fixed.

BOUNDS holds, per case and quantity, (bound, gap): gap is the restatement's own float32-versus-float64 error on that case (the
same function on float32 and on float64 inputs, measured on the CPU by tools/ae_variants_f64_report.py --gaps), and the bound
is the shared one of tests/test_hip_ae_reference.py (SHARED) wherever ten times the gap is below it, otherwise ten times the gap
rounded up to two digits — the rule of ae_pbr_cases.BOUNDS.  No bound comes from what the device gave."""
import functools
import math
from collections import OrderedDict

import numpy as np

import ae_pbr_cases as P
import ae_variants_cases as V
from sin3dm_amd import testing as T
from test_hip_ae_reference import AABB, AABB_OFF, AABB_UNIT, KINK, _placer

# encode / pred / decode 2e-5, losses 2e-5 (relative), every gradient tensor 5e-4 as |got - ref| / max(|ref|, 1e-2 gmax) in L2,
# analytically zero gradients 1e-5 of gmax; norm1 is the PBR net's twice-used norm (max-abs over max-abs, per tensor)
SHARED = {"encode": 2e-5, "pred": 2e-5, "loss": 2e-5, "grad": 5e-4, "zero": 1e-5, "norm1": 5e-4}
LOSS = dict(sdf_loss="weightedl1", thr=0.05, ratio=0.999, tw=1.0, renorm=False)
TEX_CHANNELS = {"geo": 0, "skip": 8, "pbr": 8}
# conv biases whose only consumer is an InstanceNorm: a constant per channel, which the norm removes.  For the PBR net that is
# also everything that adds a constant to f0 = tex_convs.0(...), which only tex_convs.1's input norm reads.
ZERO_GRAD = {
    "geo": ("geo_encoder.bias", "geo_convs.in_layers.0.bias"),
    "skip": ("geo_encoder.bias", "geo_convs.in_layers.0.bias", "tex_encoder.bias", "tex_convs.in_layers.0.bias"),
    "pbr": ("geo_encoder.bias", "geo_convs.in_layers.0.bias", "tex_encoder.bias", "tex_convs.0.in_layers.0.bias",
            "tex_convs.0.out_layers.1.bias", "tex_convs.0.shortcut.bias", "tex_convs.1.in_layers.1.bias"),
}
NORM1 = tuple(f"tex_convs.1.norm_{p}.{leaf}" for p in V.PLANES for leaf in ("weight", "bias"))


def _case(net, hwd, cfg, N, place="uniform", aabb=AABB, seed=0, tc=None, offset=0.0, enc=None, band_rows=None, **loss):
    return dict(net=net, hwd=hwd, cfg=cfg, N=N, place=place, aabb=aabb, seed=seed, tc=TEX_CHANNELS[net] if tc is None else tc,
                offset=offset, enc=enc or ("pbr" if net == "pbr" else "skip"), band_rows=band_rows, loss=dict(LOSS, **loss))


def _band_rows(thr, ratio):
    """|sdf| at the float32 band fl32(thr * ratio), one ulp either side of it, and at the product of the two rounded factors
    (one ulp below the band at (0.03, 0.9), one above at (0.15, 0.999)); both signs"""
    f = np.float32
    b = f(thr * ratio)
    vals = np.asarray([np.nextafter(b, f(0)), b, np.nextafter(b, f(1)), f(f(thr) * f(ratio))], f)
    assert vals[3] != b
    return np.concatenate([vals, -vals])


def _cases():
    big = 65536 + 17
    shapes = OrderedDict((
        # planes H x W x D, (geo, tex, up, hidden, layers), N, placement, aabb
        ("geo-1x6x5-N1-uniform", _case("geo", (1, 6, 5), (4, 8, 32, 32, 4), 1, seed=1)),
        ("geo-2x33x3-N64-lattice-unit", _case("geo", (2, 33, 3), (8, 4, 32, 64, 4), 64, "lattice", AABB_UNIT, 2)),
        ("geo-7x4x9-N63-faces-off", _case("geo", (7, 4, 9), (4, 8, 64, 256, 4), 63, "faces", AABB_OFF, 3)),
        ("geo-13x16x11-N65553-uniform", _case("geo", (13, 16, 11), (4, 4, 96, 128, 4), big, seed=4)),
        ("skip8-1x6x5-N1000-cell", _case("skip", (1, 6, 5), (4, 8, 64, 256, 4), 1000, "cell", seed=5)),
        ("skip8-7x4x9-N65-faces-off", _case("skip", (7, 4, 9), (8, 4, 32, 64, 4), 65, "faces", AABB_OFF, 6)),
        ("skip8-2x33x3-N1-uniform", _case("skip", (2, 33, 3), (4, 4, 96, 128, 4), 1, seed=7)),
        ("skip8-13x16x11-N65553-uniform-off", _case("skip", (13, 16, 11), (4, 8, 32, 32, 4), big, aabb=AABB_OFF, seed=8)),
        # the two-loss call with ooff / TC away from 3 and 8
        ("skip1-7x4x9-N257-uniform", _case("skip", (7, 4, 9), (4, 8, 32, 64, 4), 257, seed=9, tc=1)),
        ("skip2-7x4x9-N257-uniform", _case("skip", (7, 4, 9), (4, 8, 32, 64, 4), 257, seed=10, tc=2)),
        ("skip5-7x4x9-N257-uniform", _case("skip", (7, 4, 9), (4, 8, 32, 64, 4), 257, seed=11, tc=5)),
        # 1x6x5 and 3x3x3 are at or below the 3x3 blocks' reach; at 3x3x3 every pixel is a border pixel
        ("pbr-1x6x5-N1-uniform", _case("pbr", (1, 6, 5), (4, 8, 32, 64, 4), 1, seed=12)),
        ("pbr-2x33x3-N64-lattice-unit", _case("pbr", (2, 33, 3), (4, 8, 64, 256, 4), 64, "lattice", AABB_UNIT, 13)),
        ("pbr-3x3x3-N63-cell", _case("pbr", (3, 3, 3), (4, 8, 32, 64, 4), 63, "cell", seed=14)),
        ("pbr-7x4x9-N1000-faces-off", _case("pbr", (7, 4, 9), (8, 4, 64, 128, 4), 1000, "faces", AABB_OFF, 15)),
        ("pbr-13x16x11-N65553-uniform-off", _case("pbr", (13, 16, 11), (4, 8, 32, 32, 4), big, aabb=AABB_OFF, seed=16)),
        ("pbr.offset-2x33x3-N65-uniform", _case("pbr", (2, 33, 3), (4, 8, 64, 256, 4), 65, seed=17, offset=3.0)),
    ))
    modes = OrderedDict()
    for i, (net, tag) in enumerate((("skip", "skip8"), ("pbr", "pbr"))):
        def m(seed, **loss):
            return _case(net, (7, 4, 9), (4, 8, 32, 64, 4), 1000, seed=seed + 10 * i, **loss)
        modes[f"{tag}-l1"] = m(20, sdf_loss="l1")
        modes[f"{tag}-weightedl1"] = m(21)
        modes[f"{tag}-weight0.37-ratio0.5"] = m(22, tw=0.37, ratio=0.5)
        modes[f"{tag}-renorm"] = m(23, renorm=True)
        modes[f"{tag}-band-holds-all"] = m(24, all_band=True)
        modes[f"{tag}-band-holds-one"] = m(25, one_row=True)
    for i, enc in enumerate(("skip", "pbr")):                  # data_type sdf on either network class: variant 1 both times
        def g(seed, **loss):
            return _case("geo", (7, 4, 9), (4, 8, 32, 64, 4), 1000, seed=seed + 10 * i, enc=enc, **loss)
        modes[f"geo.{enc}-l1"] = g(40, sdf_loss="l1")
        modes[f"geo.{enc}-weightedl1"] = g(41)
        modes[f"geo.{enc}-renorm"] = g(42, renorm=True)
    band = OrderedDict()
    for net, tag, s in (("skip", "skip8", 60), ("pbr", "pbr", 62)):
        for j, (thr, ratio) in enumerate(((0.03, 0.9), (0.15, 0.999))):
            band[f"{tag}-band-{thr}-{ratio}"] = _case(net, (7, 4, 9), (4, 8, 64, 256, 4), 64, seed=s + j, thr=thr, ratio=ratio,
                                                      band_rows=_band_rows(thr, ratio))
    return shapes, modes, band


SHAPES, MODES, BAND = _cases()
CASES = OrderedDict(list(SHAPES.items()) + list(MODES.items()) + list(BAND.items()))

QUANTITIES = ("encode", "pred", "loss", "grad", "zero", "norm1")


def _row(*pairs):
    return dict(zip(QUANTITIES, pairs))


# (bound, gap) per case for encode, pred, loss / grad, zero and, for the PBR net, norm1; written by
# tools/ae_variants_f64_report.py --gaps from the CPU alone
BOUNDS = {
    "geo-1x6x5-N1-uniform":
        _row((2.0e-05, 3.33e-07), (2.0e-05, 8.15e-08), (2.0e-05, 3.13e-08),
             (5.0e-04, 8.54e-07), (1.0e-05, 2.61e-08)),
    "geo-2x33x3-N64-lattice-unit":
        _row((2.0e-05, 5.46e-07), (2.0e-05, 8.11e-07), (2.0e-05, 1.57e-07),
             (5.0e-04, 7.87e-07), (1.0e-05, 5.96e-08)),
    "geo-7x4x9-N63-faces-off":
        _row((2.0e-05, 2.34e-07), (2.0e-05, 5.97e-07), (2.0e-05, 6.05e-08),
             (5.0e-04, 5.70e-07), (1.0e-05, 1.45e-08)),
    "geo-13x16x11-N65553-uniform":
        _row((2.0e-05, 3.41e-07), (2.0e-05, 1.52e-06), (2.0e-05, 2.12e-08),
             (5.0e-04, 9.80e-07), (1.0e-05, 1.25e-08)),
    "skip8-1x6x5-N1000-cell":
        _row((2.0e-05, 8.76e-07), (2.0e-05, 5.79e-07), (2.0e-05, 7.84e-07),
             (5.0e-04, 9.74e-07), (1.0e-05, 1.05e-08)),
    "skip8-7x4x9-N65-faces-off":
        _row((2.0e-05, 7.34e-07), (2.0e-05, 4.33e-07), (2.0e-05, 3.23e-07),
             (5.0e-04, 7.20e-07), (1.0e-05, 2.96e-08)),
    "skip8-2x33x3-N1-uniform":
        _row((2.0e-05, 7.76e-07), (2.0e-05, 1.50e-06), (3.0e-05, 2.95e-06),
             (5.0e-04, 2.54e-06), (1.0e-05, 1.46e-08)),
    "skip8-13x16x11-N65553-uniform-off":
        _row((2.0e-05, 1.47e-06), (2.3e-05, 2.23e-06), (2.0e-05, 1.31e-06),
             (5.0e-04, 1.06e-06), (1.0e-05, 7.92e-08)),
    "skip1-7x4x9-N257-uniform":
        _row((2.0e-05, 5.36e-07), (2.0e-05, 7.60e-07), (2.0e-05, 1.35e-07),
             (5.0e-04, 8.23e-07), (1.0e-05, 3.36e-08)),
    "skip2-7x4x9-N257-uniform":
        _row((2.0e-05, 5.87e-07), (2.0e-05, 7.23e-07), (2.0e-05, 9.11e-08),
             (5.0e-04, 6.56e-07), (1.0e-05, 3.09e-08)),
    "skip5-7x4x9-N257-uniform":
        _row((2.0e-05, 9.64e-07), (2.0e-05, 1.19e-06), (2.0e-05, 5.66e-08),
             (5.0e-04, 6.71e-07), (1.0e-05, 1.59e-08)),
    "pbr-1x6x5-N1-uniform":
        _row((2.0e-05, 1.01e-06), (2.0e-05, 7.05e-07), (2.7e-05, 2.61e-06),
             (5.0e-04, 2.17e-06), (1.0e-05, 3.77e-08), (5.0e-04, 8.25e-07)),
    "pbr-2x33x3-N64-lattice-unit":
        _row((2.0e-05, 9.12e-07), (2.0e-05, 1.36e-06), (2.0e-05, 4.70e-07),
             (5.0e-04, 1.25e-06), (1.0e-05, 2.39e-08), (5.0e-04, 7.72e-07)),
    "pbr-3x3x3-N63-cell":
        _row((2.0e-05, 9.52e-07), (2.0e-05, 7.73e-07), (2.0e-05, 2.93e-07),
             (5.0e-04, 1.51e-06), (1.0e-05, 1.37e-08), (5.0e-04, 5.27e-07)),
    "pbr-7x4x9-N1000-faces-off":
        _row((2.0e-05, 8.60e-07), (2.0e-05, 1.04e-06), (2.0e-05, 7.55e-07),
             (5.0e-04, 9.42e-07), (1.0e-05, 2.03e-08), (5.0e-04, 6.11e-07)),
    "pbr-13x16x11-N65553-uniform-off":
        _row((2.0e-05, 1.32e-06), (2.0e-05, 1.57e-06), (2.0e-05, 1.02e-06),
             (5.0e-04, 1.17e-06), (1.0e-05, 4.34e-08), (5.0e-04, 6.76e-07)),
    "pbr.offset-2x33x3-N65-uniform":
        _row((2.0e-05, 1.13e-06), (2.0e-05, 1.47e-06), (2.0e-05, 2.99e-07),
             (5.0e-04, 1.28e-06), (1.0e-05, 2.00e-08), (5.0e-04, 1.71e-06)),
    "skip8-l1":
        _row((2.0e-05, 1.02e-06), (2.0e-05, 1.14e-06), (2.0e-05, 4.66e-07),
             (5.0e-04, 7.22e-07), (1.0e-05, 1.90e-08)),
    "skip8-weightedl1":
        _row((2.0e-05, 1.40e-06), (2.0e-05, 6.06e-07), (2.0e-05, 3.75e-07),
             (5.0e-04, 7.65e-07), (1.0e-05, 2.93e-08)),
    "skip8-weight0.37-ratio0.5":
        _row((2.0e-05, 1.51e-06), (2.0e-05, 1.06e-06), (2.0e-05, 9.65e-07),
             (5.0e-04, 8.36e-07), (1.0e-05, 3.90e-08)),
    "skip8-renorm":
        _row((2.0e-05, 9.28e-07), (2.0e-05, 6.73e-07), (2.0e-05, 6.36e-07),
             (5.0e-04, 6.96e-07), (1.0e-05, 2.30e-08)),
    "skip8-band-holds-all":
        _row((2.0e-05, 1.41e-06), (2.0e-05, 1.17e-06), (2.0e-05, 6.77e-07),
             (5.0e-04, 7.21e-07), (1.0e-05, 2.33e-08)),
    "skip8-band-holds-one":
        _row((2.0e-05, 9.51e-07), (2.0e-05, 8.71e-07), (2.0e-05, 9.91e-08),
             (5.0e-04, 6.34e-07), (1.0e-05, 2.34e-08)),
    "pbr-l1":
        _row((2.0e-05, 1.19e-06), (2.0e-05, 1.01e-06), (2.0e-05, 7.67e-07),
             (5.0e-04, 1.18e-06), (1.0e-05, 1.79e-08), (5.0e-04, 4.94e-07)),
    "pbr-weightedl1":
        _row((2.0e-05, 1.39e-06), (2.0e-05, 8.58e-07), (2.0e-05, 3.35e-07),
             (5.0e-04, 1.00e-06), (1.0e-05, 1.82e-08), (5.0e-04, 3.74e-07)),
    "pbr-weight0.37-ratio0.5":
        _row((2.0e-05, 9.84e-07), (2.0e-05, 7.41e-07), (2.0e-05, 3.41e-07),
             (5.0e-04, 9.17e-07), (1.0e-05, 4.27e-08), (5.0e-04, 4.39e-07)),
    "pbr-renorm":
        _row((2.0e-05, 1.07e-06), (2.0e-05, 1.09e-06), (2.0e-05, 6.46e-07),
             (5.0e-04, 1.12e-06), (1.0e-05, 1.75e-08), (5.0e-04, 5.29e-07)),
    "pbr-band-holds-all":
        _row((2.0e-05, 1.33e-06), (2.0e-05, 8.01e-07), (2.0e-05, 1.08e-06),
             (5.0e-04, 8.70e-07), (1.0e-05, 2.27e-08), (5.0e-04, 5.82e-07)),
    "pbr-band-holds-one":
        _row((2.0e-05, 1.06e-06), (2.0e-05, 7.68e-07), (2.0e-05, 6.30e-07),
             (5.0e-04, 1.05e-06), (1.0e-05, 1.74e-08), (5.0e-04, 8.03e-07)),
    "geo.skip-l1":
        _row((2.0e-05, 3.41e-07), (2.0e-05, 9.30e-07), (2.0e-05, 6.11e-08),
             (5.0e-04, 5.20e-07), (1.0e-05, 1.85e-08)),
    "geo.skip-weightedl1":
        _row((2.0e-05, 2.27e-07), (2.0e-05, 6.39e-07), (2.0e-05, 3.23e-08),
             (5.0e-04, 5.67e-07), (1.0e-05, 2.38e-08)),
    "geo.skip-renorm":
        _row((2.0e-05, 2.68e-07), (2.0e-05, 6.51e-07), (2.0e-05, 1.22e-07),
             (5.0e-04, 5.51e-07), (1.0e-05, 3.98e-08)),
    "geo.pbr-l1":
        _row((2.0e-05, 3.01e-07), (2.0e-05, 7.00e-07), (2.0e-05, 1.92e-08),
             (5.0e-04, 5.76e-07), (1.0e-05, 2.11e-08)),
    "geo.pbr-weightedl1":
        _row((2.0e-05, 3.91e-07), (2.0e-05, 1.25e-06), (2.0e-05, 9.70e-09),
             (5.0e-04, 4.97e-07), (1.0e-05, 4.14e-08)),
    "geo.pbr-renorm":
        _row((2.0e-05, 3.07e-07), (2.0e-05, 6.96e-07), (2.0e-05, 8.77e-09),
             (5.0e-04, 6.95e-07), (1.0e-05, 3.94e-08)),
    "skip8-band-0.03-0.9":
        _row((2.0e-05, 9.12e-07), (2.0e-05, 4.60e-07), (2.0e-05, 1.51e-07),
             (5.0e-04, 7.64e-07), (1.0e-05, 1.35e-08)),
    "skip8-band-0.15-0.999":
        _row((2.0e-05, 9.88e-07), (2.0e-05, 5.51e-07), (2.0e-05, 1.90e-07),
             (5.0e-04, 7.96e-07), (1.0e-05, 2.21e-08)),
    "pbr-band-0.03-0.9":
        _row((2.0e-05, 1.07e-06), (2.0e-05, 8.84e-07), (2.0e-05, 1.93e-07),
             (5.0e-04, 9.46e-07), (1.0e-05, 1.51e-08), (5.0e-04, 6.56e-07)),
    "pbr-band-0.15-0.999":
        _row((2.0e-05, 1.15e-06), (2.0e-05, 1.05e-06), (2.0e-05, 1.46e-07),
             (5.0e-04, 1.04e-06), (1.0e-05, 1.68e-08), (5.0e-04, 8.25e-07)),
}


def bound_for(quantity, gap):
    """the shared bound wherever ten times the gap is below it, otherwise ten times the gap rounded up to two digits"""
    ten = 10 * gap
    if ten < SHARED[quantity]:
        return SHARED[quantity]
    e = math.floor(math.log10(ten)) - 1
    return float(f"{math.ceil(ten / 10 ** e - 1e-9) * 10 ** e:.1e}")


def decoder_built(case):
    """Whether the inference decoder (s3d_decoder.hip: run_decode) has a compiled k_decode<UPT, HIDT> for the case's widths after
    padding to 32: it has five tile pairs, and refuses every other pair by name.  The training tier takes any multiples of 32."""
    up, hid = CASES[case]["cfg"][2:4]
    return (-(-up // 32), -(-hid // 32)) in {(2, 8), (1, 1), (1, 8), (1, 2), (3, 4)}


def quantities(case):
    c = CASES[case]
    return ("encode", "pred", "loss", "grad", "zero") + (("norm1",) if c["net"] == "pbr" else ())


# ------------------------------------------------------------------------------------------------ inputs
def restated(case):
    """the case as ae_variants_cases / ae_pbr_cases name it: kind and args"""
    c = CASES[case]
    return dict(kind=c["net"], args=c["cfg"], tex_channels=c["tc"])


def shapes(case):
    c = CASES[case]
    geo, tex, up, hid, layers = c["cfg"]
    if c["net"] == "geo":
        return T.geo_only_param_shapes(geo, up, hid, layers, with_encoder=True)
    if c["net"] == "pbr":
        return T.pbr_param_shapes(*c["cfg"], c["tc"], with_encoder=True)
    return T.ae_param_shapes(*c["cfg"], c["tc"], with_encoder=True)


@functools.lru_cache(maxsize=None)
def _inputs(case):
    c = CASES[case]
    sd = T.synthetic_state_dict(shapes(case), c["seed"])
    if c["offset"]:
        sd["tex_convs.0.out_layers.1.bias"] = sd["tex_convs.0.out_layers.1.bias"] + c["offset"]
    import torch
    H, W, D = c["hwd"]
    vol = torch.tanh(torch.from_numpy(T.synthetic_noise((1, 1 + c["tc"], 2 * H, 2 * W, 2 * D), 1200 + c["seed"])))
    vol[:, 1:] = 0.5 * vol[:, 1:] + 0.5
    return sd, vol


def state_dict(case):
    """float32 torch tensors (synthetic, the case's seed; pbr.offset adds its bias offset)"""
    return dict(_inputs(case)[0])


def volume(case):
    """[1, 1 + tex_channels, 2H, 2W, 2D] float32: a tanh-squashed sdf channel, material channels in [0, 1]"""
    return _inputs(case)[1]


def band(case):
    """the float32 bound of the texture band"""
    lo = CASES[case]["loss"]
    return np.float32((1.0 if lo["renorm"] else lo["thr"]) * lo["ratio"])


def _decode(case, sd, pts, fm, taps):
    import torch
    c = CASES[case]
    aabb = torch.tensor(c["aabb"], dtype=pts.dtype)
    if c["net"] == "pbr":
        return P.decode(sd, pts, fm, aabb, c["cfg"][0], taps=taps)
    return V.decode(sd, pts, fm, aabb, c["net"], c["cfg"][0], taps)


@functools.lru_cache(maxsize=None)
def batch(case):
    """Deterministic (pts [N,3], sdf [N,1], tex [N,tc] or None) float32 with every kink at least KINK away in float64.
    all_band: every |sdf| at most half the threshold; one_row: row 0 inside the band and every other row between the band and
    the threshold; band_rows: sdf values pinned into the first rows (kept through redraws: only their points and targets move)."""
    import torch
    c = CASES[case]
    lo, N, tc = c["loss"], c["N"], c["tc"]
    rng = np.random.Generator(np.random.PCG64(100 + c["seed"]))
    thr = lo["thr"]
    draw_pts = _placer(c["place"], c["hwd"], c["aabb"], rng)
    lim = 0.5 * thr if lo.get("all_band") else thr
    scale = 1.0 / thr if lo["renorm"] else 1.0

    def draw_sdf(n):
        if lo.get("one_row"):                                  # the band ends at ratio * thr = 0.999 thr
            s = rng.uniform(0.9995 * thr, thr, size=(n, 1)) * rng.choice([-1.0, 1.0], size=(n, 1))
        else:
            s = np.clip(rng.normal(0, 0.6 * thr, size=(n, 1)), -lim, lim)
        return (s * scale).astype(np.float32)

    pts, sdf = draw_pts(N), draw_sdf(N)
    tex = rng.uniform(0, 1, size=(N, tc)).astype(np.float32)
    pinned = np.zeros(N, bool)
    rows = np.asarray([0.3 * thr * scale], np.float32) if lo.get("one_row") else c["band_rows"]
    if rows is not None:
        sdf[:len(rows), 0] = rows
        pinned[:len(rows)] = True
    sd64 = {k: v.double() for k, v in state_dict(case).items()}
    with torch.no_grad():
        fm64 = V.encode(sd64, volume(case).double(), c["net"])
    todo = np.arange(N)
    for _ in range(40):
        taps = []
        with torch.no_grad():
            pred = _decode(case, sd64, torch.from_numpy(pts[todo]).double(), fm64, taps).numpy()
        m = np.min([t.abs().min(1).values.numpy() for t in taps], axis=0)
        m = np.minimum(m, np.abs(pred[:, 0] - sdf[todo, 0]))
        if lo["sdf_loss"] == "weightedl1":
            m = np.minimum(m, np.abs(sdf[todo, 0]))
        if tc:
            m = np.minimum(m, np.abs(pred[:, 1:] - tex[todo]).min(1))
        bad = todo[m < KINK]
        if not len(bad):
            to = torch.from_numpy
            return to(pts), to(sdf), to(tex) if tc else None
        pts[bad] = draw_pts(len(bad))
        free = bad[~pinned[bad]]
        sdf[free] = draw_sdf(len(free))
        tex[bad] = rng.uniform(0, 1, size=(len(bad), tc)).astype(np.float32)
        todo = bad
    raise RuntimeError(f"{case}: {len(bad)} rows stay within {KINK} of a kink")


def kink_distance(case):
    """the smallest float64 distance of any row of the case's batch to a kink"""
    import torch
    c = CASES[case]
    pts, sdf, tex = batch(case)
    sd64 = {k: v.double() for k, v in state_dict(case).items()}
    taps = []
    with torch.no_grad():
        pred = _decode(case, sd64, pts.double(), V.encode(sd64, volume(case).double(), c["net"]), taps)
    m = min(float(t.abs().min()) for t in taps)
    m = min(m, float((pred[:, :1] - sdf.double()).abs().min()))
    if c["loss"]["sdf_loss"] == "weightedl1":
        m = min(m, float(sdf.abs().min()))
    if tex is not None:
        m = min(m, float((pred[:, 1:] - tex.double()).abs().min()))
    return m


# ------------------------------------------------------------------------------------------------ reference and metrics
def forward_backward(case, dtype, fault=None):
    """the restatement's iteration on the case's batch in `dtype`: (feature maps, pred, losses, {name: gradient})"""
    c = CASES[case]
    lo = c["loss"]
    sd = {k: v.to(dtype) for k, v in state_dict(case).items()}
    pts, sdf, tex = (None if t is None else t.to(dtype) for t in batch(case))
    fn = P.forward_backward if c["net"] == "pbr" else V.forward_backward
    return fn(restated(case), sd, volume(case).to(dtype), pts, sdf, tex, fault=fault, aabb=c["aabb"], thr=lo["thr"], ratio=lo["ratio"],
              tex_weight=lo["tw"], sdf_loss=lo["sdf_loss"], sdf_renorm=lo["renorm"], geo_dim=c["cfg"][0])


@functools.lru_cache(maxsize=None)
def reference(case):
    """float64, computed once per case and shared; do not write to it"""
    import torch
    return forward_backward(case, torch.float64)


def errors(case, fm, pred, losses, grads):
    """Every quantity of one iteration (tensors on the host, any dtype; losses in the reference's order, further entries must
    be zero) against the float64 reference: encode and pred as max-abs over max-abs, losses relative, `grad` the worst
    |got - ref| / max(|ref|, 1e-2 gmax) in L2 over the tensors that are not analytically zero with its name, `zero` the largest
    |got| / gmax over those that are, `norm1` the PBR net's tex_convs.1.norm_* as max-abs over max-abs."""
    from conftest import relerr
    c = CASES[case]
    fm_r, pred_r, loss_r, grad_r = reference(case)
    assert set(grads) == set(grad_r), sorted(set(grads) ^ set(grad_r))
    out = {"encode": max(relerr(f.numpy(), r.numpy()) for f, r in zip(fm, fm_r)), "pred": relerr(pred.numpy(), pred_r.numpy())}
    got = [float(v) for v in losses]
    assert all(v == 0.0 for v in got[len(loss_r):]), got
    out["loss"] = max(abs(a - float(b)) / abs(float(b)) for a, b in zip(got, loss_r.values()))
    gmax = max(float(v.norm()) for v in grad_r.values())
    worst, zero = (0.0, ""), 0.0
    for name, ref in grad_r.items():
        g = grads[name].double()
        if name in ZERO_GRAD[c["net"]]:
            zero = max(zero, float(g.norm()) / gmax)
        else:
            worst = max(worst, (float((g - ref).norm()) / max(float(ref.norm()), 1e-2 * gmax), name))
    out["grad"], out["grad_at"], out["zero"] = worst[0], worst[1], zero
    if c["net"] == "pbr":
        out["norm1"] = max(relerr(grads[k].numpy(), grad_r[k].numpy()) for k in NORM1)
    return out


def float32_gap(case, fault=None):
    """the float32 restatement (optionally with a fault) against the float64 reference"""
    import torch
    fm, pred, ls, grads = forward_backward(case, torch.float32, fault)
    return errors(case, fm, pred, list(ls.values()), grads)


# ------------------------------------------------------------------------------------------------ the device
def network(case, tmp_path=None):
    """The case's network on the device with its weights: constructed directly, or, with a directory, inside a ShapeAutoEncoder
    built from the command line's strings (-> (net, ae))."""
    import torch
    from types import SimpleNamespace
    from sin3dm_amd.encoding.model import ShapeAutoEncoder
    from sin3dm_amd.encoding.networks import AutoEncoderGroupPBR, AutoEncoderGroupSkip
    c = CASES[case]
    lo, ae = c["loss"], None
    if tmp_path is None:
        cls = AutoEncoderGroupPBR if c["enc"] == "pbr" else AutoEncoderGroupSkip
        net = cls(*c["cfg"], use_tex=c["net"] != "geo", tex_channels=max(c["tc"], 1)).to(torch.device("cuda:0"))
        net.build_training_tier(material_heads=c["net"] == "pbr")
    else:
        assert c["tc"] in (0, 8)
        geo, tex, up, hid, layers = c["cfg"]
        ns = SimpleNamespace(enc_net_type=c["enc"], fdim_geo=geo, fdim_tex=tex, fdim_up=up, hidden_dim=hid, n_hidden_layers=layers,
                             data_type="sdf" if c["net"] == "geo" else "sdfpbr", sdf_loss=lo["sdf_loss"], tex_loss="l1",
                             tex_weight=lo["tw"], tex_threshold_ratio=lo["ratio"], sdf_renorm=int(lo["renorm"]), enc_lr=1e-3,
                             enc_lr_split=0.2, enc_lr_decay=0.1, enc_n_iters=10, gpu_id=0)
        ae = ShapeAutoEncoder(str(tmp_path), ns)
        ae._build_tier()
        ae.sdf_threshold = lo["thr"]
        net = ae.net
    assert net.variant == {"geo": 1, "skip": 0, "pbr": 2}[c["net"]]
    missing, unexpected = net.load_state_dict(state_dict(case), strict=False)
    assert not unexpected and missing == ["aabb"]
    return net, ae


def device_run(case, net, ae=None):
    """One case on the device, as tests/test_hip_ae_reference.py:_check runs it: a larger batch first (stale workspace where this
    batch's padded rows land), encode, net(vol, pts) against net.decode(pts, fm), loss_and_grads with pred, and the same call
    again.  With `ae`, ShapeAutoEncoder.train_step on the same batch afterwards.  Returns the errors of errors() plus `decode`
    and the exact-equality findings, which the caller asserts."""
    import torch
    from conftest import relerr
    from sin3dm_amd.encoding.model import ae_loss_cfg
    c = CASES[case]
    lo = c["loss"]
    dev = torch.device("cuda:0")
    pts, sdf, tex = batch(case)
    vol_c, pts_c, sdf_c = volume(case).to(dev), pts.to(dev), sdf.to(dev)
    tex_c = None if tex is None else tex.to(dev)
    net.reset_aabb(torch.tensor(c["aabb"], dtype=torch.float32, device=dev))
    lc = ae_loss_cfg(lo["sdf_loss"], "l1", lo["thr"], lo["ratio"], lo["tw"], lo["renorm"])
    big = torch.arange(2 * len(pts) + 64, device=dev) % len(pts)
    net.loss_and_grads(vol_c, pts_c[big], sdf_c[big], None if tex_c is None else tex_c[big], lc)
    fm = net.encode(vol_c)
    pred = net(vol_c, pts_c)
    dec, refused = None, None
    try:
        dec = net.decode(pts_c, fm)
    except NotImplementedError as e:                             # the caller asserts that this is decoder_built()'s answer
        refused = str(e)
    losses, pred2, g = net.loss_and_grads(vol_c, pts_c, sdf_c, tex_c, lc, want_pred=True)
    losses, g = losses.clone(), g.clone()
    losses2, _, g2 = net.loss_and_grads(vol_c, pts_c, sdf_c, tex_c, lc)
    out = errors(case, [f.cpu() for f in fm], pred.cpu(), losses.cpu().tolist(), {k: v.cpu() for k, v in net.split_flat(g).items()})
    out["decode"] = None if dec is None else relerr(dec.cpu().numpy(), reference(case)[1].numpy())
    out["decode_refused"] = refused
    out["losses"] = losses.cpu().tolist()
    out["finite"] = bool(torch.isfinite(g).all())
    out["pred_same"] = torch.equal(pred2, pred)
    out["again_same"] = torch.equal(losses, losses2) and torch.equal(g, g2)
    if ae is not None:
        ae.input_grid, ae.aabb = vol_c, torch.tensor(c["aabb"], dtype=torch.float32, device=dev)
        net.reset_aabb(ae.aabb)
        ae._set_optimizer(ae.init_lr, ae.min_lr_ratio)
        data = {"pts": pts_c, "sdf": sdf_c}
        if tex_c is not None:
            data["tex"] = tex_c
        step = ae.train_step(data)
        assert tuple(step) == net.loss_names
        out["train_step_same"] = all(torch.equal(step[k], losses[i]) for i, k in enumerate(net.loss_names)) and torch.equal(ae._grad, g)
    return out
