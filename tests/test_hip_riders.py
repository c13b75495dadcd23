"""Riders: in the inference forward of the virtual-concat path three small GroupNorm launches run in the first blocks of a 1x1
convolution that neither feeds nor needs them (Fwd::resblock / Fwd::resblock_cat, k_conv_mfma<CFG, true>): k_gn_partials_up in W_a's
launch, k_gn_finalize_cat in W_b's, the k_gn_finalize behind the pooling in the down block's skip_connection.  The bodies are the
kernels' own (s3d_riders.h), so s3d_set_riders(0) — every stage a launch of its own — must give the same bits, and so must the forms
that cannot carry a rider and launch everything alone."""
import numpy as np
import pytest
import torch

from sin3dm_amd import _lib, testing as T

pytestmark = pytest.mark.gpu

RIDER_NAMES = ("carrying k_gn_partials_up", "carrying k_gn_finalize_cat", "carrying k_gn_finalize (plain)")


def _model(mc):
    from sin3dm_amd.diffusion.unet_triplane import TriplaneUNetModelSmall
    m = TriplaneUNetModelSmall(12, mc, 12, channel_mult=(1, 2), use_scale_shift_norm=True)
    m.load_state_dict(T.synthetic_state_dict(T.unet_param_shapes(model_channels=mc, channel_mult=(1, 2)), 0))
    return m.to(torch.device("cuda:0")).eval()


def _forward(model, hwd, B, options, riders=True):
    """(output, names of the kernels the 1x1 launches dispatched) of two equal forwards under `options`, riders on or off."""
    H, W, D = hwd
    dev = torch.device("cuda:0")
    x = torch.from_numpy(T.synthetic_noise((B, 12, H + D, W + D), 31)).to(dev)
    t = torch.arange(B, device=dev, dtype=torch.float32) * 37.0 + 5.0
    try:
        for k, v in options.items():
            _lib.set_option(k, v)
        _lib.set_riders(riders)
        model.profile(1, classes=2)
        with torch.no_grad():
            y = model(x, t, H=H, W=W, D=D).clone()
            y2 = model(x, t, H=H, W=W, D=D)
        model.profile_read()
        assert torch.equal(y, y2), "the second forward gives other bits"
        return y.cpu().numpy(), model.profile_kernel(1)
    finally:
        _lib.set_riders(True)
        for k in options:
            _lib.set_option(k, None)


@pytest.mark.parametrize("mc", [32, 128])
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("hwd", [(16, 16, 16), (24, 16, 8)], ids=lambda s: "x".join(map(str, s)))
def test_riders_give_the_bits_of_separate_launches(hwd, B, mc):
    """Riders on (the default) against off on fresh handles: all three pairs ride (the library names them), none does when off, and
    the UNet output is the same bit for bit.  (16,16,16): whole 8x8 tiles on the half-resolution planes; (24,16,8): planes of
    12x8, 12x4 and 8x4 there — ragged tiles in the rider that reads u, and fewer convolution blocks than rider blocks."""
    y, names = _forward(_model(mc), hwd, B, {})
    for n in RIDER_NAMES:
        assert n in names, (n, names)
    y0, names0 = _forward(_model(mc), hwd, B, {}, riders=False)
    assert "carrying" not in names0 and "k_conv_mfma<1x1>" in names0, names0
    assert np.array_equal(y, y0), float(np.abs(y - y0).max())


def test_forms_that_cannot_carry_a_rider_launch_alone():
    """CONV1X1_T=1 (the transposed 1x1 epilogue, bit-identical to the default) carries nothing and equals the default bits;
    VCAT=0 (the materialised concat: other rounding, no virtual-concat path) carries nothing with riders on or off and gives
    the same bits both ways."""
    hwd, B, mc = (24, 16, 8), 2, 32
    y, names = _forward(_model(mc), hwd, B, {})
    assert all(n in names for n in RIDER_NAMES), names
    yt, names_t = _forward(_model(mc), hwd, B, {"CONV1X1_T": 1})
    assert "carrying" not in names_t and "transposed accumulators" in names_t, names_t
    assert np.array_equal(y, yt)
    yv, names_v = _forward(_model(mc), hwd, B, {"VCAT": 0})
    yv0, names_v0 = _forward(_model(mc), hwd, B, {"VCAT": 0}, riders=False)
    assert "carrying" not in names_v and "carrying" not in names_v0, (names_v, names_v0)
    assert np.array_equal(yv, yv0)


def test_switching_riders_on_a_live_handle():
    """One handle, the switch moved between launches (the arena layout does not depend on it)."""
    hwd, B = (16, 16, 16), 1
    m = _model(128)
    a, na = _forward(m, hwd, B, {})
    b, nb = _forward(m, hwd, B, {}, riders=False)
    c, _ = _forward(m, hwd, B, {})
    assert "carrying" in na and "carrying" not in nb and np.array_equal(a, b) and np.array_equal(a, c)
