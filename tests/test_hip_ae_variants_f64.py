"""The auto-encoder training step (s3d_ae.hip, s3d_ae_kernels.hip) of the geometry-only net, the skip net with 8 material
channels and its three grouped losses, the skip net at texture widths 1, 2 and 5, and the PBR net with its second 3x3 block and
three heads, against float64 autograd of the restatement (tests/ae_variants_cases.py, tests/ae_pbr_cases.py) over the grid of
tests/ae_f64_cases.py: planes at and below the 3x3 and 5x5 blocks' reach, 1 to 65 553 points, points outside the box, on its
faces, on texel centres and edges and all in one cell, off-centre boxes, every loss mode, bands that hold every row and exactly
one, and rows one ulp either side of the band.

Each case runs as tests/test_hip_ae_reference.py:_check does (a larger batch first, encode, the training forward against the
inference decoder, losses and every gradient tensor, the same bits on a second call), with the bounds of ae_f64_cases.BOUNDS,
each of which stands beside the float32 gap it comes from.  One PBR case has widths (64, 128), which the training tier takes and
the inference decoder has no compiled tile pair for: there `net.decode` must refuse by name, and `net(vol, pts)` alone is held to
float64.  The CPU half, with the injected faults, is
tests/test_ae_variants_f64_host.py; the figures are in profiles/ae_variants_f64.txt."""
import pytest

import ae_f64_cases as A

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _threads():
    import torch
    n = torch.get_num_threads()
    torch.set_num_threads(min(16, n))
    yield
    torch.set_num_threads(n)


def _check(case, record, tmp_path=None):
    net, ae = A.network(case, tmp_path)
    e = A.device_run(case, net, ae)
    B = {q: b for q, (b, _) in A.BOUNDS[case].items()}
    record("errors", {k: e[k] for k in A.quantities(case) + ("decode", "grad_at", "losses")})
    print(case, " ".join(f"{q} {e[q]:.2e} ({B[q]:.1e})" for q in A.quantities(case)), "decode", "refused" if e["decode"] is None else f"{e['decode']:.2e}", e["grad_at"])
    assert e["finite"]
    assert e["encode"] < B["encode"], e["encode"]
    assert e["pred"] < B["pred"], e["pred"]
    if A.decoder_built(case):
        assert e["decode"] is not None and e["decode"] < B["pred"], (e["decode"], e["decode_refused"])
    else:       # widths the training tier takes and the inference decoder has no tile pair for: refused by name, never computed
        up, hid = A.CASES[case]["cfg"][2:4]
        assert e["decode"] is None and "no compiled kernel" in e["decode_refused"], e["decode_refused"]
        assert f"feat_channel_up={up}" in e["decode_refused"] and f"mlp_hidden_channels={hid}" in e["decode_refused"]
    assert e["pred_same"]                                        # loss_and_grads(want_pred=True) returns net(vol, pts)'s bits
    assert e["loss"] < B["loss"], (e["loss"], e["losses"])
    assert e["grad"] < B["grad"], (e["grad"], e["grad_at"])
    assert e["zero"] < B["zero"], e["zero"]
    if "norm1" in B:                                             # tex_convs.1's twice-used norm on its own
        assert e["norm1"] < B["norm1"], e["norm1"]
    assert e["again_same"]                                       # fixed reduction orders: the same bits again
    if ae is not None:
        assert e["train_step_same"]                              # ShapeAutoEncoder.train_step gives the direct call's bits


@pytest.mark.parametrize("case", list(A.SHAPES))
def test_shapes_configs_points(case, record_property):
    _check(case, record_property)


@pytest.mark.parametrize("case", list(A.MODES))
def test_loss_modes(case, tmp_path, record_property):
    """through ShapeAutoEncoder's string-to-mode map: data_type sdf on --enc_net_type skip and pbr, sdfpbr on both"""
    _check(case, record_property, tmp_path)


@pytest.mark.parametrize("case", list(A.BAND))
def test_band_boundary_rows(case, tmp_path, record_property):
    """Rows with |sdf| at fl32(thr * ratio), one ulp either side, and at the product of the two rounded factors: the three group
    losses and their gradients take exactly the rows of the float32 test (tests/test_ae_variants_f64_host.py shows that two rows
    more leave the bounds)."""
    _check(case, record_property, tmp_path)
