"""The auto-encoder training tier's network variants without a GPU: the parameter manifest behind s3d_ae_create_variant, the
configurations it refuses, the two decisions where the reference does not work, and a float64 restatement
(tests/ae_variants_cases.py) that reproduces tests/golden/ae_variants.npz and, with one deliberate mistake injected, leaves the
bounds tests/test_ae_variants_gpu.py holds the device to."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

import ae_variants_cases as V
from conftest import digest_errors, golden, relerr
from sin3dm_amd import _lib, testing as T


def _create(variant, cfg):
    lib = _lib.load()
    h = C.c_void_p()
    rc = lib.s3d_ae_create_variant(C.byref(_lib.DecoderCfg(*cfg)), variant, C.byref(h))
    return lib, rc, h


@pytest.mark.parametrize("variant, cfg, shapes", [
    (0, (4, 8, 64, 256, 4, 3), T.ae_param_shapes(4, 8, 64, 256, 4, 3, with_encoder=True)),
    (0, (4, 8, 64, 256, 4, 8), T.ae_param_shapes(4, 8, 64, 256, 4, 8, with_encoder=True)),
    (0, (4, 8, 32, 64, 4, 8), T.ae_param_shapes(4, 8, 32, 64, 4, 8, with_encoder=True)),
    (1, (4, 8, 64, 256, 4, 3), T.geo_only_param_shapes(4, 64, 256, 4, with_encoder=True)),
    (1, (8, 0, 32, 64, 4, 0), T.geo_only_param_shapes(8, 32, 64, 4, with_encoder=True)),        # variant 1 ignores tex_*
], ids=["skip3", "skip8", "skip8.narrow", "geo", "geo.8"])
def test_param_manifest(variant, cfg, shapes):
    """names, shapes, offsets and the group split of the flat vector equal the testing.* manifest with the encoders"""
    lib, rc, h = _create(variant, cfg)
    assert rc == 0, _lib.last_error()
    try:
        assert lib.s3d_ae_out_channels(h) == (1 if variant == 1 else 1 + cfg[5])
        got, off_expect = [], 0
        for i in range(lib.s3d_ae_num_params(h)):
            name, shape, nd, off = C.c_char_p(), (C.c_int64 * 5)(), C.c_int(), C.c_int64()
            _lib.check(lib.s3d_ae_param_info(h, i, C.byref(name), shape, C.byref(nd), C.byref(off)))
            shp = tuple(shape[k] for k in range(nd.value))
            assert off.value == off_expect, name.value
            off_expect += int(np.prod(shp))
            got.append((name.value.decode(), shp))
        # the flat vector keeps the geo group first (encoder, convs, decoder), then the tex group
        want = [(k, tuple(v)) for k, v in shapes.items() if k.startswith("geo_")] + \
               [(k, tuple(v)) for k, v in shapes.items() if not k.startswith("geo_")]
        assert got == want
        tb = C.c_int64()
        assert lib.s3d_ae_param_numel(h, C.byref(tb)) == off_expect
        assert tb.value == sum(int(np.prod(v)) for k, v in shapes.items() if k.startswith("geo_"))
        if variant == 1:
            assert tb.value == off_expect                        # no tex group
    finally:
        lib.s3d_ae_destroy(h)


@pytest.mark.parametrize("variant, cfg", [
    (2, (4, 8, 64, 256, 4, 3)),           # the PBR net has 8 material channels
    (2, (4, 8, 64, 256, 4, 8)),           # and its training tier is not built
    (0, (4, 8, 64, 256, 4, 9)),           # 9 texture channels
    (0, (4, 8, 48, 256, 4, 8)),           # up not a multiple of 32
    (1, (4, 8, 48, 256, 4, 3)),
    (0, (4, 12, 64, 256, 4, 8)),          # more than 12 feature channels
    (0, (4, 8, 64, 256, 2, 8)),           # mlp_hidden_layers != 4
], ids=["pbr.tc3", "pbr", "tc9", "up48", "geo.up48", "feat16", "layers2"])
def test_unsupported_configurations_are_refused(variant, cfg):
    lib, rc, h = _create(variant, cfg)
    assert rc == _lib.ERR_UNSUPPORTED and not h.value, (rc, _lib.last_error())


def _cfg(**kw):
    base = dict(enc_net_type="skip", fdim_geo=4, fdim_tex=8, fdim_up=64, hidden_dim=256, n_hidden_layers=4, data_type="sdftex",
                tex_loss="l1", gpu_id=0)
    base.update(kw)
    return SimpleNamespace(**base)


@pytest.mark.parametrize("tex_loss", ["l2", "huber"])
def test_sdfpbr_refuses_a_loss_the_reference_leaves_undefined(tmp_path, tex_loss):
    """the reference trains sdfpbr with --tex_loss l2 | huber without any material loss (model.py:226-233 defines l1 only)"""
    import torch
    from sin3dm_amd.encoding.model import ShapeAutoEncoder
    with pytest.raises(ValueError, match="sdfpbr"):
        ShapeAutoEncoder(str(tmp_path), _cfg(data_type="sdfpbr", tex_loss=tex_loss), device=torch.device("cpu"))
    ShapeAutoEncoder(str(tmp_path), _cfg(data_type="sdftex", tex_loss=tex_loss), device=torch.device("cpu"))
    ae = ShapeAutoEncoder(str(tmp_path), _cfg(data_type="sdfpbr"), device=torch.device("cpu"))
    assert ae.net.loss_names == ("sdf_loss", "rgb_loss", "mr_loss", "normal_loss")
    geo = ShapeAutoEncoder(str(tmp_path), _cfg(data_type="sdf"), device=torch.device("cpu"))
    assert geo.net.loss_names == ("sdf_loss",) and geo.net.out_channels == 1


def test_the_training_tier_is_switched_on_explicitly():
    """a network as constructed keeps its earlier contract (tests/test_pbr_host.py: decode only, and it says so); build_training_tier(),
    which ShapeAutoEncoder calls before it loads training data, switches the tier on — except for the PBR net with texture"""
    from sin3dm_amd.encoding.networks import AutoEncoderGroupPBR, AutoEncoderGroupSkip
    assert AutoEncoderGroupSkip(4, 8, 64, 256, 4).training_tier_built                     # sdftex: from construction, as before
    for net in (AutoEncoderGroupSkip(4, 8, 64, 256, 4, use_tex=False), AutoEncoderGroupPBR(4, 8, 64, 256, 4, use_tex=False),
                AutoEncoderGroupSkip(4, 8, 64, 256, 4, tex_channels=8)):
        assert not net.training_tier_built
        with pytest.raises(NotImplementedError, match="build_training_tier"):
            net.flat_parameters
        assert net.build_training_tier() is net and net.training_tier_built
    pbr = AutoEncoderGroupPBR(4, 8, 64, 256, 4, tex_channels=8)
    with pytest.raises(NotImplementedError, match="not built"):
        pbr.build_training_tier()
    assert not pbr.training_tier_built


@pytest.mark.parametrize("split, rates", [(0.2, [1e-3]), (-1.0, [5e-3])])
def test_optimizer_groups_of_the_geometry_only_net(split, rates):
    """sdf has no tex group (the reference crashes in tex_parameters() with lr_split > 0): one group at the geometry group's rate"""
    import torch
    from sin3dm_amd.encoding.model import FlatGroupAdamW
    net = SimpleNamespace(flat_parameters=torch.zeros(100), tex_group_begin=100)
    opt = FlatGroupAdamW(net, 5e-3, split)
    assert opt.ranges == ((0, 100),) and opt.lrs == pytest.approx(rates)
    two = FlatGroupAdamW(SimpleNamespace(flat_parameters=torch.zeros(100), tex_group_begin=40), 5e-3, 0.2)
    assert two.ranges == ((0, 40), (40, 100)) and two.lrs == pytest.approx([1e-3, 5e-3])


# ------------------------------------------------------------------------------------------------ restatement
_cache = {}


def _restated(case, fault=None):
    """the float64 restatement's iteration on the fixture's batch, computed once per (case, fault)"""
    import torch
    if (case, fault) not in _cache:
        g = golden("ae_variants")
        sd = {k: v.double() for k, v in T.synthetic_state_dict(V.shapes(case), V.SEED_WEIGHTS).items()}
        pts, sdf, tex = (None if a is None else torch.from_numpy(a).double() for a in V.batch(case, int(g[f"{case}.seed"])))
        torch.set_num_threads(4)
        _cache[(case, fault)] = V.forward_backward(case, sd, torch.from_numpy(V.volume(case)).double(), pts, sdf, tex, fault=fault)
    return _cache[(case, fault)]


def _errors(case, result):
    g = golden("ae_variants")
    fm, pred, ls, grads = result
    w = digest_errors({k: v.numpy() for k, v in grads.items()}, g, f"{case}.grad")
    return {"encode": max(relerr(f.numpy(), g[f"{case}.{k}"]) for f, k in zip(fm, V.PLANES)),
            "pred": relerr(pred.numpy(), g[f"{case}.pred"]),
            "loss": float(np.max(np.abs(np.asarray([float(ls[k]) for k in V.loss_names(case)]) - g[f"{case}.losses"]))),
            "grad.norm": w["norm"], "grad.proj": w["proj"], "grad.full": w["full"]}


@pytest.mark.parametrize("case", list(V.CASES))
def test_restatement_reproduces_the_fixture(case):
    err = _errors(case, _restated(case))
    g = golden("ae_variants")
    for k, v in err.items():
        # float64 against the reference's float32: its recorded float32-versus-float64 gap, with room for another summation order
        assert v <= 2 * float(g[f"{case}.gap.{k}"]) + 1e-7, (k, v, float(g[f"{case}.gap.{k}"]))
        assert v < 0.1 * V.BOUNDS[k], (k, v)


def test_one_mean_over_eight_columns_leaves_the_bounds():
    """injected fault: the sdfpbr material loss as ONE l1 mean over the eight columns.  The sum of the three group means is not
    the one mean, and the groups' gradients come out scaled 3/8 : 2/8 : 3/8 of what they are — the bounds of the GPU test see both"""
    err = _errors("skip8", _restated("skip8", fault="one_mean"))
    assert err["loss"] > 100 * V.BOUNDS["loss"], err
    assert err["grad.norm"] > 100 * V.BOUNDS["grad.norm"] and err["grad.proj"] > 10 * V.BOUNDS["grad.proj"], err
    assert err["encode"] < V.BOUNDS["encode"] and err["pred"] < V.BOUNDS["pred"], err      # the forward pass is untouched
