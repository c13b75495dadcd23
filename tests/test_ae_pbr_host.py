"""CPU-only checks of the PBR network's auto-encoder training tier (s3d_ae_create_pbr): the flat-vector manifest of the library,
what it refuses, the Python opt-in and parameter groups, and the float64 restatement of tests/ae_pbr_cases.py against the vectors
captured from the reference (tests/golden/ae_pbr.npz) — with each of the injected faults shown to leave the bounds that
tests/test_ae_pbr_gpu.py holds the device to."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

import ae_pbr_cases as P
from conftest import digest_errors, golden, relerr
from sin3dm_amd import _lib, testing as T

ITER_KEYS = ("encode", "pred", "loss", "grad.norm", "grad.proj", "grad.full")


def _create(cfg):
    lib = _lib.load()
    h = C.c_void_p()
    rc = lib.s3d_ae_create_pbr(C.byref(_lib.DecoderCfg(*cfg)), C.byref(h))
    return lib, rc, h


# ------------------------------------------------------------------------------------------------ ABI
@pytest.mark.parametrize("cfg", [(4, 8, 64, 256, 4, 8), (4, 8, 32, 64, 4, 8), (8, 4, 64, 128, 4, 8)], ids=["pbr", "pbr.narrow", "geo8.tex4"])
def test_param_manifest(cfg):
    """names, shapes and running offsets equal testing.pbr_param_shapes with the encoders: the geo group, then tex_encoder,
    tex_convs.0, tex_convs.1 (in_layers.1, no shortcut), rgb, mr and normal heads; tex_group_begin is tex_encoder's first element"""
    shapes = T.pbr_param_shapes(*cfg, with_encoder=True)
    lib, rc, h = _create(cfg)
    assert rc == 0, _lib.last_error()
    try:
        assert lib.s3d_ae_out_channels(h) == 9
        got, offs, off_expect = [], {}, 0
        for i in range(lib.s3d_ae_num_params(h)):
            name, shape, nd, off = C.c_char_p(), (C.c_int64 * 5)(), C.c_int(), C.c_int64()
            _lib.check(lib.s3d_ae_param_info(h, i, C.byref(name), shape, C.byref(nd), C.byref(off)))
            shp = tuple(shape[k] for k in range(nd.value))
            assert off.value == off_expect, name.value
            offs[name.value.decode()] = off.value
            off_expect += int(np.prod(shp))
            got.append((name.value.decode(), shp))
        want = [(k, tuple(v)) for k, v in shapes.items() if k.startswith("geo_")] + \
               [(k, tuple(v)) for k, v in shapes.items() if not k.startswith("geo_")]
        assert got == want
        names = [k for k, _ in got]
        assert "tex_convs.1.in_layers.1.weight" in names and not any(k.startswith("tex_convs.1.shortcut") for k in names)
        tb = C.c_int64()
        assert lib.s3d_ae_param_numel(h, C.byref(tb)) == off_expect
        assert tb.value == offs["tex_encoder.weight"] == sum(int(np.prod(v)) for k, v in shapes.items() if k.startswith("geo_"))
    finally:
        lib.s3d_ae_destroy(h)


@pytest.mark.parametrize("cfg, figures", [
    ((4, 8, 64, 256, 4, 3), ("3",)),              # the PBR net has 8 material channels
    ((4, 8, 48, 256, 4, 8), ("48",)),             # up not a multiple of 32
    ((4, 8, 64, 200, 4, 8), ("200",)),            # hidden width not a multiple of 32
    ((4, 8, 64, 256, 2, 8), ("2",)),              # mlp_hidden_layers != 4
    ((4, 6, 64, 256, 4, 8), ("6",)),              # a feature group that is no multiple of 4
    ((4, 12, 64, 256, 4, 8), ("12",)),            # more than 12 feature channels together
], ids=["tc3", "up48", "hid200", "layers2", "tex6", "feat16"])
def test_unsupported_configurations_are_refused(cfg, figures):
    lib, rc, h = _create(cfg)
    assert rc == _lib.ERR_UNSUPPORTED and not h.value, (rc, _lib.last_error())
    assert all(f in _lib.last_error() for f in figures), _lib.last_error()


def test_the_variant_constructor_names_the_new_call():
    lib = _lib.load()
    h = C.c_void_p()
    rc = lib.s3d_ae_create_variant(C.byref(_lib.DecoderCfg(4, 8, 64, 256, 4, 8)), 2, C.byref(h))
    assert rc == _lib.ERR_UNSUPPORTED and not h.value and "s3d_ae_create_pbr" in _lib.last_error()


# ------------------------------------------------------------------------------------------------ Python
def test_the_opt_in_switches_the_tier_on():
    from sin3dm_amd.encoding.networks import AutoEncoderGroupPBR, AutoEncoderGroupSkip
    net = AutoEncoderGroupPBR(4, 8, 64, 256, 4, tex_channels=8)
    assert not net.training_tier_built
    with pytest.raises(NotImplementedError, match="not built"):
        net.build_training_tier()
    assert not net.training_tier_built
    assert net.build_training_tier(material_heads=True) is net and net.training_tier_built
    assert net.loss_names == P.LOSS_NAMES and net.out_channels == 9
    with pytest.raises(ValueError, match="material_heads"):
        AutoEncoderGroupSkip(4, 8, 64, 256, 4, tex_channels=8).build_training_tier(material_heads=True)


def test_tex_parameters_cover_the_flat_tex_group():
    """the names of tex_parameters() are exactly the manifest's entries from tex_group_begin on (reference :260-262); the
    state_dict keeps the reference's names"""
    from sin3dm_amd.encoding.networks import AutoEncoderGroupPBR
    cfg = (4, 8, 64, 256, 4, 8)
    net = AutoEncoderGroupPBR(*cfg[:5], tex_channels=8)
    shapes = T.pbr_param_shapes(*cfg, with_encoder=True)
    assert {k: tuple(v.shape) for k, v in net.state_dict().items() if k != "aabb"} == {k: tuple(v) for k, v in shapes.items()}
    lib, rc, h = _create(cfg)
    assert rc == 0
    try:
        tb = C.c_int64()
        total = lib.s3d_ae_param_numel(h, C.byref(tb))
        tex_names = []
        for i in range(lib.s3d_ae_num_params(h)):
            name, off = C.c_char_p(), C.c_int64()
            _lib.check(lib.s3d_ae_param_info(h, i, C.byref(name), None, None, C.byref(off)))
            if off.value >= tb.value:
                tex_names.append(name.value.decode())
    finally:
        lib.s3d_ae_destroy(h)
    ids = {id(p) for p in net.tex_parameters()}
    assert sorted(tex_names) == sorted(n for n, p in net.named_parameters() if id(p) in ids)
    assert sum(p.numel() for p in net.tex_parameters()) == total - tb.value
    assert sum(p.numel() for p in net.geo_parameters()) == tb.value
    assert all(n.startswith(("tex_encoder", "tex_convs.0", "tex_convs.1", "rgb_decoder", "mr_decoder", "normal_decoder")) for n in tex_names)


def test_optimizer_has_two_ranges():
    import torch
    from sin3dm_amd.encoding.model import FlatGroupAdamW
    shapes = T.pbr_param_shapes(4, 8, 64, 256, 4, 8, with_encoder=True)
    total = sum(int(np.prod(v)) for v in shapes.values())
    tb = sum(int(np.prod(v)) for k, v in shapes.items() if k.startswith("geo_"))
    opt = FlatGroupAdamW(SimpleNamespace(flat_parameters=torch.zeros(total), tex_group_begin=tb), 5e-3, 0.2)
    assert opt.ranges == ((0, tb), (tb, total)) and opt.lrs == pytest.approx([1e-3, 5e-3])


@pytest.mark.parametrize("tex_loss", ["l2", "huber"])
def test_sdfpbr_on_the_pbr_net_refuses_l2_and_huber(tmp_path, tex_loss):
    import torch
    from sin3dm_amd.encoding.model import ShapeAutoEncoder
    cfg = SimpleNamespace(enc_net_type="pbr", fdim_geo=4, fdim_tex=8, fdim_up=64, hidden_dim=256, n_hidden_layers=4,
                          data_type="sdfpbr", tex_loss=tex_loss, gpu_id=0)
    with pytest.raises(ValueError, match="sdfpbr"):
        ShapeAutoEncoder(str(tmp_path), cfg, device=torch.device("cpu"))


# ------------------------------------------------------------------------------------------------ restatement
_cache = {}


def _restated(case, fault=None):
    """the float64 restatement's iteration on the fixture's batch, computed once per (case, fault)"""
    import torch
    if (case, fault) not in _cache:
        g = golden("ae_pbr")
        sd = {k: v.double() for k, v in P.state_dict(case).items()}
        pts, sdf, tex = (torch.from_numpy(a).double() for a in P.batch(case, int(g[f"{case}.seed"])))
        torch.set_num_threads(4)
        _cache[(case, fault)] = P.forward_backward(case, sd, torch.from_numpy(P.volume(case)).double(), pts, sdf, tex, fault=fault)
    return _cache[(case, fault)]


def _errors(case, result):
    g = golden("ae_pbr")
    fm, pred, ls, grads = result
    w = digest_errors({k: v.numpy() for k, v in grads.items()}, g, f"{case}.grad")
    return {"encode": max(relerr(f.numpy(), g[f"{case}.{k}"]) for f, k in zip(fm, P.PLANES)),
            "pred": relerr(pred.numpy(), g[f"{case}.pred"]),
            "loss": float(np.max(np.abs(np.asarray([float(ls[k]) for k in P.LOSS_NAMES]) - g[f"{case}.losses"]))),
            "grad.norm": w["norm"], "grad.proj": w["proj"], "grad.full": w["full"]}


def test_the_bounds_follow_the_rule():
    """per quantity the shared bound of ae_variants_cases.BOUNDS wherever ten times the fixture's gap stays under it, otherwise
    ten times the gap (rounded up to two digits)"""
    import ae_variants_cases as V
    g = golden("ae_pbr")
    for case, table in P.BOUNDS.items():
        assert set(table) == set(V.BOUNDS)
        for k, b in table.items():
            ten = 10 * float(g[f"{case}.gap.{k}"])
            if ten < V.BOUNDS[k]:
                assert b == V.BOUNDS[k], (case, k, b, ten)
            else:
                assert ten <= b <= 1.02 * ten, (case, k, b, ten)
        assert 10 * float(g[f"{case}.gap.steps.loss"]) < P.STEPS_LOSS


@pytest.mark.parametrize("case", list(P.CASES))
def test_restatement_reproduces_the_fixture(case):
    err = _errors(case, _restated(case))
    g = golden("ae_pbr")
    print(case, " ".join(f"{k} {v:.2e}" for k, v in err.items()))
    for k, v in err.items():
        assert v < P.BOUNDS[case][k], (k, v)
        # float64 against the reference's float32: its recorded float32-versus-float64 gap, with room for another summation order
        assert v <= 2 * float(g[f"{case}.gap.{k}"]) + 1e-7, (k, v, float(g[f"{case}.gap.{k}"]))


@pytest.mark.parametrize("fault", P.FAULTS)
def test_each_fault_leaves_the_bounds(fault):
    """every injected mistake, alone, breaks at least one bound of the GPU test by a wide margin (case pbr)"""
    err = _errors("pbr", _restated("pbr", fault=fault))
    over = {k: v / P.BOUNDS["pbr"][k] for k, v in err.items()}
    print(fault, " ".join(f"{k} {v:.2e} ({over[k]:.0f}x)" for k, v in err.items()))
    assert max(over.values()) > 10, (fault, err)
    if fault in ("residual_f0", "norm0_on_input", "sigmoid"):
        assert over["pred"] > 10, (fault, err)                    # forward mistakes show in pred already
    else:
        assert over["pred"] < 1 and max(over["grad.norm"], over["grad.proj"], over["grad.full"]) > 10, (fault, err)
