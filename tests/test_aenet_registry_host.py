"""CPU-only: the parameter registries of the auto-encoder's two handles (s3d_decoder, s3d_ae) over a grid of configurations, and
every refusal of their constructors, of set_param (unet, decoder) and of param_info (unet, decoder, ae) as literal tables.

A constructor that accepts a configuration must list exactly the parameters of the testing.* manifest (which restates the
reference constructors, independently of the library): names, shapes, order; on the ae handle the offsets are the running sum and
the texture group begins at tex_encoder.weight (or at the end when there is one net).  A refusal must give the code and the whole
s3d_last_error() text of the tables below, which were recorded from the library as it stood before the two handles shared one
description of the net and the three handles one registry body.  Whether a constructor accepts a grid configuration depends on
(constructor, variant, tex_channels) alone — widths and feature groups of the grid are legal everywhere — so GRID_REFUSED is keyed by
that and the test holds every configuration of the grid to it."""
import ctypes as C
import itertools

import numpy as np
import pytest

from sin3dm_amd import _lib, testing as T

INVALID, UNSUPPORTED = _lib.ERR_INVALID, _lib.ERR_UNSUPPORTED
WIDTHS = ((64, 256), (32, 64), (32, 32), (96, 128), (16, 32))      # (feat_channel_up, mlp_hidden_channels); the last pads on the decoder
GROUPS = ((4, 8), (8, 4))                                          # (geo_feat_channels, tex_feat_channels)
TEX_CHANNELS = (1, 3, 8)
# constructor -> the variants it is asked for (the two without a variant argument build one net each)
CTORS = {"decoder_create": (0,), "decoder_create_variant": (0, 1, 2), "ae_create": (0,), "ae_create_variant": (0, 1, 2), "ae_create_pbr": (2,)}

PBR_WANTS_8 = "ae training: the PBR net has 8 material channels, got tex_channels=%d"
# (constructor, variant, tex_channels) -> (code, text); everything else of the grid is accepted
GRID_REFUSED = {
    ("decoder_create", 0, 8): (UNSUPPORTED, "decoder: tex_channels must be 1..3"),
    ("ae_create_variant", 2, 1): (UNSUPPORTED, PBR_WANTS_8 % 1),
    ("ae_create_variant", 2, 3): (UNSUPPORTED, PBR_WANTS_8 % 3),
    ("ae_create_variant", 2, 8): (UNSUPPORTED, "ae training: the PBR net (variant 2) is not built by this call; use s3d_ae_create_pbr"),
    ("ae_create_pbr", 2, 1): (UNSUPPORTED, PBR_WANTS_8 % 1),
    ("ae_create_pbr", 2, 3): (UNSUPPORTED, PBR_WANTS_8 % 3),
}

BASE = dict(geo=4, tex=8, up=64, hid=256, layers=4, tc=3)
# one illegal value per rule: (constructor, variant, overrides of BASE, (code, text)); None where the constructor does not look at the
# field (the geometry-only net ignores tex_*; the decoder's PBR net has its three heads whatever tex_channels says) and accepts
ILLEGAL = [
    ('decoder_create', 0, {'layers': 2}, (UNSUPPORTED, 'decoder: mlp_hidden_layers=2 (only the default 4 is built)')),
    ('decoder_create', 0, {'up': 0}, (INVALID, 'decoder: bad widths')),
    ('decoder_create', 0, {'hid': 0}, (INVALID, 'decoder: bad widths')),
    ('decoder_create', 0, {'geo': 33}, (UNSUPPORTED, 'decoder: feature groups must have 1..32 channels')),
    ('decoder_create', 0, {'tex': 33}, (UNSUPPORTED, 'decoder: feature groups must have 1..32 channels')),
    ('decoder_create', 0, {'tc': 0}, (UNSUPPORTED, 'decoder: tex_channels must be 1..3')),
    ('decoder_create', 0, {'tc': 9}, (UNSUPPORTED, 'decoder: tex_channels must be 1..3')),
    ('decoder_create', 0, {'null': 'cfg'}, (INVALID, 'decoder_create: null argument')),
    ('decoder_create', 0, {'null': 'out'}, (INVALID, 'decoder_create: null argument')),
    ('decoder_create_variant', 0, {'layers': 2}, (UNSUPPORTED, 'decoder: mlp_hidden_layers=2 (only the default 4 is built)')),
    ('decoder_create_variant', 0, {'up': 0}, (INVALID, 'decoder: bad widths')),
    ('decoder_create_variant', 0, {'hid': 0}, (INVALID, 'decoder: bad widths')),
    ('decoder_create_variant', 0, {'geo': 33}, (UNSUPPORTED, 'decoder: feature groups must have 1..32 channels')),
    ('decoder_create_variant', 0, {'tex': 33}, (UNSUPPORTED, 'decoder: feature groups must have 1..32 channels')),
    ('decoder_create_variant', 0, {'tc': 0}, (UNSUPPORTED, 'decoder: tex_channels must be 1..8')),
    ('decoder_create_variant', 0, {'tc': 9}, (UNSUPPORTED, 'decoder: tex_channels must be 1..8')),
    ('decoder_create_variant', 0, {'null': 'cfg'}, (INVALID, 'decoder_create: null argument')),
    ('decoder_create_variant', 0, {'null': 'out'}, (INVALID, 'decoder_create: null argument')),
    ('decoder_create_variant', 1, {'layers': 2}, (UNSUPPORTED, 'decoder: mlp_hidden_layers=2 (only the default 4 is built)')),
    ('decoder_create_variant', 1, {'up': 0}, (INVALID, 'decoder: bad widths')),
    ('decoder_create_variant', 1, {'hid': 0}, (INVALID, 'decoder: bad widths')),
    ('decoder_create_variant', 1, {'geo': 33}, (UNSUPPORTED, 'decoder: feature groups must have 1..32 channels')),
    ('decoder_create_variant', 1, {'tex': 33}, None),
    ('decoder_create_variant', 1, {'tc': 0}, None),
    ('decoder_create_variant', 1, {'tc': 9}, None),
    ('decoder_create_variant', 1, {'null': 'cfg'}, (INVALID, 'decoder_create: null argument')),
    ('decoder_create_variant', 1, {'null': 'out'}, (INVALID, 'decoder_create: null argument')),
    ('decoder_create_variant', 2, {'layers': 2, 'tc': 8}, (UNSUPPORTED, 'decoder: mlp_hidden_layers=2 (only the default 4 is built)')),
    ('decoder_create_variant', 2, {'up': 0, 'tc': 8}, (INVALID, 'decoder: bad widths')),
    ('decoder_create_variant', 2, {'hid': 0, 'tc': 8}, (INVALID, 'decoder: bad widths')),
    ('decoder_create_variant', 2, {'geo': 33, 'tc': 8}, (UNSUPPORTED, 'decoder: feature groups must have 1..32 channels')),
    ('decoder_create_variant', 2, {'tex': 33, 'tc': 8}, (UNSUPPORTED, 'decoder: feature groups must have 1..32 channels')),
    ('decoder_create_variant', 2, {'tc': 0}, None),
    ('decoder_create_variant', 2, {'tc': 9}, None),
    ('decoder_create_variant', 2, {'null': 'cfg', 'tc': 8}, (INVALID, 'decoder_create: null argument')),
    ('decoder_create_variant', 2, {'null': 'out', 'tc': 8}, (INVALID, 'decoder_create: null argument')),
    ('decoder_create_variant', 3, {}, (INVALID, 'decoder: variant 3 (0 skip net with texture, 1 geometry only, 2 PBR)')),
    ('ae_create', 0, {'layers': 2}, (UNSUPPORTED, 'ae: mlp_hidden_layers=2 (only the default 4 is built)')),
    ('ae_create', 0, {'up': 0}, (UNSUPPORTED, 'ae training: feat_channel_up=0 and mlp_hidden_channels=256 must be multiples of 32')),
    ('ae_create', 0, {'hid': 0}, (UNSUPPORTED, 'ae training: feat_channel_up=64 and mlp_hidden_channels=0 must be multiples of 32')),
    ('ae_create', 0, {'geo': 33}, (UNSUPPORTED, 'ae training: feature groups must be multiples of 4 channels, at most 12 together; got geo=33 tex=8')),
    ('ae_create', 0, {'tex': 33}, (UNSUPPORTED, 'ae training: feature groups must be multiples of 4 channels, at most 12 together; got geo=4 tex=33')),
    ('ae_create', 0, {'tc': 0}, (UNSUPPORTED, 'ae: tex_channels must be 1..8, got 0')),
    ('ae_create', 0, {'tc': 9}, (UNSUPPORTED, 'ae: tex_channels must be 1..8, got 9')),
    ('ae_create', 0, {'null': 'cfg'}, (INVALID, 'ae_create: null argument')),
    ('ae_create', 0, {'null': 'out'}, (INVALID, 'ae_create: null argument')),
    ('ae_create_variant', 0, {'layers': 2}, (UNSUPPORTED, 'ae: mlp_hidden_layers=2 (only the default 4 is built)')),
    ('ae_create_variant', 0, {'up': 0}, (UNSUPPORTED, 'ae training: feat_channel_up=0 and mlp_hidden_channels=256 must be multiples of 32')),
    ('ae_create_variant', 0, {'hid': 0}, (UNSUPPORTED, 'ae training: feat_channel_up=64 and mlp_hidden_channels=0 must be multiples of 32')),
    ('ae_create_variant', 0, {'geo': 33}, (UNSUPPORTED, 'ae training: feature groups must be multiples of 4 channels, at most 12 together; got geo=33 tex=8')),
    ('ae_create_variant', 0, {'tex': 33}, (UNSUPPORTED, 'ae training: feature groups must be multiples of 4 channels, at most 12 together; got geo=4 tex=33')),
    ('ae_create_variant', 0, {'tc': 0}, (UNSUPPORTED, 'ae: tex_channels must be 1..8, got 0')),
    ('ae_create_variant', 0, {'tc': 9}, (UNSUPPORTED, 'ae: tex_channels must be 1..8, got 9')),
    ('ae_create_variant', 0, {'null': 'cfg'}, (INVALID, 'ae_create: null argument')),
    ('ae_create_variant', 0, {'null': 'out'}, (INVALID, 'ae_create: null argument')),
    ('ae_create_variant', 1, {'layers': 2}, (UNSUPPORTED, 'ae: mlp_hidden_layers=2 (only the default 4 is built)')),
    ('ae_create_variant', 1, {'up': 0}, (UNSUPPORTED, 'ae training: feat_channel_up=0 and mlp_hidden_channels=256 must be multiples of 32')),
    ('ae_create_variant', 1, {'hid': 0}, (UNSUPPORTED, 'ae training: feat_channel_up=64 and mlp_hidden_channels=0 must be multiples of 32')),
    ('ae_create_variant', 1, {'geo': 33}, (UNSUPPORTED, 'ae training: feature groups must be multiples of 4 channels, at most 12 together; got geo=33 tex=0')),
    ('ae_create_variant', 1, {'tex': 33}, None),
    ('ae_create_variant', 1, {'tc': 0}, None),
    ('ae_create_variant', 1, {'tc': 9}, None),
    ('ae_create_variant', 1, {'null': 'cfg'}, (INVALID, 'ae_create: null argument')),
    ('ae_create_variant', 1, {'null': 'out'}, (INVALID, 'ae_create: null argument')),
    ('ae_create_variant', 2, {'layers': 2, 'tc': 8}, (UNSUPPORTED, 'ae: mlp_hidden_layers=2 (only the default 4 is built)')),
    ('ae_create_variant', 2, {'up': 0, 'tc': 8}, (UNSUPPORTED, 'ae training: feat_channel_up=0 and mlp_hidden_channels=256 must be multiples of 32')),
    ('ae_create_variant', 2, {'hid': 0, 'tc': 8}, (UNSUPPORTED, 'ae training: feat_channel_up=64 and mlp_hidden_channels=0 must be multiples of 32')),
    ('ae_create_variant', 2, {'geo': 33, 'tc': 8}, (UNSUPPORTED, 'ae training: feature groups must be multiples of 4 channels, at most 12 together; got geo=33 tex=8')),
    ('ae_create_variant', 2, {'tex': 33, 'tc': 8}, (UNSUPPORTED, 'ae training: feature groups must be multiples of 4 channels, at most 12 together; got geo=4 tex=33')),
    ('ae_create_variant', 2, {'tc': 0}, (UNSUPPORTED, 'ae training: the PBR net has 8 material channels, got tex_channels=0')),
    ('ae_create_variant', 2, {'tc': 9}, (UNSUPPORTED, 'ae training: the PBR net has 8 material channels, got tex_channels=9')),
    ('ae_create_variant', 2, {'null': 'cfg', 'tc': 8}, (INVALID, 'ae_create: null argument')),
    ('ae_create_variant', 2, {'null': 'out', 'tc': 8}, (INVALID, 'ae_create: null argument')),
    ('ae_create_variant', 3, {}, (INVALID, 'ae_create: variant 3 (0 skip net, 1 geometry only, 2 PBR net)')),
    ('ae_create_pbr', 2, {'layers': 2, 'tc': 8}, (UNSUPPORTED, 'ae: mlp_hidden_layers=2 (only the default 4 is built)')),
    ('ae_create_pbr', 2, {'up': 0, 'tc': 8}, (UNSUPPORTED, 'ae training: feat_channel_up=0 and mlp_hidden_channels=256 must be multiples of 32')),
    ('ae_create_pbr', 2, {'hid': 0, 'tc': 8}, (UNSUPPORTED, 'ae training: feat_channel_up=64 and mlp_hidden_channels=0 must be multiples of 32')),
    ('ae_create_pbr', 2, {'geo': 33, 'tc': 8}, (UNSUPPORTED, 'ae training: feature groups must be multiples of 4 channels, at most 12 together; got geo=33 tex=8')),
    ('ae_create_pbr', 2, {'tex': 33, 'tc': 8}, (UNSUPPORTED, 'ae training: feature groups must be multiples of 4 channels, at most 12 together; got geo=4 tex=33')),
    ('ae_create_pbr', 2, {'tc': 0}, (UNSUPPORTED, 'ae training: the PBR net has 8 material channels, got tex_channels=0')),
    ('ae_create_pbr', 2, {'tc': 9}, (UNSUPPORTED, 'ae training: the PBR net has 8 material channels, got tex_channels=9')),
    ('ae_create_pbr', 2, {'null': 'cfg', 'tc': 8}, (INVALID, 'ae_create_pbr: null argument')),
    ('ae_create_pbr', 2, {'null': 'out', 'tc': 8}, (INVALID, 'ae_create_pbr: null argument')),
]
SET_PARAM = [
    ('unet', 'rank', (INVALID, 'size mismatch for time_embed.0.weight')),
    ('unet', 'extent', (INVALID, 'size mismatch for time_embed.0.weight')),
    ('unet', 'unknown', (INVALID, "unexpected key 'no.such.weight' in state_dict")),
    ('unet', 'null.handle', (INVALID, 'set_param: null argument')),
    ('unet', 'null.name', (INVALID, 'set_param: null argument')),
    ('unet', 'null.data', (INVALID, 'set_param: null argument')),
    ('unet', 'null.shape', (INVALID, 'set_param: null argument')),
    ('decoder', 'rank', (INVALID, 'size mismatch for geo_convs.in_layers.0.weight')),
    ('decoder', 'extent', (INVALID, 'size mismatch for geo_convs.in_layers.0.weight')),
    ('decoder', 'unknown', (INVALID, "unexpected key 'no.such.weight' in decoder state_dict")),
    ('decoder', 'null.handle', (INVALID, 'decoder set_param: null argument')),
    ('decoder', 'null.name', (INVALID, 'decoder set_param: null argument')),
    ('decoder', 'null.data', (INVALID, 'decoder set_param: null argument')),
    ('decoder', 'null.shape', (INVALID, 'decoder set_param: null argument')),
]
PARAM_INFO = [
    ('unet', -1, (INVALID, 'param_info: index -1 out of range')),
    ('unet', 'n', (INVALID, 'param_info: index 74 out of range')),
    ('unet', 'null', (INVALID, 'param_info: index 0 out of range')),
    ('decoder', -1, (INVALID, 'decoder param_info: index -1 out of range')),
    ('decoder', 'n', (INVALID, 'decoder param_info: index 82 out of range')),
    ('decoder', 'null', (INVALID, 'decoder param_info: index 0 out of range')),
    ('ae', -1, (INVALID, 'ae param_info: index -1 out of range')),
    ('ae', 'n', (INVALID, 'ae param_info: index 52 out of range')),
    ('ae', 'null', (INVALID, 'ae param_info: index 0 out of range')),
]


def create(ctor, variant, geo, tex, up, hid, layers, tc, null=None):
    """(code, handle) of one constructor call; null: "cfg" or "out" passes a null pointer there"""
    lib = _lib.load()
    cfg = None if null == "cfg" else C.byref(_lib.DecoderCfg(geo, tex, up, hid, layers, tc))
    h = C.c_void_p()
    out = None if null == "out" else C.byref(h)
    if ctor in ("decoder_create_variant", "ae_create_variant"):
        rc = getattr(lib, "s3d_" + ctor)(cfg, variant, out)
    else:
        rc = getattr(lib, "s3d_" + ctor)(cfg, out)
    return rc, h


def destroy(ctor, h):
    (_lib.load().s3d_decoder_destroy if ctor.startswith("decoder") else _lib.load().s3d_ae_destroy)(h)


def manifest(variant, geo, tex, up, hid, tc, with_encoder):
    if variant == 0:
        sh = T.ae_param_shapes(geo, tex, up, hid, 4, tc, with_encoder=with_encoder)
    elif variant == 1:
        sh = T.geo_only_param_shapes(geo, up, hid, 4, with_encoder=with_encoder)
    else:
        sh = T.pbr_param_shapes(geo, tex, up, hid, 4, tc, with_encoder=with_encoder)
    # state_dict order of the flat vector: the geometry net, then the texture net (the manifests list both encoders first)
    return [(k, tuple(v)) for k, v in sh.items() if k.startswith("geo_")] + [(k, tuple(v)) for k, v in sh.items() if not k.startswith("geo_")]


def registry(ctor, h):
    """[(name, shape, offset or None)] of a decoder / ae handle"""
    lib, out = _lib.load(), []
    ae = ctor.startswith("ae")
    for i in range((lib.s3d_ae_num_params if ae else lib.s3d_decoder_num_params)(h)):
        name, shape, nd, off = C.c_char_p(), (C.c_int64 * 5)(), C.c_int(), C.c_int64()
        if ae:
            assert lib.s3d_ae_param_info(h, i, C.byref(name), shape, C.byref(nd), C.byref(off)) == 0, _lib.last_error()
        else:
            assert lib.s3d_decoder_param_info(h, i, C.byref(name), shape, C.byref(nd)) == 0, _lib.last_error()
        out.append((name.value.decode(), tuple(shape[k] for k in range(nd.value)), off.value if ae else None))
    return out


@pytest.mark.parametrize("ctor", list(CTORS))
def test_grid(ctor):
    """every configuration of the grid: the expected registry, or the refusal of GRID_REFUSED"""
    lib = _lib.load()
    ae = ctor.startswith("ae")
    for variant, (up, hid), (geo, tex), tc in itertools.product(CTORS[ctor], WIDTHS, GROUPS, TEX_CHANNELS):
        if ae and (up, hid) == (16, 32):
            continue                                           # (the padded widths are the decoder handle's)
        what = (ctor, variant, up, hid, geo, tex, tc)
        rc, h = create(ctor, variant, geo, tex, up, hid, 4, tc)
        want = GRID_REFUSED.get((ctor, variant, tc))
        if want:
            assert (rc, _lib.last_error()) == want, what
            assert not h.value, what
            continue
        assert rc == 0, (what, _lib.last_error())
        try:
            got = registry(ctor, h)
            assert [(n, s) for n, s, _ in got] == manifest(variant, geo, tex, up, hid, tc, with_encoder=ae), what
            oc = (lib.s3d_ae_out_channels if ae else lib.s3d_decoder_out_channels)(h)
            assert oc == (1 + tc, 1, 9)[variant], what
            if ae:
                sizes = [int(np.prod(s)) for _, s, _ in got]
                assert [o for _, _, o in got] == [sum(sizes[:i]) for i in range(len(sizes))], what
                tb = C.c_int64()
                assert lib.s3d_ae_param_numel(h, C.byref(tb)) == sum(sizes), what
                offs = {n: o for n, _, o in got}
                assert tb.value == offs.get("tex_encoder.weight", sum(sizes)), what
                assert ("tex_encoder.weight" in offs) == (variant != 1), what
        finally:
            destroy(ctor, h)


@pytest.mark.parametrize("ctor, variant, over, want", ILLEGAL, ids=[f"{c}.{v}.{'.'.join(f'{k}{x}' for k, x in o.items())}" for c, v, o, _ in ILLEGAL])
def test_illegal(ctor, variant, over, want):
    null = over.get("null")
    rc, h = create(ctor, variant, null=null, **dict(BASE, **{k: v for k, v in over.items() if k != "null"}))
    if want is None:
        assert rc == 0 and h.value, _lib.last_error()
        destroy(ctor, h)
    else:
        assert (rc, _lib.last_error()) == want
        assert not h.value


def unet_handle():
    cfg = _lib.UNetCfg(in_channels=12, model_channels=32, out_channels=12, num_res_blocks=1, n_levels=1, use_scale_shift_norm=1, is_rollout=1)
    cfg.channel_mult[0] = 1
    h = C.c_void_p()
    assert _lib.load().s3d_unet_create(C.byref(cfg), C.byref(h)) == 0, _lib.last_error()
    return h


@pytest.fixture(scope="module")
def handles():
    lib = _lib.load()
    hs = {"unet": unet_handle(), "decoder": create("decoder_create_variant", 2, **BASE)[1], "ae": create("ae_create", 0, **BASE)[1]}
    assert all(h.value for h in hs.values())
    yield hs
    lib.s3d_unet_destroy(hs["unet"]); lib.s3d_decoder_destroy(hs["decoder"]); lib.s3d_ae_destroy(hs["ae"])


# the first parameter of the two handles with a set_param: unet time_embed.0.weight [128, 32], decoder geo_convs.in_layers.0.weight [192, 4, 5, 5]
FIRST = {"unet": (b"time_embed.0.weight", (128, 32)), "decoder": (b"geo_convs.in_layers.0.weight", (192, 4, 5, 5))}


def set_param(handles, which, case):
    lib = _lib.load()
    fn = lib.s3d_unet_set_param if which == "unet" else lib.s3d_decoder_set_param
    name, shape = FIRST[which]
    data = (C.c_float * int(np.prod(shape)))()
    arr = lambda s: (C.c_int64 * len(s))(*s)
    if case == "good":
        return fn(handles[which], name, data, arr(shape), len(shape))
    if case == "rank":
        return fn(handles[which], name, data, arr(shape[:-1]), len(shape) - 1)
    if case == "extent":
        return fn(handles[which], name, data, arr(shape[:-1] + (shape[-1] + 1,)), len(shape))
    if case == "unknown":
        return fn(handles[which], b"no.such.weight", data, arr(shape), len(shape))
    null = {"null.handle": (None, name, data, arr(shape)), "null.name": (handles[which], None, data, arr(shape)),
            "null.data": (handles[which], name, None, arr(shape)), "null.shape": (handles[which], name, data, None)}[case]
    return fn(*null, len(shape))


def test_set_param_accepts(handles):
    for which in FIRST:
        assert set_param(handles, which, "good") == 0, _lib.last_error()


@pytest.mark.parametrize("which, case, want", SET_PARAM, ids=[f"{w}.{c}" for w, c, _ in SET_PARAM])
def test_set_param_refusals(handles, which, case, want):
    assert (set_param(handles, which, case), _lib.last_error()) == want


def param_info(handles, which, index):
    """index: an int on the handle, or "null" for index 0 on a null handle"""
    lib = _lib.load()
    h, i = (None, 0) if index == "null" else (handles[which], index)
    if isinstance(i, str):                                     # "n": one past the last
        i = {"unet": lib.s3d_unet_num_params, "decoder": lib.s3d_decoder_num_params, "ae": lib.s3d_ae_num_params}[which](h)
    name, shape, nd = C.c_char_p(), (C.c_int64 * 5)(), C.c_int()
    if which == "ae":
        return lib.s3d_ae_param_info(h, i, C.byref(name), shape, C.byref(nd), None)
    return (lib.s3d_unet_param_info if which == "unet" else lib.s3d_decoder_param_info)(h, i, C.byref(name), shape, C.byref(nd))


@pytest.mark.parametrize("which, index, want", PARAM_INFO, ids=[f"{w}.{i}" for w, i, _ in PARAM_INFO])
def test_param_info_refusals(handles, which, index, want):
    assert (param_info(handles, which, index), _lib.last_error()) == want


def test_param_info_null_outputs(handles):
    """name, shape and ndim are each optional"""
    lib = _lib.load()
    assert lib.s3d_unet_param_info(handles["unet"], 0, None, None, None) == 0
    assert lib.s3d_decoder_param_info(handles["decoder"], 0, None, None, None) == 0
    assert lib.s3d_ae_param_info(handles["ae"], 0, None, None, None, None) == 0
