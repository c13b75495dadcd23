"""CPU-only: PBR and geometry-only assets — the parameter registries of the decoder variants and of the
Python modules against the reference's recorded state_dict, get_networks' dispatch, the float64 restatement (pbr_cases.py)
pinned to the reference's outputs, and the PBR OBJ / GLB writers read back with the standard library."""
import ctypes as C
import json
import os
import struct
import zlib
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import pbr_cases as P
from conftest import golden, relerr
from sin3dm_amd import _lib, testing as T


def recorded(g, key):
    return [(str(n), tuple(int(v) for v in s if v)) for n, s in zip(g[f"{key}.param_names"], g[f"{key}.param_shapes"])]


def registry(variant, up, hid, tex_channels=8):
    lib = _lib.load()
    h = C.c_void_p()
    cfg = _lib.DecoderCfg(4, 8, up, hid, 4, tex_channels)
    _lib.check(lib.s3d_decoder_create_variant(C.byref(cfg), variant, C.byref(h)))
    try:
        out = []
        for i in range(lib.s3d_decoder_num_params(h)):
            name, shape, nd = C.c_char_p(), (C.c_int64 * 4)(), C.c_int()
            _lib.check(lib.s3d_decoder_param_info(h, i, C.byref(name), shape, C.byref(nd)))
            out.append((name.value.decode(), tuple(shape[k] for k in range(nd.value))))
        return out, lib.s3d_decoder_out_channels(h)
    finally:
        lib.s3d_decoder_destroy(h)


def cfg(enc_net_type, data_type, up=64, hid=256):
    return SimpleNamespace(enc_net_type=enc_net_type, data_type=data_type, fdim_geo=4, fdim_tex=8, fdim_up=up, hidden_dim=hid,
                           n_hidden_layers=4)


@pytest.mark.parametrize("tag", ["small", "wide"])
def test_variant_registries_equal_the_reference_state_dict(tag):
    g = golden("pbr_decoder")
    up, hid = (int(v) for v in g[f"pbr.{tag}.cfg"][:2])
    reg, width = registry(2, up, hid)
    assert reg == recorded(g, f"pbr.{tag}") and width == 9
    assert "tex_convs.1.in_layers.1.weight" in dict(reg) and "tex_convs.1.shortcut.weight" not in dict(reg)
    reg, width = registry(1, up, hid)
    assert reg == recorded(g, f"geo.{tag}") and width == 1
    reg, width = registry(0, up, hid, 8)
    assert reg == list(T.ae_param_shapes(4, 8, up, hid, 4, 8).items()) and width == 9
    reg0, width0 = registry(0, up, hid, 3)
    assert reg0 == list(T.ae_param_shapes(4, 8, up, hid, 4, 3).items()) and width0 == 4


def test_create_keeps_refusing_what_it_refused():
    lib = _lib.load()
    h = C.c_void_p()
    cfg8 = _lib.DecoderCfg(4, 8, 64, 256, 4, 8)
    assert lib.s3d_decoder_create(C.byref(cfg8), C.byref(h)) == _lib.ERR_UNSUPPORTED          # variant 0's own entry point: 1..3
    assert lib.s3d_decoder_create_variant(C.byref(cfg8), 3, C.byref(h)) == _lib.ERR_INVALID
    assert _lib.ABI_VERSION >= 10 and lib.s3d_abi_version() == _lib.ABI_VERSION


@pytest.mark.parametrize("tag", ["small", "wide"])
def test_module_state_dicts_and_strict_loading(tag):
    from sin3dm_amd.encoding.networks import AutoEncoderGroupPBR, AutoEncoderGroupSkip, get_networks
    g = golden("pbr_decoder")
    up, hid = (int(v) for v in g[f"pbr.{tag}.cfg"][:2])
    enc = ("geo_encoder", "tex_encoder", "aabb")
    net = get_networks(cfg("pbr", "sdfpbr", up, hid))
    assert isinstance(net, AutoEncoderGroupPBR) and net.out_channels == 9
    sd = net.state_dict()
    assert [(k, tuple(v.shape)) for k, v in sd.items() if not k.startswith(enc)] == recorded(g, f"pbr.{tag}")
    assert tuple(sd["tex_encoder.weight"].shape) == (8, 9, 4, 4, 4) and tuple(sd["geo_encoder.weight"].shape) == (4, 1, 4, 4, 4)
    # a reference-shaped checkpoint (T.pbr_param_shapes(with_encoder=True) + aabb is the reference's state_dict) loads strictly
    full = T.synthetic_state_dict(T.pbr_param_shapes(4, 8, up, hid, 4, 8, with_encoder=True), 5)
    full["aabb"] = torch.tensor([-0.7, -1.0, -0.45, 0.7, 1.0, 0.45])
    assert sorted(full) == sorted(sd)
    net.load_state_dict(full, strict=True)
    assert torch.equal(net.state_dict()["rgb_decoder.second_layers.4.weight"], full["rgb_decoder.second_layers.4.weight"])
    assert len(net.geo_parameters()) + len(net.tex_parameters()) == len(list(net.parameters()))
    assert len(net.geo_parameters()) == len(recorded(g, f"geo.{tag}")) + 2 and len(net.tex_parameters()) > 3 * 12
    for geo_net in (get_networks(cfg("skip", "sdf", up, hid)), get_networks(cfg("pbr", "sdf", up, hid))):
        assert isinstance(geo_net, AutoEncoderGroupSkip) and geo_net.out_channels == 1 and geo_net.in_feat_channels == 4
        gsd = geo_net.state_dict()
        assert [(k, tuple(v.shape)) for k, v in gsd.items() if not k.startswith(enc)] == recorded(g, f"geo.{tag}")
        assert sorted(k for k in gsd if k.startswith(enc)) == ["aabb", "geo_encoder.bias", "geo_encoder.weight"]
        assert geo_net.tex_parameters() == []
        gfull = T.synthetic_state_dict(T.geo_only_param_shapes(4, up, hid, 4, with_encoder=True), 5)
        gfull["aabb"] = full["aabb"]
        geo_net.load_state_dict(gfull, strict=True)
        with pytest.raises(RuntimeError):
            geo_net.load_state_dict(full, strict=True)                      # texture keys are unexpected here


def test_get_networks_dispatch():
    from sin3dm_amd.encoding.networks import AutoEncoderGroupPBR, AutoEncoderGroupSkip, get_networks
    with pytest.raises(ValueError) as e:
        get_networks(cfg("pbr", "sdftex"))
    assert "enc_net_type" in str(e.value) and "data_type" in str(e.value)
    with pytest.raises(NotImplementedError):
        get_networks(cfg("base", "sdftex"))
    with pytest.raises(ValueError):
        get_networks(cfg("nonesuch", "sdftex"))
    net = get_networks(cfg("skip", "sdfpbr"))
    assert type(net) is AutoEncoderGroupSkip and net.out_channels == 9 and net.variant == 0
    assert tuple(net.state_dict()["tex_decoder.second_layers.4.weight"].shape) == (8, 256)
    assert tuple(net.state_dict()["tex_encoder.weight"].shape) == (8, 9, 4, 4, 4)
    net = get_networks(cfg("skip", "sdftex"))
    assert type(net) is AutoEncoderGroupSkip and net.out_channels == 4 and net.training_tier_built
    # training and encoding of the new variants are not built, and say so
    for c in (cfg("pbr", "sdfpbr"), cfg("skip", "sdf"), cfg("pbr", "sdf"), cfg("skip", "sdfpbr")):
        net = get_networks(c)
        assert isinstance(net, (AutoEncoderGroupPBR, AutoEncoderGroupSkip)) and not net.training_tier_built
        vol = torch.zeros(1, 1, 8, 8, 8)
        for call in (lambda: net.encode(vol), lambda: net(vol, torch.zeros(4, 3)),
                     lambda: net.loss_and_grads(vol, torch.zeros(4, 3), torch.zeros(4, 1), torch.zeros(4, 3), None),
                     lambda: net.flat_parameters):
            with pytest.raises(NotImplementedError, match="not built"):
                call()


# ------------------------------------------------------------------ the float64 restatement, pinned to the reference
PIN = 1e-5          # 10x the reference's own fp32-vs-fp64 gap on these inputs (6.2e-7 small, 1.1e-6 wide)


@pytest.mark.parametrize("tag", ["small", "wide"])
def test_restatement_is_pinned_to_the_reference(tag):
    g = golden("pbr_decoder")
    up, hid = (int(v) for v in g[f"pbr.{tag}.cfg"][:2])
    fm = [torch.from_numpy(g[f"pbr.{tag}.{p}"]).double() for p in T.PLANES]
    pts, aabb = g[f"pbr.{tag}.pts"], g[f"pbr.{tag}.aabb"]
    sd = P.weights("pbr", up, hid)
    feats = P.plane_stage("pbr", sd, fm)
    errs = {}
    for grp in ("geo", "tex0", "tex"):
        for p, f in zip(T.PLANES, feats[grp]):
            errs[f"{grp}_{p}"] = relerr(f.numpy(), g[f"pbr.{tag}.{grp}_{p}"])
    errs["out"] = relerr(P.decode("pbr", sd, pts, fm, aabb, feats).numpy(), g[f"pbr.{tag}.out"])
    errs["out_default_aabb"] = relerr(P.decode("pbr", sd, pts[:33], fm, [-1, -1, -1, 1, 1, 1], feats).numpy(), g[f"pbr.{tag}.out_default_aabb"])
    gfm = [f[:, :4] for f in fm]
    gsd = P.weights("geo", up, hid)
    errs["geo.out"] = relerr(P.decode("geo", gsd, pts, gfm, aabb).numpy(), g[f"geo.{tag}.out"])
    errs["geo.out_default_aabb"] = relerr(P.decode("geo", gsd, pts[:33], gfm, [-1, -1, -1, 1, 1, 1]).numpy(), g[f"geo.{tag}.out_default_aabb"])
    if tag == "small":
        ssd = P.weights("skip8", up, hid)
        errs["skip8.out"] = relerr(P.decode("skip8", ssd, pts, fm, aabb).numpy(), g[f"skip8.{tag}.out"])
        errs["skip8.out_default_aabb"] = relerr(P.decode("skip8", ssd, pts[:33], fm, [-1, -1, -1, 1, 1, 1]).numpy(), g[f"skip8.{tag}.out_default_aabb"])
    print(tag, {k: f"{v:.2e}" for k, v in errs.items()})
    assert max(errs.values()) < PIN, errs
    # the golden itself is not vacuous for the clamp and border tests built on it
    mat = g[f"pbr.{tag}.out"][:, 1:]
    assert 0.3 < float(((mat < 0) | (mat > 1)).mean()) < 0.7 and g[f"pbr.{tag}.out"].shape == (257, 9)


# ------------------------------------------------------------------ writers
def read_png(data):
    """(array [h,w,ch] uint8, colour type) of an 8-bit non-interlaced PNG whose rows all use filter 0"""
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, idat, hdr = 8, b"", None
    while pos < len(data):
        n, tag = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        assert struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])[0] == zlib.crc32(tag + body) & 0xFFFFFFFF
        if tag == b"IHDR":
            hdr = struct.unpack(">IIBBBBB", body)
        elif tag == b"IDAT":
            idat += body
        pos += 12 + n
    w, h, depth, ctype = hdr[:4]
    ch = {0: 1, 2: 3, 4: 2, 6: 4}[ctype]
    rows = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(h, 1 + w * ch)
    assert depth == 8 and (rows[:, 0] == 0).all()
    return rows[:, 1:].reshape(h, w, ch), ctype


def toy_mesh():
    verts = np.asarray([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32)
    tris = np.asarray([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]], np.int32)
    uvs = np.random.Generator(np.random.PCG64(3)).uniform(0, 1, size=(12, 2)).astype(np.float32)
    img = np.random.Generator(np.random.PCG64(4)).integers(0, 256, size=(16, 16, 8), dtype=np.uint8)
    return verts, tris, uvs, img


def test_export_pbr_obj(tmp_path):
    from sin3dm_amd.encoding import isosurface as iso
    verts, tris, uvs, img = toy_mesh()
    al, me, ro, no = iso.split_pbr_image(img)
    assert np.array_equal(al, img[..., :3]) and np.array_equal(me, img[..., 3]) and np.array_equal(ro, img[..., 4]) and np.array_equal(no, img[..., 5:])
    out = tmp_path / "mesh"
    iso.export_pbr_obj(str(out / "object.obj"), verts, tris, uvs, al, me, ro, no)
    found = sorted(os.path.relpath(os.path.join(r, f), out) for r, _, fs in os.walk(out) for f in fs)
    assert found == ["object.mtl", "object.obj", "textures/albedo.png", "textures/metallic.png", "textures/normal.png", "textures/roughness.png"]
    mtl = open(out / "object.mtl").read().splitlines()
    assert mtl == ["newmtl material_0", "Ns 250", "Ks 0.5 0.5 0.5", "Ke 0 0 0", "Ni 1.5", "d 1.0", "illum 2", "Ps 0.0", "Pc 0.0", "Pcr 0.03",
                   "aniso 0.0", "anisor 0.0", "map_Kd textures/albedo.png", "map_Pm textures/metallic.png", "map_Pr textures/roughness.png",
                   "map_Bump -bm 1.000000 textures/normal.png"]
    for name, want, ctype in (("albedo", al, 2), ("metallic", me[..., None], 0), ("roughness", ro[..., None], 0), ("normal", no, 2)):
        got, ct = read_png(open(out / "textures" / f"{name}.png", "rb").read())
        assert ct == ctype and np.array_equal(got[::-1], want), name            # row 0 of the array is the PNG's bottom row
    lines = open(out / "object.obj").read().splitlines()
    assert lines[0] == "mtllib object.mtl" and sum(l.startswith("v ") for l in lines) == 4 and sum(l.startswith("vt ") for l in lines) == 12
    faces = [l for l in lines if l.startswith("f ")]
    assert faces[0] == "f 1/1 3/2 2/3" and len(faces) == 4 and "usemtl material_0" in lines
    with pytest.raises(TypeError):
        iso.export_pbr_obj(str(out / "object.obj"), verts, tris, uvs, al, me, ro, no, Kd=[1, 1, 1])
    with pytest.raises(ValueError):
        iso.export_pbr_obj(str(out / "object.obj"), verts, tris, uvs, al, al, ro, no)


def test_export_pbr_glb(tmp_path):
    from sin3dm_amd.encoding import isosurface as iso
    verts, tris, uvs, img = toy_mesh()
    al, me, ro, no = iso.split_pbr_image(img)
    iso.export_pbr_obj(str(tmp_path / "o" / "object.obj"), verts, tris, uvs, al, me, ro, no)
    path = tmp_path / "object.glb"
    iso.export_pbr_glb(str(path), verts, tris, uvs, al, me, ro, no)
    data = open(path, "rb").read()
    magic, version, total = struct.unpack("<III", data[:12])
    jlen, jtag = struct.unpack("<II", data[12:20])
    g = json.loads(data[20:20 + jlen])
    blen, btag = struct.unpack("<II", data[20 + jlen:28 + jlen])
    blob = data[28 + jlen:]
    assert magic == 0x46546C67 and version == 2 and total == len(data) and jtag == 0x4E4F534A and btag == 0x004E4942 and blen == len(blob)
    assert jlen % 4 == 0 and blen % 4 == 0 and g["buffers"][0]["byteLength"] == blen
    assert len(g["images"]) == 3 and len(g["textures"]) == 3 and len(g["materials"]) == 1
    m = g["materials"][0]
    pm = m["pbrMetallicRoughness"]
    assert pm["metallicFactor"] == 1.0 and pm["roughnessFactor"] == 1.0 and m["doubleSided"] is True
    assert g["meshes"][0]["primitives"][0]["material"] == 0

    def image_of(slot):
        bv = g["bufferViews"][g["images"][g["textures"][slot["index"]]["source"]]["bufferView"]]
        return blob[bv["byteOffset"]:bv["byteOffset"] + bv["byteLength"]]
    assert image_of(pm["baseColorTexture"]) == open(tmp_path / "o" / "textures" / "albedo.png", "rb").read()
    packed, ct = read_png(image_of(pm["metallicRoughnessTexture"]))
    assert ct == 2 and (packed[..., 0] == 0).all() and np.array_equal(packed[::-1, :, 1], ro) and np.array_equal(packed[::-1, :, 2], me)
    normal, ct = read_png(image_of(m["normalTexture"]))
    assert ct == 2 and np.array_equal(normal[::-1], no)
    assert len({pm["baseColorTexture"]["index"], pm["metallicRoughnessTexture"]["index"], m["normalTexture"]["index"]}) == 3
    assert g["accessors"][0]["count"] == g["accessors"][1]["count"] == 12
