"""The baked normal map on the device: s3d_tex_normal_texels and s3d_tex_dilate_nearest against the float64
restatement of tests/normal_bake_cases.py (whose conditions tests/test_normal_bake_host.py holds), the round trip through the
shader's decoding rule, decode_texmesh(normal_map="field") in every export, the default exports, arrays against files in the
renderer, and the analytic sphere.  Every device call is made twice and must give the same bits."""
import functools
import json
import os
import struct

import numpy as np
import pytest
import torch

import normal_bake_cases as NB

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _cu(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a if dtype is None else np.asarray(a).astype(dtype))).to(DEV)


@functools.lru_cache(maxsize=None)
def device_bake(name):
    """(image [T*T, 3], status [T*T]) of s3d_tex_normal_texels on a case's arrays, numpy; two calls, the same bits"""
    from sin3dm_amd import _lib
    c = NB.case(name)
    T = c["T"]
    args = [_cu(c["grad"]), _cu(c["idx"]), _cu(c["verts"]), _cu(c["tris"]), _cu(c["corner0"]), None if c["base"] is None else _cu(c["base"]),
            _cu(c["tangents"])]
    grad, idx, verts, tris, corner0, base, tangents = args
    outs = []
    for fill in (7, 200):
        image = torch.full((T * T, 3), fill, device=DEV, dtype=torch.uint8)
        status = torch.full((T * T,), fill, device=DEV, dtype=torch.uint8)
        _lib.check(_lib.load().s3d_tex_normal_texels(_lib.ptr(grad), _lib.ptr(idx), idx.shape[0], _lib.ptr(verts), verts.shape[0], _lib.ptr(tris),
                                                     _lib.ptr(corner0), c["F"], T, c["n"], c["c"], _lib.ptr(base), _lib.ptr(tangents),
                                                     _lib.ptr(image), _lib.ptr(status), _lib.stream_ptr()))
        torch.cuda.synchronize()
        outs.append((image.cpu().numpy(), status.cpu().numpy()))
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])
    return outs[0]


@pytest.mark.parametrize("name", tuple(NB.SHAPES))
def test_bytes_and_status_against_the_restatement(name):
    """(a): status equal everywhere; bytes equal but for one level within float32_delta of a rounding boundary"""
    image, status = device_bake(name)
    problems, share, ones = NB.check_bake(image, status, NB.case(name))
    print(f"case {name}: close share {share:.4f}, {ones} bytes off by one")
    assert not problems, problems


@pytest.mark.parametrize("name", tuple(NB.SHAPES))
def test_round_trip_through_the_shaders_rule(name):
    """(b): decoded by s3d_pbr_shade's formula in the bake's frame, every encoded texel lies within 0.40 degrees of g^"""
    image, _ = device_bake(name)
    problems, worst = NB.check_round_trip(image, NB.case(name))
    print(f"case {name}: worst angle {worst:.4f} degrees")
    assert not problems, problems


def test_no_entries_and_no_faces():
    from sin3dm_amd import _lib
    image = torch.zeros((64, 3), device=DEV, dtype=torch.uint8)
    status = torch.ones((64,), device=DEV, dtype=torch.uint8)
    _lib.check(_lib.load().s3d_tex_normal_texels(None, None, 0, None, 0, None, None, 0, 8, 1, 8, None, None, _lib.ptr(image), _lib.ptr(status),
                                                 _lib.stream_ptr()))
    torch.cuda.synchronize()
    assert (image.cpu().numpy() == NB.FLAT).all() and not status.any()


@pytest.mark.parametrize("channels", [1, 3])
def test_dilate_nearest(channels):
    """(c)"""
    from sin3dm_amd import _lib
    image, mask = NB.dilate_case(channels)
    T = image.shape[0]
    q, fid = _cu(image), _cu(np.where(mask, 3, -1).reshape(-1), np.int32)
    outs = []
    for fill in (9, 250):
        out = torch.full((T, T, channels), fill, device=DEV, dtype=torch.uint8)
        _lib.check(_lib.load().s3d_tex_dilate_nearest(_lib.ptr(q), _lib.ptr(fid), T, channels, _lib.ptr(out), _lib.stream_ptr()))
        torch.cuda.synchronize()
        outs.append(out.cpu().numpy())
    assert np.array_equal(outs[0], outs[1])
    assert np.array_equal(outs[0], NB.dilate_nearest(image, mask)) and not NB.check_dilate(outs[0], image, mask)


def test_bake_normal_map_is_the_two_kernels():
    """isosurface.bake_normal_map on a case's mesh: its own corner0 and tangents, the restatement on the same"""
    from sin3dm_amd.encoding import isosurface as iso
    c = dict(NB.case("patch"))
    T = c["T"]
    verts, tris, base = _cu(c["verts"]), _cu(c["tris"]), _cu(np.nan_to_num(c["base"]))
    seen = []

    def grad_fn(p):
        seen.append(p)
        return torch.stack([0.3 * p[:, 0], -0.2 * p[:, 1], 1.0 + 0.1 * p[:, 2]], 1)
    image, status, tangents = iso.bake_normal_map(verts, tris, T, grad_fn, base_normals=base)
    again = iso.bake_normal_map(verts, tris, T, grad_fn, base_normals=base)
    assert all(torch.equal(a, b) for a, b in zip((image, status, tangents), again)) and len(seen) == 2
    face_id, pos, corner0, atlas = iso.atlas_texels(verts, tris, T)
    assert (atlas.n, atlas.c) == (c["n"], c["c"]) and tuple(image.shape) == (T, T, 3) and tuple(status.shape) == (T, T)
    idx = torch.nonzero(face_id >= 0).squeeze(1)
    assert torch.equal(seen[0], pos[idx])
    c.update(name="patch_own", corner0=corner0.cpu().numpy(), tangents=tangents.cpu().numpy(), idx=idx.cpu().numpy(), base=base.cpu().numpy(),
             grad=grad_fn(pos[idx]).cpu().numpy())
    got, mask = image.cpu().numpy(), (face_id >= 0).view(T, T).cpu().numpy()
    problems, share, ones = NB.check_bake(np.where(mask[..., None], got, NB.FLAT), status.cpu().numpy(), c, reference=NB.bake(c))
    assert not problems, problems
    assert np.array_equal(NB.dilate_nearest(got, mask), got) and (got[~mask] != NB.FLAT).any()          # the gutters hold their neighbours
    assert ones or np.array_equal(got, NB.bake_dilated(c)[0])
    with pytest.raises(ValueError):
        iso.bake_normal_map(verts, tris, T, lambda p: p[:, :2])
    with pytest.raises(ValueError):
        iso.bake_normal_map(verts, tris, T, grad_fn, base_normals=base[:-1])


# ------------------------------------------------------------------ (d), (e), (f): the exports
@functools.lru_cache(maxsize=None)
def _experiment(data_type):
    from test_sdf_grad_gpu import _experiment as other
    if data_type != "sdftex":
        return other(data_type)
    import tempfile
    from test_cli_gpu import make_experiment
    from test_pbr_gpu import autoencoder
    from sin3dm_amd.utils import parser_util as pu
    from sin3dm_amd.utils.triplane_util import load_triplane_data
    tag = make_experiment(tempfile.mkdtemp(prefix="normal_bake_"), hwd=(8, 10, 8))
    ae = autoencoder(tag)
    assert ae.data_type == "sdftex"
    return ae, [f.unsqueeze(0) for f in load_triplane_data(pu.encoding_feat_path(tag), device=DEV, compose=False)]


def _glb(path):
    """(gltf, accessor(i) -> float32 [count, width], image_bytes(i))"""
    raw = open(path, "rb").read()
    magic, version, total = struct.unpack_from("<III", raw, 0)
    assert magic == 0x46546C67 and version == 2 and total == len(raw)
    n, kind = struct.unpack_from("<II", raw, 12)
    assert kind == 0x4E4F534A
    gltf = json.loads(raw[20:20 + n])
    m, kind = struct.unpack_from("<II", raw, 20 + n)
    assert kind == 0x004E4942
    blob = raw[28 + n:28 + n + m]

    def accessor(i):
        a = gltf["accessors"][i]
        bv = gltf["bufferViews"][a["bufferView"]]
        width = {"VEC4": 4, "VEC3": 3, "VEC2": 2}[a["type"]]
        assert bv["byteLength"] == a["count"] * width * 4 and bv.get("target") == 34962
        return np.frombuffer(blob, "<f4", a["count"] * width, bv["byteOffset"]).reshape(-1, width)

    def image_bytes(i):
        bv = gltf["bufferViews"][gltf["images"][i]["bufferView"]]
        return blob[bv["byteOffset"]:bv["byteOffset"] + bv["byteLength"]]
    return gltf, accessor, image_bytes


KW = dict(n_faces=600, texture_reso=256)


@pytest.mark.parametrize("data_type", ["sdftex", "sdfpbr"])
def test_decode_texmesh_bakes_the_field(data_type, tmp_path):
    """(d)"""
    from test_sdf_grad_gpu import RESO, _files, _parse_obj
    from test_texmesh_host import decode_png
    from sin3dm_amd.encoding import isosurface as iso
    from sin3dm_amd.rendering.rasterizer import vertex_normals
    ae, fm = _experiment(data_type)
    aabb = ae._resize_aabb((fm[0].shape[-2], fm[0].shape[-1], fm[1].shape[-1]))
    plain = ae.decode_texmesh(str(tmp_path / "plain"), fm, RESO, **KW)
    obj = ae.decode_texmesh(str(tmp_path / "obj"), fm, RESO, normal_map="field", **KW)
    glb = ae.decode_texmesh(str(tmp_path / "glb"), fm, RESO, normal_map="field", file_format="glb", **KW)
    for o in (obj, glb):
        assert torch.equal(o["verts"], plain["verts"]) and torch.equal(o["tris"], plain["tris"]) and torch.equal(o["image"], plain["image"])
        assert tuple(o["normal_map"].shape) == (256, 256, 3) and o["normal_map"].dtype == torch.uint8
        assert tuple(o["normal_status"].shape) == (256, 256) and torch.equal(o["normal_status"] > 0, o["mask"])
        assert torch.equal(o["normals"], vertex_normals(o["verts"], o["tris"]))
        assert torch.equal(o["normal_map"], obj["normal_map"]) and torch.equal(o["normal_status"], obj["normal_status"])
    st = obj["normal_status"][obj["mask"]]
    print(data_type, "status counts 1..4:", [int((st == k).sum()) for k in (1, 2, 3, 4)])
    assert int(((st == 1) | (st == 4)).sum()) > 0.5 * st.numel()
    nmap = obj["normal_map"].cpu().numpy()
    assert len(np.unique(nmap[obj["mask"].cpu().numpy()], axis=0)) > 100                     # a map, not a constant
    # ---- the direct call on the returned mesh
    direct = iso.bake_normal_map(obj["verts"], obj["tris"], 256, lambda p: ae.net.sdf_and_grad(p, fm, aabb=aabb)[1], base_normals=obj["normals"])
    assert torch.equal(direct[0][obj["mask"]], obj["normal_map"][obj["mask"]]) and torch.equal(direct[0], obj["normal_map"])
    assert torch.equal(direct[1], obj["normal_status"])
    # ---- OBJ: files, MTL, PNG, vn
    fo, fp = _files(str(tmp_path / "obj")), _files(str(tmp_path / "plain"))
    if data_type == "sdftex":
        assert sorted(fo) == ["object.mtl", "object.obj", "object.png", "object_normal.png"] and sorted(fp) == ["object.mtl", "object.obj", "object.png"]
        assert fo["object.png"] == fp["object.png"]
        mtl = fo["object.mtl"].decode().splitlines()
        assert mtl[-1] == "map_Bump -bm 1.000000 object_normal.png" and mtl[:-1] == fp["object.mtl"].decode().splitlines()
        png = fo["object_normal.png"]
    else:
        from test_pbr_gpu import PBR_OBJ_FILES
        assert sorted(fo) == sorted(fp) == PBR_OBJ_FILES and fo["object.mtl"] == fp["object.mtl"]
        assert b"map_Bump -bm 1.000000 textures/normal.png" in fo["object.mtl"]
        for name in ("albedo", "metallic", "roughness"):
            assert fo[f"textures/{name}.png"] == fp[f"textures/{name}.png"]
        png = fo["textures/normal.png"]
        assert png != fp["textures/normal.png"]
    assert png == iso.png_bytes(nmap[::-1]) and np.array_equal(np.asarray(decode_png(png)).reshape(256, 256, 3), nmap[::-1])
    pv, pvn, pf = _parse_obj(str(tmp_path / "obj" / "object.obj"))
    assert len(pvn) == len(pv) == obj["verts"].shape[0] and pf.shape == (obj["tris"].shape[0], 3, 3) and np.array_equal(pf[..., 2], pf[..., 0])
    assert np.abs(pvn - obj["normals"].cpu().numpy()).max() < 1e-6
    assert b"\nvn " not in fp["object.obj"]
    # ---- GLB: attributes, tangents, the normal texture
    gltf, accessor, image_bytes = _glb(str(tmp_path / "glb" / "object.glb"))
    attrs = gltf["meshes"][0]["primitives"][0]["attributes"]
    assert set(attrs) == {"POSITION", "TEXCOORD_0", "NORMAL", "TANGENT"} and (attrs["POSITION"], attrs["TEXCOORD_0"], attrs["NORMAL"]) == (0, 1, 2)
    assert gltf["accessors"][attrs["TANGENT"]]["type"] == "VEC4"
    corners = glb["tris"].reshape(-1).long()
    normal, tangent = accessor(attrs["NORMAL"]), accessor(attrs["TANGENT"])
    assert np.array_equal(normal, glb["normals"][corners].cpu().numpy()) and np.array_equal(accessor(0), glb["verts"][corners].cpu().numpy())
    assert tangent.shape == (len(corners), 4) and set(np.abs(tangent[:, 3])) == {1.0}
    assert np.abs(np.linalg.norm(tangent[:, :3].astype(np.float64), axis=1) - 1).max() < 1e-5
    assert np.abs((tangent[:, :3].astype(np.float64) * normal).sum(1)).max() < 1e-5
    assert np.array_equal(tangent, iso.corner_tangents(normal, direct[2]))
    n_images = 2 if data_type == "sdftex" else 3
    assert len(gltf["images"]) == len(gltf["textures"]) == n_images
    mat = gltf["materials"][0]
    tex = mat["normalTexture"]["index"]
    assert tex == n_images - 1 and gltf["textures"][tex]["source"] == tex and image_bytes(tex) == iso.png_bytes(nmap[::-1])
    assert mat["pbrMetallicRoughness"]["baseColorTexture"]["index"] == 0
    gp, _, plain_images = _glb(str(_write_plain_glb(ae, fm, tmp_path)))
    assert "normalTexture" not in gp["materials"][0] or data_type == "sdfpbr"
    assert image_bytes(0) == plain_images(0)
    # ---- normals="field" are the base normals when asked for
    both = ae.decode_texmesh(str(tmp_path / "both"), fm, RESO, normal_map="field", normals="field", **KW)
    assert not torch.equal(both["normals"], obj["normals"]) and not torch.equal(both["normal_map"], obj["normal_map"])
    again = iso.bake_normal_map(both["verts"], both["tris"], 256, lambda p: ae.net.sdf_and_grad(p, fm, aabb=aabb)[1], base_normals=both["normals"])
    assert torch.equal(again[0], both["normal_map"])
    # ---- the projection changes the map and nothing else
    proj = ae.decode_texmesh(str(tmp_path / "proj"), fm, RESO, normal_map="field", normal_map_project=2, **KW)
    assert not torch.equal(proj["normal_map"], obj["normal_map"]) and torch.equal(proj["image"], obj["image"])
    assert torch.equal(proj["verts"], obj["verts"]) and torch.equal(proj["gb_pos"], obj["gb_pos"])
    for bad in (dict(normal_map="faces"), dict(normal_map="field", normal_map_project=-1), dict(normal_map="field", normal_map_max_move=0.0)):
        with pytest.raises(ValueError):
            ae.decode_texmesh(str(tmp_path / "bad"), fm, RESO, **bad, **KW)


def _write_plain_glb(ae, fm, tmp_path):
    from test_sdf_grad_gpu import RESO
    ae.decode_texmesh(str(tmp_path / "plain_glb"), fm, RESO, file_format="glb", **KW)
    return tmp_path / "plain_glb" / "object.glb"


def test_sdf_has_no_atlas_to_bake_on(tmp_path):
    from test_sdf_grad_gpu import RESO
    ae, fm = _experiment("sdf")
    with pytest.raises(ValueError, match="atlas"):
        ae.decode_texmesh(str(tmp_path / "sdf"), fm, RESO, normal_map="field", **KW)
    assert not os.path.exists(str(tmp_path / "sdf"))


@pytest.mark.parametrize("data_type", ["sdftex", "sdfpbr"])
def test_default_exports_do_not_reach_the_bake(data_type, tmp_path, monkeypatch):
    """(e): default keywords, with bake_normal_map made to raise, against the keywords spelled out: the same bytes, no
    object_normal.png, no TANGENT"""
    from test_sdf_grad_gpu import RESO, _files
    from sin3dm_amd.encoding import isosurface as iso
    ae, fm = _experiment(data_type)
    spelled = dict(normal_map=None, normal_map_project=0, normal_map_max_move=1.0)
    for fmt in ("obj", "glb"):
        ae.decode_texmesh(str(tmp_path / f"b_{fmt}"), fm, RESO, file_format=fmt, **spelled, **KW)

    def touched(*a, **k):
        raise AssertionError("a default export reached the normal bake")
    monkeypatch.setattr(iso, "bake_normal_map", touched)
    monkeypatch.setattr(type(ae), "_bake_field_normal_map", touched)
    for fmt in ("obj", "glb"):
        out = ae.decode_texmesh(str(tmp_path / f"a_{fmt}"), fm, RESO, file_format=fmt, **KW)
        assert out is not None and "normal_map" not in out and "normal_status" not in out and "normals" not in out
        fa, fb = _files(str(tmp_path / f"a_{fmt}")), _files(str(tmp_path / f"b_{fmt}"))
        assert fa and sorted(fa) == sorted(fb) and all(fa[n] == fb[n] for n in fa), fmt
        assert "object_normal.png" not in fa and all(b"TANGENT" not in data and b"\nvn " not in data for data in fa.values())
    with pytest.raises(AssertionError, match="reached the normal bake"):
        ae.decode_texmesh(str(tmp_path / "c"), fm, RESO, normal_map="field", **KW)


@pytest.mark.parametrize("data_type", ["sdftex", "sdfpbr"])
def test_arrays_and_files_render_alike(data_type, tmp_path):
    """(f): the `normal` pass under "pbr" with the returned maps equals, bit for bit, the same call with the materials that
    obj_io.load_obj + pbr.load_pbr_maps read from the written OBJ, and differs from the call without the normal map.
    Both calls take the geometry of the file (load_obj's verts, faces, uvs): the OBJ's six decimals are not the arrays' float32
    values, and two renders of geometry that differs in the seventh digit are not comparable bit for bit: the returned geometry
    against the file's differs on 405 of 73 728 pixels (silhouette samples, up to 57 levels) for either data type; the figure is
    printed."""
    from test_sdf_grad_gpu import RESO
    from sin3dm_amd.data.obj_io import load_obj
    from sin3dm_amd.rendering import pbr
    from sin3dm_amd.rendering.rasterizer import render_views
    ae, fm = _experiment(data_type)
    out = ae.decode_texmesh(str(tmp_path / "o"), fm, RESO, normal_map="field", **KW)
    path = str(tmp_path / "o" / "object.obj")
    mesh = load_obj(path)
    mats = [m for _, m in pbr.load_pbr_maps(path, mesh["materials"])]
    assert len(mats) == 1 and mats[0]["normal_image"] is not None and mats[0]["image"] is not None
    assert np.array_equal(mats[0]["normal_image"], out["normal_map"].cpu().numpy()[::-1])
    assert mesh["verts"].shape[0] == out["verts"].shape[0]
    verts, tris = _cu(mesh["verts"], np.float32), _cu(mesh["faces"], np.int32)
    uvs = _cu(mesh["uvs"], np.float32)
    img = out["image"].flip(0)
    own = {"Kd": mats[0].get("Kd", (1.0, 1.0, 1.0)), "image": img[..., :3], "normal_image": out["normal_map"].flip(0)}
    if data_type == "sdfpbr":
        own.update(metallic_image=img[..., 3], roughness_image=img[..., 4])
    kw = dict(uvs=uvs, shading="pbr", passes=("normal",), resolution=(96, 96), normals=out["normals"])
    from_files = render_views(verts, tris, materials=mats, **kw)
    from_arrays = render_views(verts, tris, materials=[own], **kw)
    assert torch.equal(from_files, render_views(verts, tris, materials=mats, **kw))
    assert torch.equal(from_arrays, from_files)
    without = render_views(verts, tris, materials=[{k: v for k, v in own.items() if k != "normal_image"}], **kw)
    assert not torch.equal(without, from_files) and torch.equal(without[..., 3], from_files[..., 3])
    returned = render_views(out["verts"], out["tris"], materials=[own], **dict(kw, uvs=out["uvs"].reshape(-1, 3, 2)))
    d = (returned != from_files).any(-1)
    print(f"{data_type}: returned float32 geometry against the file's six decimals: {int(d.sum())} of {d.numel()} pixels differ, "
          f"largest step {int((returned.int() - from_files.int()).abs().max())} levels")


# ------------------------------------------------------------------ (g): the analytic sphere
@functools.lru_cache(maxsize=None)
def sphere_errors(texreso=256, side=96):
    """(mean angular error in degrees with the map, without it, covered pixels): an octahedron cut to 32 faces in the unit sphere,
    the field p -> p baked on its flat normals and drawn "pbr_flat", against the same octahedron cut to 8 192 faces drawn "smooth" """
    from sin3dm_amd.encoding import isosurface as iso
    from sin3dm_amd.rendering import camera
    from sin3dm_amd.rendering.rasterizer import render_views
    v, f = NB.octasphere(1)
    assert len(f) == 32
    verts, tris = _cu(v), _cu(f)
    image, status, _ = iso.bake_normal_map(verts, tris, texreso, lambda p: p, base_normals=None)
    again = iso.bake_normal_map(verts, tris, texreso, lambda p: p, base_normals=None)
    assert torch.equal(image, again[0]) and torch.equal(status, again[1])
    face_id, _, corner0, atlas = iso.atlas_texels(verts, tris, texreso)
    assert set(status[face_id.view(texreso, texreso) >= 0].cpu().numpy().tolist()) == {4}                    # flat base normals
    uvs = torch.from_numpy(atlas.uvs(corner0.cpu().numpy())).to(DEV).reshape(-1, 3, 2)
    views = camera.standard_views(np.full(3, -1.0), np.full(3, 1.0), (side, side))
    kw = dict(views=views, resolution=(side, side), passes=("normal",))
    with_map = render_views(verts, tris, uvs=uvs, materials=[{"Kd": (1.0, 1.0, 1.0), "normal_image": image.flip(0)}], shading="pbr_flat", **kw)
    without = render_views(verts, tris, uvs=uvs, materials=[{"Kd": (1.0, 1.0, 1.0)}], shading="pbr_flat", **kw)
    vf, ff = NB.octasphere(5)
    assert len(ff) == 8192
    fine = render_views(_cu(vf), _cu(ff), shading="smooth", **kw)
    a, b, c = (x.cpu().numpy() for x in (with_map, without, fine))
    keep = (a[..., 3] == 255) & (b[..., 3] == 255) & (c[..., 3] == 255)
    return NB.mean_angle_deg(a, c, keep), NB.mean_angle_deg(b, c, keep), int(keep.sum())


def test_analytic_sphere():
    """(g): the map brings the 32-face render strictly closer to the 8 192-face one than the flat normals are"""
    with_map, without, n = sphere_errors()
    print(f"mean angular error over {n} pixels: {with_map:.3f} degrees with the map, {without:.3f} without, ratio {without / with_map:.1f}")
    assert n > 8 * 96 * 96 // 8 and with_map < without


def test_constant_field_renders_constant():
    """The bake and the shader agree on the frame, handedness and row order included: the map of a constant field g, drawn on the
    32-face octahedron with its flat normals, shows g on every face whose outward side is g's side.  All texels of such a face hold
    the same bytes (flat base normal: one frame per face), so the bilinear lookup is exact; what is left is the map's quantisation
    (asin(sqrt(3) / 255) = 0.389 degrees) and the pass's own (the same again): 0.80 degrees with the float32 slack."""
    from sin3dm_amd.encoding import isosurface as iso
    from sin3dm_amd.rendering import camera
    from sin3dm_amd.rendering.rasterizer import render_views
    g = np.array([0.3, 0.5, 0.8]) / np.linalg.norm([0.3, 0.5, 0.8])
    v, f = NB.octasphere(1)
    verts, tris = _cu(v), _cu(f)
    image, status, _ = iso.bake_normal_map(verts, tris, 256, lambda p: torch.from_numpy(g).float().to(DEV).expand(p.shape[0], 3), base_normals=None)
    face_id, _, corner0, atlas = iso.atlas_texels(verts, tris, 256)
    uvs = torch.from_numpy(atlas.uvs(corner0.cpu().numpy())).to(DEV).reshape(-1, 3, 2)
    kw = dict(views=camera.standard_views(np.full(3, -1.0), np.full(3, 1.0), (96, 96)), resolution=(96, 96), passes=("normal",), uvs=uvs,
              shading="pbr_flat", supersample=1)
    drawn = render_views(verts, tris, materials=[{"Kd": (1.0, 1.0, 1.0), "normal_image": image.flip(0)}], **kw).cpu().numpy()
    flat = render_views(verts, tris, materials=[{"Kd": (1.0, 1.0, 1.0)}], **kw).cpu().numpy()
    vec, covered = NB.normal_pass_vectors(drawn)
    outward, _ = NB.normal_pass_vectors(flat)
    keep = covered & ((outward * g).sum(-1) > 0.05)
    ang = NB.angle_deg(vec[keep], np.broadcast_to(g, vec[keep].shape))
    print(f"constant field: {int(keep.sum())} pixels, largest angle {ang.max():.3f} degrees")
    assert keep.sum() > 5000 and ang.max() <= 0.80


def test_render_sample_hands_the_map_to_the_shader(tmp_path, monkeypatch):
    """sample.render_sample with shading "pbr": the baked map of an sdftex export is the material's normal_image"""
    from test_sdf_grad_gpu import RESO
    from sin3dm_amd import sample
    from sin3dm_amd.rendering.rasterizer import render_views
    ae, fm = _experiment("sdftex")
    mesh = ae.decode_texmesh(str(tmp_path / "o"), fm, RESO, normal_map="field", **KW)
    calls = []

    def spy(verts, tris, **kw):
        calls.append(kw)
        return render_views(verts, tris, **dict(kw, resolution=(48, 48)))
    import sin3dm_amd.rendering.rasterizer as rz
    monkeypatch.setattr(rz, "render_views", spy)
    with_map = sample.render_sample(str(tmp_path / "a"), mesh, "pbr")
    without = sample.render_sample(str(tmp_path / "b"), {k: v for k, v in mesh.items() if k != "normal_map"}, "pbr")
    flat = sample.render_sample(str(tmp_path / "c"), mesh, "")
    assert len(with_map) == len(without) == len(flat) == 8
    assert torch.equal(calls[0]["materials"][0]["normal_image"], mesh["normal_map"].flip(0)) and torch.equal(calls[0]["normals"], mesh["normals"])
    assert "normal_image" not in calls[1]["materials"][0] and "normal_image" not in calls[2]["materials"][0] and "shading" not in calls[2]
    a, b = (open(p[0], "rb").read() for p in (with_map, without))
    assert a != b
