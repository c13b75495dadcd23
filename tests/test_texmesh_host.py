"""CPU-only: the host half of the textured mesh export — the analytic per-face atlas against a NumPy
rasterisation of its stated rule, the OBJ/MTL/PNG and GLB writers read back with the standard library, S3D_MESH parsing."""
import json
import math
import os
import struct
import zlib

import numpy as np
import pytest

from conftest import REPO  # noqa: F401


# ------------------------------------------------------------------ the atlas rule, restated
def rasterise(F, T):
    """face id per texel [T,T] (y, x), -1 = uncovered, and how many charts claim each texel.  A texel belongs to face k iff its
    centre (x+.5, y+.5) lies in the closed chart triangle; evaluated in integers at 2x scale with edge functions."""
    half = (F + 1) // 2
    n = max(1, math.ceil(math.sqrt(half)))
    while n * n < half:
        n += 1
    while n > 1 and (n - 1) * (n - 1) >= half:
        n -= 1
    c = T // n
    face = np.full((T, T), -1, np.int64)
    claims = np.zeros((T, T), np.int64)
    ly, lx = np.meshgrid(np.arange(c), np.arange(c), indexing="ij")
    X, Y = 2 * lx + 1, 2 * ly + 1                                               # texel centres at 2x scale
    charts = (np.asarray([[1, 1], [c - 4, 1], [1, c - 4]]) * 2, np.asarray([[c - 1, c - 1], [4, c - 1], [c - 1, 4]]) * 2)
    inside = []
    for tri in charts:
        ok = np.ones((c, c), bool)
        for i in range(3):
            (ax, ay), (bx, by) = tri[i], tri[(i + 1) % 3]
            ok &= (bx - ax) * (Y - ay) - (by - ay) * (X - ax) >= 0              # counter-clockwise: inside is to the left
        inside.append(ok)
    for k in range(F):
        cell = k // 2
        ox, oy = (cell % n) * c, (cell // n) * c
        m = inside[k % 2]
        claims[oy:oy + c, ox:ox + c] += m
        face[oy:oy + c, ox:ox + c][m] = k
    return face, claims, n, c


def min_chebyshev_between_faces(face):
    """smallest Chebyshev distance between texels of different faces, searched up to 2 (returns 3 when none is closer)"""
    T = face.shape[0]
    for d in (1, 2):
        for dy in range(-d, d + 1):
            for dx in range(-d, d + 1):
                if max(abs(dy), abs(dx)) != d:
                    continue
                a = face[max(0, dy):T + min(0, dy), max(0, dx):T + min(0, dx)]
                b = face[max(0, -dy):T + min(0, -dy), max(0, -dx):T + min(0, -dx)]
                if ((a >= 0) & (b >= 0) & (a != b)).any():
                    return d
    return 3


@pytest.mark.parametrize("F,T", [(1, 64), (2, 64), (7, 128), (2000, 512), (10000, 2048)])
def test_atlas_layout(F, T):
    from sin3dm_amd.encoding.isosurface import triangle_atlas
    at = triangle_atlas(F, T)
    face, claims, n, c = rasterise(F, T)
    assert (at.n, at.c, at.L) == (n, c, c - 5) and at.n == math.ceil(math.sqrt(math.ceil(F / 2))) and c >= 8
    assert claims.max() == 1                                                     # no texel covered twice
    assert min_chebyshev_between_faces(face) >= 3
    # texels per chart from the rule: centres with x, y >= 1 and x + y <= c - 4 (the upper chart is its mirror image), i.e. the
    # lattice points of a triangle with L = c - 5 points on each leg: L (L + 1) / 2
    L = c - 5
    counts = np.bincount(face[face >= 0], minlength=F)
    assert (counts == L * (L + 1) // 2).all(), (counts.min(), counts.max(), L)
    corners = np.asarray(at.corners)
    assert corners.shape == (F, 3, 2) and corners.min() >= 0 and corners.max() <= T
    # the corners are the stated ones, counter-clockwise, and each chart's texels lie inside its own cell
    for k in sorted({0, 1, F - 1} & set(range(F))):
        cell = k // 2
        o = np.asarray([(cell % n) * c, (cell // n) * c])
        want = [[1, 1], [c - 4, 1], [1, c - 4]] if k % 2 == 0 else [[c - 1, c - 1], [4, c - 1], [c - 1, 4]]
        assert np.array_equal(corners[k], o + np.asarray(want))
        e1, e2 = corners[k][1] - corners[k][0], corners[k][2] - corners[k][0]
        assert e1[0] * e2[1] - e1[1] * e2[0] > 0
        ys, xs = np.nonzero(face == k)
        assert xs.min() >= o[0] and xs.max() < o[0] + c and ys.min() >= o[1] and ys.max() < o[1] + c
    # uvs: vertex j of face k is chart corner (j - corner0[k]) mod 3
    r = np.arange(F) % 3
    uv = at.uvs(r).reshape(F, 3, 2)
    for k in sorted({0, 1, F - 1} & set(range(F))):
        for j in range(3):
            assert np.allclose(uv[k, j] * T, corners[k, (j - r[k]) % 3])
    assert abs(at.utilisation - L * L / (c * c)) < 1e-12


def test_atlas_too_many_faces_for_the_texture():
    from sin3dm_amd.encoding.isosurface import triangle_atlas
    with pytest.raises(ValueError) as e:
        triangle_atlas(10000, 256)                                              # 71 cells per row: 3 texels each
    assert "--n_faces" in str(e.value) and "--texreso" in str(e.value)
    assert triangle_atlas(10000, 71 * 8).c == 8                                  # the smallest cell that is accepted


# ------------------------------------------------------------------ writers
def decode_png(data):
    """stdlib PNG reader for 8-bit non-interlaced images: every filter type"""
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    off, chunks = 8, []
    while off < len(data):
        n, tag = struct.unpack(">I4s", data[off:off + 8])
        body = data[off + 8:off + 8 + n]
        assert struct.unpack(">I", data[off + 8 + n:off + 12 + n])[0] == zlib.crc32(tag + body) & 0xFFFFFFFF
        chunks.append((tag, body))
        off += 12 + n
    assert chunks[0][0] == b"IHDR" and chunks[-1] == (b"IEND", b"")
    w, h, depth, ctype, comp, flt, inter = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (depth, comp, flt, inter) == (8, 0, 0, 0)
    ch = {0: 1, 2: 3, 4: 2, 6: 4}[ctype]
    raw = zlib.decompress(b"".join(b for t, b in chunks if t == b"IDAT"))
    stride = w * ch
    assert len(raw) == h * (stride + 1)
    out = np.zeros((h, stride), np.uint8)
    prev = np.zeros(stride, np.int64)
    for y in range(h):
        ft = raw[y * (stride + 1)]
        line = np.frombuffer(raw, np.uint8, stride, y * (stride + 1) + 1).astype(np.int64)
        cur = line.copy() if ft == 0 else np.zeros(stride, np.int64)
        for i in range(stride if ft else 0):
            a = cur[i - ch] if i >= ch else 0
            b = prev[i]
            c = prev[i - ch] if i >= ch else 0
            if ft == 0:
                p = 0
            elif ft == 1:
                p = a
            elif ft == 2:
                p = b
            elif ft == 3:
                p = (a + b) // 2
            else:
                pa, pb, pc = abs(b - c), abs(a - c), abs(a + b - 2 * c)
                p = a if pa <= pb and pa <= pc else b if pb <= pc else c
            cur[i] = (line[i] + p) & 255
        out[y] = cur
        prev = cur
    return out.reshape(h, w, ch)


def two_triangles():
    v = np.asarray([[0.0, 0.0, 0.0], [1.0, 0.0, 0.25], [1.0, 1.5, 0.0], [0.0, 1.0, -0.5]], np.float32)
    f = np.asarray([[0, 1, 2], [0, 2, 3]], np.int32)
    uv = np.random.Generator(np.random.PCG64(2)).uniform(0, 1, (6, 2)).astype(np.float32)
    img = np.random.Generator(np.random.PCG64(3)).integers(0, 256, (16, 16, 3), dtype=np.uint8)
    return v, f, uv, img


def parse_obj(path):
    v, vt, f, other = [], [], [], []
    for line in open(path):
        w = line.split()
        if w[0] == "v":
            v.append([float(x) for x in w[1:]])
        elif w[0] == "vt":
            vt.append([float(x) for x in w[1:]])
        elif w[0] == "f":
            f.append([[int(i) for i in x.split("/")] for x in w[1:]])
        else:
            other.append(line.strip())
    return np.asarray(v), np.asarray(vt), np.asarray(f), other


def test_obj_mtl_png_writer(tmp_path):
    from sin3dm_amd.encoding import isosurface as iso
    v, f, uv, img = two_triangles()
    obj = str(tmp_path / "out" / "object.obj")
    iso.export_textured_obj(obj, v, f, uv, img, material={"Kd": [0.8, 0.7, 0.6], "Ka": None, "Ks": None, "Ns": 250.0})
    assert sorted(os.listdir(tmp_path / "out")) == ["object.mtl", "object.obj", "object.png"]
    png = open(tmp_path / "out" / "object.png", "rb").read()
    assert np.array_equal(decode_png(png), img[::-1])                            # texel row y = 0 is the bottom row of the picture
    try:
        from PIL import Image
    except ImportError:
        Image = None
    if Image is not None:
        assert np.array_equal(np.asarray(Image.open(tmp_path / "out" / "object.png")), img[::-1])
    pv, pvt, pf, other = parse_obj(obj)
    assert other == ["mtllib object.mtl", "usemtl material_0"]
    assert np.allclose(pv, v, atol=1e-6) and np.allclose(pvt, uv, atol=1e-6)
    assert pf.shape == (2, 3, 2) and np.array_equal(pf[:, :, 0], f + 1)
    assert np.array_equal(pf[:, :, 1], np.arange(6).reshape(2, 3) + 1)
    assert pf[:, :, 0].min() >= 1 and pf[:, :, 0].max() <= len(pv) and pf[:, :, 1].min() >= 1 and pf[:, :, 1].max() <= len(pvt)
    lines = [l.strip() for l in open(tmp_path / "out" / "object.mtl")]
    assert lines == ["newmtl material_0", "Kd 0.8 0.7 0.6", "Ka 0 0 0", "Ks 0.4 0.4 0.4", "Ns 250.0", "illum 2", "map_Kd object.png"]
    # order in the OBJ: mtllib, v, vt, usemtl, f
    kinds = [l.split()[0] for l in open(obj)]
    assert kinds == ["mtllib"] + ["v"] * 4 + ["vt"] * 6 + ["usemtl"] + ["f"] * 2
    with pytest.raises(ValueError):
        iso.export_textured_obj(obj, v, f, uv[:5], img)


def test_mtl_block_is_copied(tmp_path):
    from sin3dm_amd.encoding import isosurface as iso
    v, f, uv, img = two_triangles()
    src = tmp_path / "src.mtl"
    src.write_text("# a comment\nnewmtl wood\n  Kd 0.1 0.2 0.3\nNs 96.0\nd 1.0\nmap_Kd wood.jpg\nKs 9 9 9\nnewmtl other\nKd 5 5 5\n")
    block = iso.read_material_params_from_mtl(str(src))
    assert block == "  Kd 0.1 0.2 0.3\nNs 96.0\nd 1.0\n"
    obj = str(tmp_path / "object.obj")
    iso.export_textured_obj(obj, v, f, uv, img, material={"Kd": [0.8, 0.7, 0.6]}, mtl_str=block)
    assert open(tmp_path / "object.mtl").read() == "newmtl material_0\n" + block + "map_Kd object.png\n"
    two = tmp_path / "two.mtl"
    two.write_text("newmtl a\nKd 1 0 0\nnewmtl b\nKd 0 1 0\n")
    assert iso.read_material_params_from_mtl(str(two)) == "Kd 1 0 0\n"


def test_glb_writer(tmp_path):
    from sin3dm_amd.encoding import isosurface as iso
    v, f, uv, img = two_triangles()
    iso.export_textured_obj(str(tmp_path / "object.obj"), v, f, uv, img)
    png = open(tmp_path / "object.png", "rb").read()
    glb = tmp_path / "g" / "object.glb"
    iso.export_glb(str(glb), v, f, uv, img)
    assert os.listdir(tmp_path / "g") == ["object.glb"]
    data = open(glb, "rb").read()
    magic, version, total = struct.unpack("<III", data[:12])
    assert magic == 0x46546C67 and data[:4] == b"glTF" and version == 2 and total == len(data)
    jlen, jtype = struct.unpack("<II", data[12:20])
    assert jtype == 0x4E4F534A and jlen % 4 == 0
    g = json.loads(data[20:20 + jlen])
    blen, btype = struct.unpack("<II", data[20 + jlen:28 + jlen])
    assert btype == 0x004E4942 and blen % 4 == 0 and 28 + jlen + blen == total
    blob = data[28 + jlen:]
    assert g["asset"]["version"] == "2.0" and g["buffers"] == [{"byteLength": blen}]
    for bv in g["bufferViews"]:
        assert bv["buffer"] == 0 and bv["byteOffset"] % 4 == 0 and 0 <= bv["byteOffset"] and bv["byteOffset"] + bv["byteLength"] <= blen
    prim = g["meshes"][0]["primitives"][0]
    assert "indices" not in prim and prim.get("mode", 4) == 4
    ap, at = g["accessors"][prim["attributes"]["POSITION"]], g["accessors"][prim["attributes"]["TEXCOORD_0"]]
    assert ap["count"] == at["count"] == 3 * len(f) and ap["type"] == "VEC3" and at["type"] == "VEC2"
    assert ap["componentType"] == at["componentType"] == 5126

    def view(acc, width):
        bv = g["bufferViews"][acc["bufferView"]]
        assert bv["byteLength"] == acc["count"] * width * 4
        return np.frombuffer(blob, "<f4", acc["count"] * width, bv["byteOffset"]).reshape(-1, width)
    pos, tex = view(ap, 3), view(at, 2)
    assert np.array_equal(pos, v[f.reshape(-1)])
    assert np.allclose(tex[:, 0], uv[:, 0], atol=1e-7) and np.allclose(tex[:, 1], 1.0 - uv[:, 1], atol=1e-7)
    assert np.allclose(ap["min"], pos.min(0)) and np.allclose(ap["max"], pos.max(0))
    image = g["images"][g["textures"][0]["source"]]
    bv = g["bufferViews"][image["bufferView"]]
    assert image["mimeType"] == "image/png" and blob[bv["byteOffset"]:bv["byteOffset"] + bv["byteLength"]] == png
    mat = g["materials"][prim["material"]]
    pbr = mat["pbrMetallicRoughness"]
    assert mat["doubleSided"] is True and pbr["baseColorFactor"] == [1.0, 1.0, 1.0, 1.0]
    assert pbr["metallicFactor"] == 0.0 and pbr["roughnessFactor"] == 1.0 and pbr["baseColorTexture"]["index"] == 0


def test_png_channel_counts():
    from sin3dm_amd.encoding.isosurface import png_bytes
    rng = np.random.Generator(np.random.PCG64(9))
    for ch in (1, 2, 3, 4):
        img = rng.integers(0, 256, (5, 7, ch), dtype=np.uint8)
        assert np.array_equal(decode_png(png_bytes(img)), img)
    with pytest.raises(ValueError):
        png_bytes(np.zeros((4, 4, 3), np.float32))


# ------------------------------------------------------------------ S3D_MESH
def test_mesh_mode_from_the_environment(monkeypatch):
    from sin3dm_amd import sample
    monkeypatch.delenv("S3D_MESH", raising=False)
    assert sample.mesh_mode() == "vertex"
    monkeypatch.setenv("S3D_MESH", "")
    assert sample.mesh_mode() == "vertex"
    monkeypatch.setenv("S3D_MESH", "vertex")
    assert sample.mesh_mode() == "vertex"
    monkeypatch.setenv("S3D_MESH", "textured")
    assert sample.mesh_mode() == "textured"
    monkeypatch.setenv("S3D_MESH", "foo")
    with pytest.raises(ValueError) as e:
        sample.mesh_mode()
    assert "foo" in str(e.value)
    assert sample.mesh_mode("vertex") == "vertex"                               # an explicit argument wins over the environment


def test_decode_dispatches_on_mesh_mode(monkeypatch, tmp_path):
    """sample.decode calls decode_texmesh with the CLI's --n_faces / --texreso / --file_format only under S3D_MESH=textured, and
    finds mesh/*.mtl beside --data_path for --copy_mtl"""
    from types import SimpleNamespace
    from sin3dm_amd import sample
    from sin3dm_amd.encoding import model
    from sin3dm_amd.utils import triplane_util
    calls = []

    class FakeAE:
        def __init__(self, *a, **k):
            pass

        def load_ckpt(self, name):
            pass

        def decode_mesh(self, save_dir, fm, reso):
            calls.append(("vertex", save_dir, reso))

        def decode_texmesh(self, save_dir, fm, reso, **kw):
            calls.append(("textured", save_dir, reso, kw))
    import torch
    monkeypatch.setattr(model, "ShapeAutoEncoder", FakeAE)
    monkeypatch.setattr(triplane_util, "load_triplane_data", lambda path, device=None, compose=True: [torch.zeros(2, 3, 3)] * 3)
    monkeypatch.setattr(sample.dist_util, "dev", lambda: torch.device("cpu"))
    (tmp_path / "data" / "mesh").mkdir(parents=True)
    (tmp_path / "data" / "mesh" / "b.mtl").write_text("newmtl m\nKd 1 1 1\n")
    args = SimpleNamespace(tag=str(tmp_path / "exp"), vox=False, reso=48, n_faces=1234, texreso=512, file_format="glb", copy_mtl=True,
                           data_path=str(tmp_path / "data" / "shape.npz"))
    path = str(tmp_path / "exp" / "results" / "000" / "feat.npz")
    monkeypatch.delenv("S3D_MESH", raising=False)
    sample.decode(args, [path])
    monkeypatch.setenv("S3D_MESH", "textured")
    sample.decode(args, [path])
    args.copy_mtl = False
    sample.decode(args, [path])
    assert calls[0] == ("vertex", os.path.dirname(path), 48)
    assert calls[1] == ("textured", os.path.dirname(path), 48, {"n_faces": 1234, "texture_reso": 512, "file_format": "glb",
                                                                "mtl_path": str(tmp_path / "data" / "mesh" / "b.mtl")})
    assert calls[2][3]["mtl_path"] is None
    monkeypatch.setenv("S3D_MESH", "foo")
    with pytest.raises(ValueError):
        sample.decode(args, [path])
