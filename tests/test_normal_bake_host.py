"""CPU-only: the conditions on tests/normal_bake_cases.py.  Every check passes on the clean restatement and reports each injected
fault; the designed cases hold what they were designed for; the float32 restatement stays inside the float32 bound and under the
cap on texels near a rounding boundary; the library exports the two entry points and refuses bad arguments; the GLB's tangents."""
import os
import re

import numpy as np
import pytest

import normal_bake_cases as NB

CASES = tuple(NB.SHAPES)


@pytest.mark.parametrize("name", CASES)
def test_clean_restatement_passes_every_check(name):
    c = NB.case(name)
    img, st, _ = NB.ref(name)
    problems, share, _ = NB.check_bake(img, st, c)
    assert not problems and share <= NB.MAX_CLOSE_SHARE, (problems, share)
    problems, worst = NB.check_round_trip(img, c)
    assert not problems and worst <= 0.389 + 1e-6, (problems, worst)          # float64: the quantisation bound itself


@pytest.mark.parametrize("name", CASES)
def test_float32_restatement_stays_inside_the_bound(name):
    """float32 with the same order of operations: the same status everywhere, bytes that differ by one level only within
    float32_delta of a rounding boundary, and few such texels — what the device is held to"""
    c = NB.case(name)
    img, st, x32 = NB.bake(c, np.float32)
    problems, share, ones = NB.check_bake(img, st, c)
    print(f"case {name}: {len(x32['p'])} entries on faces, close share {share:.4f}, {ones} bytes off by one in float32")
    assert not problems, problems
    x64 = NB.ref(name)[2]
    enc = (x64["status"] == 1) | (x64["status"] == 4)
    err = np.abs(x32["val"].astype(np.float64) - x64["val"])[enc]
    assert (err <= NB.float32_delta(x64)[enc]).all(), float((err / NB.float32_delta(x64)[enc]).max())
    assert not NB.check_round_trip(img, c)[0]


def test_cases_hold_what_they_were_designed_for():
    seen_corner0, seen_upper = set(), False
    for name in CASES:
        c = NB.case(name)
        assert (c["F"], c["T"]) == NB.SHAPES[name] and NB.atlas_layout(c["F"], c["T"]) == (c["n"], c["c"])
        _, st, x = NB.ref(name)
        k_all, _, _, upper = NB.charts(c["F"], c["T"], c["n"], c["c"])
        seen_corner0 |= set(int(v) for v in c["corner0"][np.unique(x["k"])])
        seen_upper |= bool(upper[x["p"]].any()) and bool((~upper[x["p"]]).any())
        assert set(np.flatnonzero(k_all >= 0)) <= set(c["idx"].tolist())                  # every covered texel is an entry
    assert seen_corner0 == {0, 1, 2} and seen_upper
    one, two, edge, patch = (NB.case(n) for n in CASES)
    T = one["T"]
    assert one["base"] is None and ((one["idx"] < 0).any() and (one["idx"] >= T * T).any())
    assert set(NB.ref("one")[1][NB.ref("one")[2]["p"]]) == {4} and NB.ref("one")[1][0] == 0 and (NB.ref("one")[1] == 0).sum() == T * T - 6
    assert two["tris"].min() == 1000
    x = NB.ref("two")[2]
    fn = NB._face_normals(two["verts"], two["tris"])[x["k"]]
    against = NB._dot(fn, x["ghat"]) < 0
    assert against[x["k"] == 1].all() and not against[x["k"] == 0].any() and set(x["status"]) == {1}
    assert (x["frame"][against, 2] * fn[against]).sum(1).max() < 0                         # N went to the field's side
    x = NB.ref("edge")[2]
    by_face = {f: set(x["status"][x["k"] == f]) for f in range(5)}
    assert by_face == {0: {1, 2}, 1: {3}, 2: {3}, 3: {4}, 4: {4}}, by_face
    assert (x["status"] == 2).sum() == 5
    par = (np.abs(NB._dot(x["ghat"], x["frame"][:, 0])) > 1 - 1e-12) & (x["status"] == 1)
    assert par[x["k"] == 0].sum() == 1 and (x["val"][par & (x["k"] == 0)][:, 1:] == 127.5).all()
    assert not edge["tangents"][2].any() and edge["tangents"][1].any()
    x = NB.ref("patch")[2]
    assert set(x["status"]) == {1, 4} and len(x["p"]) > 3 * 256
    fn = NB._face_normals(patch["verts"], patch["tris"])[x["k"]]
    assert 0.2 < (NB._dot(fn, x["ghat"]) < 0).mean() < 0.5
    assert np.isnan(patch["base"][17]).any() and not patch["base"][7].any()
    assert (x["kT"] < 1.5).mean() > 0.9 and np.abs(x["kT"] - 1).max() > 1e-3               # Gram-Schmidt has something to do


@pytest.mark.parametrize("fault", NB.FAULTS)
def test_checks_report_each_fault(fault):
    """the byte comparison reports every fault on at least one case; the round trip reports those that break the frame"""
    hit_bytes, hit_trip = [], []
    for name in CASES:
        c = NB.case(name)
        img, st, _ = NB.bake(c, fault=fault)
        if NB.check_bake(img, st, c)[0]:
            hit_bytes.append(name)
        if NB.check_round_trip(img, c)[0]:
            hit_trip.append(name)
    print(fault, "bytes:", hit_bytes, "round trip:", hit_trip)
    assert hit_bytes, fault
    if fault in ("b_sign", "no_gram_schmidt", "no_orient", "swap_b", "scale128"):
        assert hit_trip, fault


@pytest.mark.parametrize("channels", [1, 3])
def test_dilation_restatement_and_its_faults(channels):
    image, mask = NB.dilate_case(channels)
    T = image.shape[0]
    assert mask[[0, 0, -1, -1], [0, -1, 0, -1]].all() and all(0 < m.sum() < T for m in (mask[0], mask[-1], mask[:, 0], mask[:, -1]))
    out = NB.dilate_nearest(image, mask)
    assert np.array_equal(out[mask], image[mask]) and not NB.check_dilate(out, image, mask)
    assert np.array_equal(out[11, 11], image[12, 12]) and np.array_equal(out[13, 13], image[12, 12]) and np.array_equal(out[10, 10], image[10, 10])
    for fault in NB.DILATE_FAULTS:
        assert NB.check_dilate(NB.dilate_nearest(image, mask, fault), image, mask), fault
    # every position of ORDER decides somewhere: for each j a texel whose first covered neighbour is ORDER[j]
    first = set()
    for y, x in np.argwhere(~mask):
        for j, (dx, dy) in enumerate(NB.ORDER):
            if 0 <= x + dx < T and 0 <= y + dy < T and mask[y + dy, x + dx]:
                first.add(j)
                break
    assert first == set(range(8)), first


def test_entry_points_and_refusals():
    from sin3dm_amd import _lib
    lib = _lib.load()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "sin3dm_hip.h")).read()
    for name in ("s3d_tex_normal_texels", "s3d_tex_dilate_nearest"):
        assert name in _lib.SIGNATURES and hasattr(lib, name) and re.search(rf"S3D_API int {name}\(", header)
    assert int(re.search(r"#define S3D_ABI_VERSION (\d+)", header).group(1)) == _lib.ABI_VERSION == lib.s3d_abi_version() == 13
    import ctypes as C
    fake, inv = C.c_void_p(64), _lib.ERR_INVALID
    ok_mesh = (fake, 3, fake, fake, 1)
    assert lib.s3d_tex_normal_texels(fake, fake, 1, *ok_mesh, 8, 1, 8, None, fake, None, fake, None) == inv and b"tex_normal_texels" in lib.s3d_last_error()
    assert lib.s3d_tex_normal_texels(None, fake, 1, *ok_mesh, 8, 1, 8, None, fake, fake, fake, None) == inv
    assert lib.s3d_tex_normal_texels(fake, fake, 1, *ok_mesh, 8, 1, 8, None, None, fake, fake, None) == inv              # no tangents
    assert lib.s3d_tex_normal_texels(fake, fake, 1, *ok_mesh, 8, 1, 7, None, fake, fake, fake, None) == inv              # cell < 8
    assert lib.s3d_tex_normal_texels(fake, fake, 1, *ok_mesh, 8, 2, 8, None, fake, fake, fake, None) == inv              # 2 x 8 > 8
    assert lib.s3d_tex_normal_texels(fake, fake, 1, fake, 3, fake, fake, 3, 8, 1, 8, None, fake, fake, fake, None) == inv   # 3 faces, one cell
    assert lib.s3d_tex_normal_texels(fake, fake, -1, *ok_mesh, 8, 1, 8, None, fake, fake, fake, None) == inv
    assert lib.s3d_tex_dilate_nearest(fake, fake, 8, 3, fake, None) == inv and b"tex_dilate_nearest" in lib.s3d_last_error()   # aliased
    assert lib.s3d_tex_dilate_nearest(fake, fake, 0, 3, C.c_void_p(128), None) == inv
    assert lib.s3d_tex_dilate_nearest(None, fake, 8, 3, C.c_void_p(128), None) == inv


def test_corner_tangents_of_the_glb():
    from sin3dm_amd.encoding.isosurface import corner_tangents
    rng = np.random.Generator(np.random.PCG64(3))
    n = rng.standard_normal((12, 3))
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    n[9:12] = 0                                                             # face 3: zero normals, nothing to be orthogonal to
    tb = rng.standard_normal((4, 2, 3))
    tb[1] = 0                                                               # face 1: no tangent
    tb[2, 0] = 2.5 * n[6]                                                   # face 2, corner 0: T parallel to n
    out = corner_tangents(n, tb)
    assert out.shape == (12, 4) and out.dtype == np.float32
    assert np.abs(np.linalg.norm(out[:, :3], axis=1) - 1).max() < 1e-6 and set(np.abs(out[:, 3])) == {1.0}
    assert np.abs((out[:, :3] * n).sum(1)).max() < 1e-6
    f = np.repeat(np.arange(4), 3)
    t_ref = tb[f, 0] - n * (n * tb[f, 0]).sum(1, keepdims=True)
    keep = np.array([0, 1, 2, 7, 8, 9, 10, 11])
    assert np.abs(out[keep, :3] - t_ref[keep] / np.linalg.norm(t_ref[keep], axis=1, keepdims=True)).max() < 1e-6
    assert np.array_equal(out[keep, 3], np.where((np.cross(n[keep], out[keep, :3].astype(np.float64)) * tb[f[keep], 1]).sum(1) < 0, -1.0, 1.0))
    assert (out[3:7, 3] == 1).all()
    for j in (3, 4, 5, 6):                                                  # the axis on which n is smallest, made orthogonal to n
        e = np.eye(3)[np.argmin(np.abs(n[j]))]
        want = e - n[j] * n[j].dot(e)
        assert np.abs(out[j, :3] - want / np.linalg.norm(want)).max() < 1e-6
    with pytest.raises(ValueError):
        corner_tangents(n[:9], tb)


def test_environment_switches(monkeypatch):
    from sin3dm_amd import sample
    for var in ("S3D_MESH_NORMAL_MAP", "S3D_MESH_NORMAL_MAP_PROJECT"):
        monkeypatch.delenv(var, raising=False)
    assert sample.mesh_normal_map() == "" and sample.mesh_normal_map_project() == 0
    monkeypatch.setenv("S3D_MESH_NORMAL_MAP", "field")
    monkeypatch.setenv("S3D_MESH_NORMAL_MAP_PROJECT", "2")
    assert sample.mesh_normal_map() == "field" and sample.mesh_normal_map_project() == 2
    assert sample.mesh_normal_map("") == "" and sample.mesh_normal_map_project("0") == 0
    for bad in ("faces", "Field"):
        with pytest.raises(ValueError):
            sample.mesh_normal_map(bad)
    for bad in ("-1", "two", "1.5"):
        with pytest.raises(ValueError):
            sample.mesh_normal_map_project(bad)
