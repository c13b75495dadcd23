"""CPU-only: the host half of the PBR renders (sin3dm_amd/rendering/{pbr,render_pbr}.py, s3d_render_pbr.hip).  The
restatement of tests/render_pbr_cases.py against closed forms, its measured float32 gaps and its leave-out cap on every case; the
gain ladder's gap and conditions, and the wrong light models it sees where the images at gain 1 do not; the MTL parser, the command line's argument errors, the light rig, the header, the binding and the argument checks of the entry
points (which launch nothing, so they run without a GPU)."""
import ctypes as C
import math
import os
import re
import warnings

import numpy as np
import pytest

import render_cases as R
import render_pbr_cases as P
from conftest import REPO
from sin3dm_amd import _lib
from sin3dm_amd.rendering import pbr, render_pbr

ENTRY_POINTS = ("s3d_pbr_vertex_normals", "s3d_pbr_face_tangents", "s3d_pbr_shade")


# ------------------------------------------------------------------ the restatement against closed forms
def test_sphere_normals_are_radial():
    """Area-weighted normals of an icosphere on the unit sphere point along the radius to within the facet angle: the faces
    around a vertex tilt away from its radius by at most the angular size of an edge, theta, symmetrically up to the
    icosphere's own irregularity, so the deviation is bounded by 1 - cos(theta) <= theta^2 / 2."""
    for level in (1, 2):
        v, f = R.icosphere(level)
        n = P.vertex_normals(v.astype(np.float32), f)
        edge = max(np.linalg.norm(v[a] - v[b]) for tri in f for a, b in ((tri[0], tri[1]), (tri[1], tri[2])))
        theta = 2 * math.asin(edge / 2)
        dev = 1 - (n * v).sum(1)
        print(level, "largest 1 - n.r", dev.max(), "bound", theta ** 2 / 2)
        assert np.allclose(np.linalg.norm(n, axis=1), 1, atol=1e-12) and dev.max() <= theta ** 2 / 2
    # inside out: the opposite normals, exactly
    assert np.array_equal(P.vertex_normals(v.astype(np.float32), f[:, ::-1]), -n)


def test_zero_normals_and_degenerate_tangents():
    for name in ("b_quads", "c_fin"):
        c = P.case(name, "g64")
        n = P.vertex_normals(c["verts"], c["faces"])
        assert not n[c["zero_normals"]].any() and np.linalg.norm(np.delete(n, c["zero_normals"], 0), axis=1).min(initial=1) > 0.99
    c = P.case("b_quads", "g64")
    t = P.face_tangents(c["verts"], c["faces"], c["uvs"])
    assert not t[[2, 3, 5]].any() and t[[0, 1, 4]].any((1, 2)).all()          # det == 0: no tangent, beside good faces


def test_tangents_of_an_axis_aligned_quad():
    """A quad spanning (0..2, 0..3) in x, y with uv = (x / 2, y / 3): T = d p / d u = (2, 0, 0), B = d p / d v = (0, 3, 0)."""
    verts = np.array([[0, 0, 1], [2, 0, 1], [2, 3, 1], [0, 3, 1]], dtype=np.float32)
    faces = np.array([[0, 1, 2], [0, 2, 3], [2, 1, 0]])
    uv = verts[:, :2] / [2, 3]
    for dt in (np.float64, np.float32):
        t = P.face_tangents(verts, faces, uv[faces], dt)
        assert np.allclose(t[:, 0], [2, 0, 0], atol=1e-6) and np.allclose(t[:, 1], [0, 3, 0], atol=1e-6)


def test_ggx_energy_at_roughness_one():
    """At r = 1, alpha = 1 and D = 1 / pi on the whole hemisphere; with m = 0 and N = V = L the formula is
    ambient albedo + I ((1 - F0) albedo + pi (1 / pi) G F0 / (4 + 1e-6)), G = 1, F = F0 = 0.04 ((1 - V.H)^5 = 0)."""
    verts = R.screen_verts([(10.0, 10.0, 1.0), (30.0, 10.0, 1.0), (10.0, 30.0, 1.0)], 64, 48)
    # the face fills its samples; put eye and light on the normal through the sample's point: use the restatement's own pieces
    case = dict(verts=verts, faces=np.array([[0, 1, 2]], dtype=np.int32), shading="pbr_flat", lights=np.array([[0.0, 0.0, -1.0, 0.7]]), ambient=0.2,
                uvs=np.zeros((1, 3, 2), dtype=np.float32), materials=[{"Kd": (0.8, 0.6, 0.4), "Pm": 0.0, "Pr": 1.0}])
    xy, iw = R.project(verts, R.SCREEN, 64, 48, R.SCREEN_NEAR)
    r = R.raster(xy, iw, case["faces"], 64, 48)
    smp = P.gather_samples(case, xy, iw, r["face_id"])
    centre = np.flatnonzero(smp["s"] == 16 * 64 + 16)[0]                  # sample (16, 16): nearly on the axis through the eye
    one = {k: a[centre:centre + 1] for k, a in smp.items()}
    images, _ = P.shade_pbr(case, R.SCREEN, one, 64, 48, 1)
    got = images["shaded"].reshape(-1, 4)[16 * 64 + 16, :3] / 255.0
    albedo = np.array([0.8, 0.6, 0.4], dtype=np.float32).astype(np.float64)
    # N = (0, 0, -1), V = -P / |P| with P = (x, y, 1) a little off the axis: cos = 1 / |P|
    p = np.array([(2 * 16.5 / 64 - 1), (1 - 2 * 16.5 / 48), 1.0])
    cos = 1 / np.linalg.norm(p)
    h = (np.array([0, 0, -1.0]) - p / np.linalg.norm(p))
    h /= np.linalg.norm(h)
    nh, vh = -h[2], float(-p / np.linalg.norm(p) @ h)
    F = 0.04 + 0.96 * (1 - vh) ** 5
    D = 1 / math.pi                                                            # alpha = 1: (nh^2 (1 - 1) + 1)^2 = 1
    G = 1.0 / (1.0 * 0.5 + 0.5) * cos / (cos * 0.5 + 0.5)
    want = 0.2 * albedo + 0.7 * ((1 - F) * albedo + math.pi * D * G * F / (4 * cos + 1e-6))
    assert nh > 0.9 and np.abs(got - want).max() <= 0.5 / 255 + 1e-9
    assert (images["roughness"].reshape(-1, 4)[16 * 64 + 16, :3] == 255).all() and (images["metallic"].reshape(-1, 4)[16 * 64 + 16, :3] == 0).all()


def test_bilinear_is_render_cases_tex_bilinear():
    rng = np.random.default_rng(3)
    for img in P.map_images():
        u, v = rng.uniform(-0.2, 1.2, 50), rng.uniform(-0.2, 1.2, 50)
        got = P.bilinear(img, u, v, np.float64)
        three = img if img.ndim == 3 else np.repeat(img[..., None], 3, 2)
        want = np.array([R.tex_bilinear(three, a, b) for a, b in zip(u, v)])
        assert np.array_equal(got, want[:, :got.shape[1]])


def test_white_sphere_does_not_clip():
    """The stated purpose of RIG_INTENSITY: a white sphere with metallic 0 under the default rig and ambient stays below 255."""
    v, f = R.icosphere(2)
    verts = v.astype(np.float32)
    for rough in (0.5, 1.0):
        case = dict(verts=verts, faces=f, shading="pbr", lights=pbr.three_light_rig(), ambient=_lib.RENDER_PBR_AMBIENT, uvs=None,
                    materials=[{"Kd": (1.0, 1.0, 1.0), "Pm": 0.0, "Pr": rough}])
        m = R.rig_matrix(verts.astype(np.float64), 45.0, 45.0, 32, 24)
        xy, iw = R.project(verts, m, 64, 48, R.RIG_NEAR)
        r = R.raster(xy, iw, f, 64, 48)
        images, _ = P.shade_pbr(case, m, P.gather_samples(case, xy, iw, r["face_id"]), 64, 48, 2)
        top = images["shaded"][..., :3].max()
        print("roughness", rough, "brightest level", top)
        assert 150 < top < 255


# ------------------------------------------------------------------ the measured gaps and the leave-out cap
def test_measured_gaps_are_the_recorded_ones():
    ng, tg, ig, share = P.measure()
    print("normal gap", ng, "tangent gap", tg, "image gaps", ig, "largest flagged share", share)
    assert ng <= P.NORMAL_GAP <= 1.05 * ng + 1e-12 and tg <= P.TANGENT_GAP <= 1.05 * tg + 1e-12
    assert ig == P.IMAGE_GAP
    text = open(os.path.join(REPO, "profiles", "render_pbr.txt")).read()
    for value in (f"{P.NORMAL_GAP:.2e}", f"{P.TANGENT_GAP:.2e}"):
        assert value in text, value
    assert P.IMAGE_BOUND == {p: max(1, 2 * g) for p, g in P.IMAGE_GAP.items()}


@pytest.mark.parametrize("name,grid,view", P.all_views())
def test_leave_out_cap_holds_for_the_restatement(name, grid, view):
    images, flagged, r = P.restated(name, grid, view)
    covered = r["face_id"] >= 0
    assert covered.sum() > 100 and not flagged[~covered].any()
    print(name, grid, view, "covered", int(covered.sum()), "flagged", int(flagged.sum()))
    assert flagged.sum() <= R.MAX_LEFT_OUT * covered.sum()
    assert r["unclear"].sum() <= R.MAX_LEFT_OUT * covered.sum()
    assert set(images) == set(P.PASSES) == set(_lib.RENDER_PASSES)


def test_cases_cover_what_they_are_for():
    assert sorted({len(P.case(n, "g64")["lights"]) for n in P.CASES}) == [0, 1, 3, 4]
    sizes = [(m.shape[1], m.shape[0]) for m in P.map_images()]
    assert sizes == [(5, 7), (8, 8), (3, 4), (6, 5)] and P.map_images()[2].min() == 0
    assert len(R.icosphere(2)[1]) == 320 and len(P.case("a_sphere", "g64")["matrices"]) == 8
    # inside out: every visible face is seen from behind its stored winding
    c = P.case("d_inside_out", "g64")
    xy, iw = R.project(c["verts"], c["matrices"][0], 64, 48, c["near"])
    r = R.raster(xy, iw, c["faces"], 64, 48)
    front_sign = -1 if np.linalg.det(np.asarray(c["matrices"][0])[[0, 1, 3]][:, :3]) < 0 else 1
    seen = np.unique(r["face_id"][r["face_id"] >= 0])
    assert len(seen) > 20 and all((-1 if R.setup(xy, iw, c["faces"], f)[2] else 1) * front_sign < 0 for f in seen)
    # the roughness clamp is reached, and the normal map tilts strongly
    im, _, _ = P.restated("b_quads", "g64")
    assert im["roughness"][..., 0][im["roughness"][..., 3] == 255].min() < 255 * P.MIN_ROUGHNESS
    t = P.map_images()[3].astype(np.float64) / 255 * 2 - 1
    assert (t[..., 2] / np.linalg.norm(t, axis=2)).min() < 0.6                     # tilted by more than 50 degrees somewhere


# ------------------------------------------------------------------ the gain ladder: its gap, its conditions, the faults it sees
def test_ladder_gap_is_the_recorded_one():
    gap, each = P.measure_ladder()
    print("float32 against float64 at the readout, levels:", gap, {k: v for k, v in each.items() if any(v.values())})
    assert gap == P.LADDER_GAP
    assert P.LADDER_BOUND == {p: max(1, 2 * g) for p, g in P.LADDER_GAP.items()} == {"shaded": 2, "geo": 1}
    text = open(os.path.join(REPO, "profiles", "render_pbr.txt")).read()
    assert f"ladder gap in uint8 levels {P.LADDER_GAP}" in text
    # the flag keeps a float32 dot product's 1e-7 under a tenth of half a level at the floor of the readout
    assert 1e-7 / P.EPS_NL <= 0.1 * 0.5 / P.LADDER_FLOOR and P.LADDER_GAINS == tuple(2.0 ** k for k in range(25))


@pytest.mark.parametrize("name,view", P.ladder_views())
def test_ladder_conditions_hold_for_the_restatement(name, view):
    """Conditions on the cases, not measurements: what the three flags leave out, what depth leaves unclear and what the ladder
    cannot read (exact zeros, and channels that clip at gain 1) stay under their caps for the float64 restatement alone."""
    c, ref = P.ladder_case(name), P.ladder_restated(name, view)
    res = P.ladder_compare(ref["levels"], ref)
    print(name, view, "covered", ref["n_covered"], "flagged", ref["n_flagged"], "unclear", int(ref["raster"]["unclear"].sum()),
          "read share", {p: round(res[p][1], 4) for p in res})
    assert ref["n_covered"] > 700 and c["ambient"] == 0.0 and c["shading"] == "pbr" and len(R.icosphere(2)[1]) == len(c["faces"]) == 320
    assert ref["n_flagged"] <= R.MAX_LEFT_OUT * ref["n_covered"]
    assert ref["raster"]["unclear"].sum() <= R.MAX_LEFT_OUT * ref["n_covered"]
    for p in P.LADDER_PASSES:
        assert res[p][0] == 0 and res[p][1] >= 0.95, (p, res[p][:2])


def test_ladder_cases_cover_what_they_are_for():
    names = list(P.LADDER_CASES)
    assert names[:6] == list(P.LADDER_MATERIALS) and len(P.ladder_views()) == 6 * 3 + 3 + 3 + 1
    assert [len(P.ladder_case(n)["lights"]) for n in names] == [4] * 8 + [1]
    assert [P.ladder_case(n)["grid"] for n in names] == ["g50"] * 7 + ["g64", "g50"] and P.GRIDS["g64"][2] == 2
    mapped = P.ladder_case("n_mapped")
    assert mapped["uvs"].shape == (320, 3, 2) and mapped["materials"][0]["normal_image"] is not None
    assert all(P.ladder_case(n).get("uvs") is None for n in names if n != "n_mapped")
    # the ladder reaches small values: the readouts use at least 12 distinct gains, the longest of them past 2^20
    gains = set()
    for n, k in P.ladder_views():
        ref = P.ladder_restated(n, k)
        for p, (_, _, used) in P.ladder_compare(ref["levels"], ref).items():
            gains |= set(int(g) for g in used)
    print("gain indices read", sorted(gains))
    assert len(gains) >= 12 and max(gains) > 20
    # a pixel of the supersampled case is read only where none of its samples clips: some gains below 255 are refused for that
    ref = P.ladder_restated("s_supersampled", 0)
    assert ((ref["levels"]["shaded"] < 255) & ~ref["unclipped"]["shaded"]).any()
    # the readout rule on a hand-made ladder: 100 -> 200 -> clipped; 40 at the last unclipped gain is under the floor; never unclipped
    lev = np.zeros((25, 3), dtype=np.uint8)
    lev[:, 0], lev[:, 1], lev[:, 2] = [100, 200] + [255] * 23, [0] * 24 + [40], 255
    got, want, read, k = P.ladder_readout(lev + (lev < 255), lev)
    assert want.tolist()[:2] == [200, 40] and got.tolist()[:2] == [201, 41] and read.tolist() == [True, False, False] and k.tolist()[:2] == [1, 24]


# per fault: the largest difference in levels (shaded, geo) under the comparison of the images at gain 1 (every case, grid and view of
# P.CASES, flagged pixels left out, as test_render_pbr_gpu.py compares them) and under the ladder, on the float64 restatement
FAULT_LEVELS = {"fresnel_pow4": ((1, 1), (70, 30)), "fresnel_pow6": ((1, 1), (43, 18)), "vh_unclamped": ((0, 0), (0, 0)),
                "geo_grey_133": ((0, 1), (0, 2)), "nv_floor_1e-2": ((2, 1), (147, 1)), "min_roughness_008": ((9, 0), (88, 0)),
                "drop_fourth_light": ((3, 3), (254, 252)), "f0_045": ((4, 4), (29, 8)), "f0_041": ((1, 1), (7, 2)),
                "spec_x095": ((11, 2), (13, 6)), "spec_x099": ((2, 1), (3, 2)), "spec_guard_1e-5": ((2, 1), (129, 1)),
                "k_direct": ((21, 2), (243, 22))}
UNSEEN_AT_GAIN_ONE = ("fresnel_pow4", "fresnel_pow6", "geo_grey_133", "f0_041")     # the gap the ladder closes; update deliberately if the cases change


@pytest.mark.parametrize("fault", P.FAULTS)
def test_ladder_sees_the_fault(fault):
    assert set(FAULT_LEVELS) == set(P.FAULTS)
    old = {p: 0 for p in P.LADDER_PASSES}
    for n, g, k in P.all_views():
        c = P.case(n, g)
        Ws, Hs, ss = P.GRIDS[g]
        want, flagged, _ = P.restated(n, g, k)
        got, _ = P.shade_pbr(c, c["matrices"][k], P.gathered(n, g, k)[0], Ws, Hs, ss, fault=fault)
        keep = ~flagged.reshape(Hs // ss, ss, Ws // ss, ss).any((1, 3))
        for p in old:
            old[p] = max(old[p], int(np.abs(got[p].astype(np.int64) - want[p])[keep].max(initial=0)))
        assert all(np.array_equal(got[p], want[p]) for p in P.PASSES if p not in old)          # a fault of the light model only
    new, each = P.measure_ladder(fault, np.float64)
    seen = [k for k, v in each.items() if any(v[p] > P.LADDER_BOUND[p] for p in v)]
    print(fault, "images at gain 1:", old, "bound", {p: P.IMAGE_BOUND[p] for p in old}, "ladder:", new, "bound", P.LADDER_BOUND, "seen on", len(seen), "views")
    assert ((old["shaded"], old["geo"]), (new["shaded"], new["geo"])) == FAULT_LEVELS[fault]
    if fault in P.INERT_FAULTS:
        # H = normalize(L + V) lies between V and L, so 0 <= V.H <= 1 whenever H exists: the clamp never acts, an equivalent mutant
        assert not any(old.values()) and not any(new.values())
    else:
        assert seen and (fault != "fresnel_pow4" or all(("m0_black_dielectric", k) in seen for k in range(3)))
    assert all(old[p] <= P.IMAGE_BOUND[p] for p in old) == (fault in UNSEEN_AT_GAIN_ONE + P.INERT_FAULTS)


def test_fresnel_at_grazing_incidence():
    """One sample of a black dielectric (F0 = 0.04) on a face seen at 66 degrees from its normal, under a light near the mirror
    direction: (1 - F0)(1 - V.H)^5 is more than half of F, so the value is I NL pi D G F / (4 NL NV + 1e-6) with a Fresnel term
    that the exponent decides.  The restatement rounds 1 / w to float32 as the device does, 6e-8 relative, which moves the point by
    as much; D's denominator amplifies a change of N.H by 1 / dd < 20: a bound of 1e-5 relative leaves a factor of ten."""
    verts = R.screen_verts([(10.0, 10.0, 1.0), (30.0, 10.0, 16.0), (10.0, 30.0, 1.0)], 64, 48)      # receding steeply to the right
    a, b, c = verts.astype(np.float64)
    n = np.cross(b - a, c - a)
    n /= np.linalg.norm(n)
    d = np.array([2 * 16.5 / 64 - 1, 1 - 2 * 16.5 / 48, 1.0])                # the ray of sample (16, 16) from the eye at the origin
    n = -n if n @ d > 0 else n
    p = d * (n @ a) / (n @ d)
    v = -p / np.linalg.norm(p)
    mirror = (2 * (n @ v) * n - v) + np.array([0.02, -0.01, 0.015])          # a little off the mirror direction, so N.H < 1
    light = (mirror / np.linalg.norm(mirror)).astype(np.float32).astype(np.float64)
    case = dict(verts=verts, faces=np.array([[0, 1, 2]], dtype=np.int32), shading="pbr_flat", lights=np.array([[*light, 0.9]]), ambient=0.0,
                uvs=None, materials=[{"Kd": (0.0, 0.0, 0.0), "Pm": 0.0, "Pr": 0.5}])
    xy, iw = R.project(verts, R.SCREEN, 64, 48, R.SCREEN_NEAR)
    r = R.raster(xy, iw, case["faces"], 64, 48)
    smp = P.gather_samples(case, xy, iw, r["face_id"])
    at = np.flatnonzero(smp["s"] == 16 * 64 + 16)[0]
    one = {k: x[at:at + 1] for k, x in smp.items()}
    got = P.shade_pbr(case, R.SCREEN, one, 64, 48, 1, raw=True)["shaded"][0]
    h = light + v
    h /= np.linalg.norm(h)
    nl, nv, nh, vh = n @ light, n @ v, n @ h, v @ h
    schlick = 0.96 * (1 - vh) ** 5
    F = 0.04 + schlick
    a2, k = 0.5 ** 4, 0.5 ** 2 / 2
    D = a2 / (math.pi * (nh * nh * (a2 - 1) + 1) ** 2)
    G = nl / (nl * (1 - k) + k) * nv / (nv * (1 - k) + k)
    want = np.float32(0.9).astype(np.float64) * nl * math.pi * D * G * F / (4 * nl * nv + 1e-6)
    print("N.V", nv, "N.L", nl, "N.H", nh, "V.H", vh, "Schlick term / F", schlick / F, "value", want, "restated", got)
    assert schlick >= 0.5 * F and 0.3 < nv < 0.5 and 0.3 < nl < 0.5 and 0.2 < want < 1.0
    assert np.abs(got - want).max() <= 1e-5 * want
    for fault in ("fresnel_pow4", "fresnel_pow6"):
        wrong = P.shade_pbr(case, R.SCREEN, one, 64, 48, 1, raw=True, fault=fault)["shaded"][0]
        assert np.abs(wrong - want).min() > 0.2 * want, fault


# ------------------------------------------------------------------ the MTL parser, the rig, the command line
MTL = """# comment
newmtl body
Kd 0.5 0.25 1
Pm 0.75
Pr 0.125   # trailing
map_Kd -s 1 1 1 textures/albedo.png
map_Pm textures/metallic.png
map_Pr -o 0 0 0 textures/roughness.png
map_Bump -bm 1.000000 textures/normal.png
newmtl glass
norm other.png
Pm x
newmtl plain
Kd 1 1 1
"""


def test_mtl_parser():
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        m = pbr.parse_pbr_mtl(MTL)
    assert list(m) == ["body", "glass", "plain"] and len(w) == 1 and "Pm" in str(w[0].message)
    assert m["body"] == {"Pm": 0.75, "Pr": 0.125, "map_Pm": "textures/metallic.png", "map_Pr": "textures/roughness.png", "map_Bump": "textures/normal.png"}
    assert m["glass"] == {"map_Bump": "other.png"} and m["plain"] == {}
    assert pbr.parse_pbr_mtl("bump a.png\n") == {} and pbr.parse_pbr_mtl("newmtl a\nbump b.png\nmap_bump c.png") == {"a": {"map_Bump": "c.png"}}


def test_load_pbr_maps_and_pack(tmp_path):
    import torch
    from sin3dm_amd.data import obj_io
    from sin3dm_amd.encoding.isosurface import png_bytes
    albedo, metallic, roughness, normal = P.map_images()
    os.makedirs(tmp_path / "textures")
    for name, img in (("albedo", albedo), ("metallic", metallic), ("normal", normal)):
        open(tmp_path / "textures" / (name + ".png"), "wb").write(png_bytes(img))
    open(tmp_path / "textures" / "roughness.png", "wb").write(b"not a png")
    open(tmp_path / "m.mtl", "w").write(MTL)
    open(tmp_path / "o.obj", "w").write("mtllib m.mtl\nv 0 0 0\nv 1 0 0\nv 0 1 0\nvt 0 0\nvt 1 0\nvt 0 1\nusemtl body\nf 1/1 2/2 3/3\nusemtl plain\nf 1/1 3/3 2/2\n")
    before = sorted(obj_io.load_obj(str(tmp_path / "o.obj")))
    mesh = obj_io.load_obj(str(tmp_path / "o.obj"))
    assert sorted(mesh) == before == ["face_mat", "faces", "materials", "n_degenerate", "uvs", "verts"]
    try:
        import PIL  # noqa: F401
        have_pil = True
    except ImportError:
        have_pil = False
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        mats = pbr.load_pbr_maps(str(tmp_path / "o.obj"), mesh["materials"])
    body, plain = mats[0][1], mats[1][1]
    assert body["Pm"] == 0.75 and body["Pr"] == 0.125 and "Pm" not in plain and plain["normal_image"] is None
    assert body["roughness_image"] is None and any("roughness.png" in str(x.message) for x in w)          # unreadable: the factor, with a warning
    if have_pil:
        assert np.array_equal(body["metallic_image"], metallic) and np.array_equal(body["normal_image"], normal)
    info = pbr.has_pbr_info([body, plain])
    assert info["metallic"] and info["roughness"] and info["normal"] == have_pil
    # the table: offsets in order, one byte per texel for the scalar maps, the factors
    body.update(image=albedo, metallic_image=metallic, roughness_image=None, normal_image=normal)
    table, factors, images, nbytes = pbr.pack_pbr_materials([body, plain], torch.device("cpu"))
    assert table.dtype == np.int64 and table.shape == (2, 4, 3) and factors.dtype == np.float32
    assert table[0].tolist() == [[0, 5, 7], [105, 8, 8], [0, 0, 0], [169, 6, 5]] and not table[1].any() and nbytes == 169 + 90 == images.numel()
    assert factors.tolist() == [[0.5, 0.25, 1.0, 0.75, 0.125], [1.0, 1.0, 1.0, 0.0, 0.5]]
    assert np.array_equal(images[105:169].numpy().reshape(8, 8), metallic)
    with pytest.raises(ValueError, match="normal_image"):
        pbr.pack_pbr_materials([{"normal_image": metallic}], torch.device("cpu"))


def test_three_light_rig():
    rig = pbr.three_light_rig()
    assert rig.shape == (3, 4) and np.allclose(np.linalg.norm(rig[:, :3], axis=1), 1)
    assert np.allclose(rig[:, 3] / rig[0, 3], [1, 0.5, 0.1]) and rig[0, 3] == _lib.RENDER_RIG_INTENSITY == pbr.RIG_INTENSITY
    # blender_render_pbr.py:143-149: (radius, 0, height), (0, radius, 0.6 height), (0, -radius, height) with z up; stored meshes are y up,
    # turned by camera.ROT_X90 (x, y, z) -> (x, -z, y)
    want = np.array([[2.0, 10.0, 0.0], [0.0, 6.0, -2.0], [0.0, 10.0, 2.0]])
    assert np.allclose(rig[:, :3], want / np.linalg.norm(want, axis=1, keepdims=True))
    assert np.allclose(P.rig_lights(3), rig)
    assert np.allclose(pbr.three_light_rig(4, 5, 2.0)[1], [0, 3 / 5, -4 / 5, 1.0])
    with pytest.raises(ValueError):
        pbr.three_light_rig(0.0, 0.0)
    header = open(os.path.join(REPO, "include", "sin3dm_hip.h")).read()
    assert float(re.search(r"#define S3D_RENDER_RIG_INTENSITY (.+)f", header).group(1)) == pbr.RIG_INTENSITY
    assert f"RIG_INTENSITY = {pbr.RIG_INTENSITY}" in open(os.path.join(REPO, "DESIGN.md")).read()


def test_cli_arguments():
    a = render_pbr.parse_args(["-s", "dir/object.obj"])
    assert (a.output_path, a.azimuth, a.elevation, a.rot, a.scale, a.image_resolution, a.shading, a.supersample) == \
        (os.path.join("dir", "object.png"), 45.0, 45.0, 0.0, 1.0, (512, 512), "smooth", 2)
    b = render_pbr.parse_args(["--mesh_path", "m.obj", "-o", "out", "-az", "10", "-el", "100", "--rot", "30", "--scale", "0.5", "--image_resolution", "64",
                               "48", "--shading", "flat", "--supersample", "1"])
    assert (b.output_path, b.azimuth, b.elevation, b.rot, b.scale, b.image_resolution, b.shading, b.supersample) == \
        ("out.png", 10.0, 100.0, 30.0, 0.5, (64, 48), "flat", 1)
    for el in ("0", "180", "-180", "360"):
        with pytest.raises(ValueError, match="axis"):
            render_pbr.parse_args(["-s", "m.obj", "-el", el])
    for bad in ([], ["-s", "m.obj", "--shading", "phong"], ["-s", "m.obj", "--supersample", "9"], ["-s", "m.obj", "--image_resolution", "0", "4"],
                ["-s", "m.obj", "--scale", "0"]):
        with pytest.raises(SystemExit):
            render_pbr.parse_args(bad)
    # the camera of the reference's formula, the mesh turned about the vertical axis
    from sin3dm_amd.rendering import camera
    view, world = render_pbr.pbr_view([-1, -1, -1], [1, 1, 1], 30.0, 60.0, (64, 48), rot=90.0)
    eye = P.eye_of(view.matrix)
    model = np.linalg.inv(world) * 1.03
    assert np.allclose(world @ np.array([0, 1.0, 0]), [0, 0, 1]) and np.allclose(world @ np.array([1.0, 0, 0]), [0, 1, 0])
    assert np.allclose(eye, model @ camera.camera_position(30.0, 60.0))
    from sin3dm_amd.rendering import render_multiview as rm
    assert rm.parse_args(["-s", "m", "-o", "o"]).shading == "flat" and rm.parse_args(["-s", "m", "-o", "o", "--shading", "pbr"]).shading == "pbr"
    from sin3dm_amd import sample
    assert sample.render_shading("") == "" and sample.render_shading("pbr") == "pbr"
    with pytest.raises(ValueError, match="phong"):
        sample.render_shading("phong")


# ------------------------------------------------------------------ header, binding, argument checks
def test_header_binding_and_constants_agree():
    import sin3dm_amd.rendering as rd
    for name in ("vertex_normals", "face_tangents", "render_views"):
        assert callable(getattr(rd, name)), name
    lib = _lib.load()
    header = open(os.path.join(REPO, "include", "sin3dm_hip.h")).read()
    for name in ENTRY_POINTS:
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
        decl = re.search(r"S3D_API int " + name + r"\(([^;]*)\);", header)
        assert decl, name
        assert len(decl.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name
    assert int(re.search(r"#define S3D_ABI_VERSION (\d+)", header).group(1)) == _lib.ABI_VERSION == lib.s3d_abi_version() == 13

    def define(name):
        return re.search(r"#define " + name + r" (.+)", header).group(1).strip()
    assert int(define("S3D_RENDER_MAX_LIGHTS")) == _lib.RENDER_MAX_LIGHTS == 4
    assert int(define("S3D_RENDER_PBR_MAX_MATERIALS")) == _lib.RENDER_PBR_MAX_MATERIALS
    assert float(define("S3D_RENDER_MIN_ROUGHNESS").rstrip("f")) == _lib.RENDER_MIN_ROUGHNESS == P.MIN_ROUGHNESS == 0.089
    assert float(define("S3D_RENDER_PBR_AMBIENT").rstrip("f")) == _lib.RENDER_PBR_AMBIENT == P.AMBIENT
    assert define("S3D_RENDER_GEO_GREY") == "(134.0f / 255.0f)"
    for i, name in enumerate(_lib.RENDER_PASSES):
        assert int(define("S3D_RENDER_PASS_" + name.upper())) == i
    assert _lib.RENDER_PASSES == P.PASSES


def test_argument_errors_launch_nothing():
    """Validation happens before any launch, so it can be checked without a GPU (the pointers are never read)."""
    lib = _lib.load()
    fake = C.c_void_p(256)
    eye4 = (C.c_float * 16)(*np.eye(4, dtype=np.float32).reshape(-1))
    inv, uns = _lib.ERR_INVALID, _lib.ERR_UNSUPPORTED
    assert lib.s3d_pbr_vertex_normals(fake, -1, fake, 1, fake, fake, fake, None) == inv
    assert lib.s3d_pbr_vertex_normals(fake, 3, None, 1, fake, fake, fake, None) == inv and b"corner order" in lib.s3d_last_error()
    assert lib.s3d_pbr_vertex_normals(fake, 3, fake, 1, fake, None, fake, None) == inv
    assert lib.s3d_pbr_vertex_normals(None, 0, None, 0, None, None, None, None) == 0
    assert lib.s3d_pbr_face_tangents(fake, 3, fake, 1, None, fake, None) == inv and b"pbr_face_tangents" in lib.s3d_last_error()
    assert lib.s3d_pbr_face_tangents(fake, 3, fake, 1 << 40, fake, fake, None) == inv
    assert lib.s3d_pbr_face_tangents(None, 0, None, 0, None, None, None) == 0
    lights = (C.c_float * 20)(*([0.0, 0.0, 1.0, 1.0] * 5))
    eye = (C.c_float * 3)(0, 0, 0)
    one = (C.c_int64 * 12)(0, 4, 4, 0, 0, 0, 0, 0, 0, 0, 0, 0)
    fac = (C.c_float * 5)(1, 1, 1, 0, 0.5)

    def shade(ws=64, hs=48, ss=2, uv=fake, tangents=None, table=None, factors=None, n_mats=0, images=None, image_bytes=0, n_lights=1, li=lights,
              ambient=0.1, pas=0, e=eye, rgba=fake):
        return lib.s3d_pbr_shade(fake, fake, fake, 3, fake, 1, fake, ws, hs, ss, eye4, None, uv, None, None, None, n_mats, images, image_bytes,
                                        None, tangents, table, factors, e, li, n_lights, ambient, pas, rgba, None)
    assert shade(n_lights=5) == inv and b"lights" in lib.s3d_last_error()
    assert shade(n_lights=-1) == inv and shade(li=None) == inv
    assert shade(pas=6) == inv and b"pass" in lib.s3d_last_error() and shade(pas=-1) == inv
    assert shade(tangents=fake, uv=None) == inv and b"tangents without uv" in lib.s3d_last_error()
    assert shade(table=one, factors=fac, n_mats=1, images=fake, image_bytes=47) == inv and b"run past" in lib.s3d_last_error()
    assert shade(table=one, factors=None, n_mats=1, images=fake, image_bytes=48) == inv
    assert shade(table=one, factors=fac, n_mats=0, images=fake, image_bytes=48) == inv
    assert shade(table=one, factors=fac, n_mats=_lib.RENDER_PBR_MAX_MATERIALS + 1, images=fake, image_bytes=48) == uns
    assert shade(ss=0) == inv and b"supersample" in lib.s3d_last_error() and shade(ws=50, hs=37) == inv
    assert shade(e=None) == inv and shade(ambient=float("nan")) == inv and shade(rgba=None) == inv
    assert shade(e=(C.c_float * 3)(float("inf"), 0, 0)) == inv
    bad = (C.c_int64 * 12)(0, 4, 4, 16, 70000, 1, 0, 0, 0, 0, 0, 0)
    assert shade(table=bad, factors=fac, n_mats=1, images=fake, image_bytes=1 << 20) == inv and b"metallic" in lib.s3d_last_error()
