"""The yardstick of the PBR renders (s3d_render_pbr.hip): a NumPy restatement of the vertex normals, the face
tangents and the shading formula, and the procedural cases.  Projection, the integer raster stage and the scalar bilinear lookup
are those of tests/render_cases.py; everything here is written once for a number type `dt` and evaluated twice, in float64 (the
reference) and in float32 with the same order of operations (the measure of what float32 arithmetic alone can cost).

Tolerances are measured, not chosen: NORMAL_GAP / TANGENT_GAP are the largest relative gaps between the two evaluations over
every case (|x32 - x64| / |x64| per vector), IMAGE_GAP the largest gap per pass in uint8 levels (measure(), held by
test_render_pbr_host.py, recorded in profiles/render_pbr.txt).  The device is held to ten times the relative gaps and to
max(1, 2 * ceil(gap)) levels: a specular peak amplifies an input error in a way the flat shader does not.

Ill-conditioned samples.  Two places of the formula are not continuous in a usable way: the fallback from the smooth to the flat
normal (dot(mix, flat) <= 0: a jump) and N.V near its floor 1e-4 (the relative error of a float32 dot product of unit vectors,
about 1e-7 absolute, is 1e-3 there, under a specular term that divides by it).  A sample within EPS_FLIP of the first boundary or
within EPS_NV of the second is flagged, and pixels holding one are left out; the share of flagged samples is capped at
render_cases.MAX_LEFT_OUT per case, and the cases are chosen so that the restatement meets the cap.

The gain ladder (at the end of this file) reads the light model's float value out of the uint8 images: the same view under light
intensities scaled by 2^0 ... 2^24, each pixel-channel compared at the largest gain that does not clip, within LADDER_BOUND levels
of a level in [128, 255).  There a third flag joins the two: a sample with |N.L| < EPS_NL for a light, where the dot product's
1e-7 absolute error is a large relative error of a value proportional to it, which a high gain magnifies.  FAULTS names wrong
light models; test_render_pbr_host.py shows that the ladder sees each of them and which of them the images at gain 1 do not."""
import functools
import math

import numpy as np

import render_cases as R

PASSES = ("shaded", "albedo", "metallic", "roughness", "normal", "geo")
MIN_ROUGHNESS, GEO_GREY, NV_FLOOR = 0.089, 134.0 / 255.0, 1e-4
AMBIENT = 0.1
EPS_FLIP = 1e-5                                              # ten times the error of a float32 dot product of unit vectors
EPS_NV = 1e-3                                                # ten times NV_FLOOR: beyond it a 1e-7 error is under 1e-4 relative
EPS_NL = 3e-4                                                # the gain ladder only: 1e-7 / EPS_NL is under a tenth of half a level at 64 (>= 1.3e-4)
# measured by measure() (profiles/render_pbr.txt); the device bounds derive from them
NORMAL_GAP = 9.9e-08                                         # measured 9.885e-08
TANGENT_GAP = 1.03e-07                                       # measured 1.024e-07
IMAGE_GAP = {"shaded": 0, "albedo": 1, "metallic": 1, "roughness": 0, "normal": 0, "geo": 0}     # uint8 levels, measured
NORMAL_BOUND, TANGENT_BOUND = 10 * NORMAL_GAP, 10 * TANGENT_GAP
IMAGE_BOUND = {p: max(1, 2 * int(math.ceil(g))) for p, g in IMAGE_GAP.items()}


# ------------------------------------------------------------------ restatement: normals and tangents
def _f32(x, dt):
    """float32 data as the number type of the evaluation"""
    return np.asarray(x, dtype=np.float32).astype(dt)


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def _dot(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def _normalize(v):
    """(v / |v| or v itself, ok) with ok = the squared length is positive and finite"""
    l2 = _dot(v, v)
    ok = (l2 > 0) & np.isfinite(l2)
    ln = np.sqrt(np.where(ok, l2, 1))
    return np.where(ok[..., None], v / ln[..., None], v), ok


def vertex_normals(verts, faces, dt=np.float64):
    """[V, 3]: the normalised sum of cross(b - a, c - a) over the faces of a vertex in ascending corner order; zeros where no
    face contributes or the sum has no direction."""
    v = _f32(verts, dt).reshape(-1, 3)
    acc = np.zeros((len(v), 3), dtype=dt)
    for f in np.asarray(faces).reshape(-1, 3):
        if (f < 0).any() or (f >= len(v)).any():
            continue
        n = _cross(v[f[1]] - v[f[0]], v[f[2]] - v[f[0]])
        for j in range(3):                                       # ascending corner 3 f + j: ascending per vertex
            acc[f[j]] = acc[f[j]] + n
    out, ok = _normalize(acc)
    return np.where(ok[:, None], out, 0).astype(dt)


def face_tangents(verts, faces, uvs, dt=np.float64):
    """[F, 2, 3]: (T, B) per face; zeros where det == 0 or the result is not finite."""
    v, q = _f32(verts, dt).reshape(-1, 3), _f32(uvs, dt).reshape(-1, 3, 2)
    f = np.asarray(faces).reshape(-1, 3)
    e1, e2 = v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]]
    du1, dv1 = q[:, 1, 0] - q[:, 0, 0], q[:, 1, 1] - q[:, 0, 1]
    du2, dv2 = q[:, 2, 0] - q[:, 0, 0], q[:, 2, 1] - q[:, 0, 1]
    det = du1 * dv2 - du2 * dv1
    safe = np.where(det != 0, det, 1)
    T = (e1 * dv2[:, None] - e2 * dv1[:, None]) / safe[:, None]
    B = (e2 * du1[:, None] - e1 * du2[:, None]) / safe[:, None]
    out = np.stack([T, B], 1)
    ok = (det != 0) & np.isfinite(out.astype(np.float32)).all((1, 2))
    return np.where(ok[:, None, None], out, 0).astype(dt)


def relative_gap(x32, x64):
    """largest |x32 - x64| / |x64| over the vectors (last axis) that are not zero in the reference"""
    x32, x64 = np.asarray(x32, dtype=np.float64).reshape(-1, 3), np.asarray(x64, dtype=np.float64).reshape(-1, 3)
    ln = np.linalg.norm(x64, axis=1)
    keep = ln > 0
    assert not x32[~keep].any()
    return float((np.linalg.norm(x32 - x64, axis=1)[keep] / ln[keep]).max(initial=0.0))


# ------------------------------------------------------------------ restatement: shading
def bilinear(img, u, v, dt):
    """render_cases.tex_bilinear for arrays of (u, v), any channel count, in the number type dt: [S, C] in [0, 1]"""
    img = np.asarray(img)
    img = img[..., None] if img.ndim == 2 else img
    H, W = img.shape[:2]
    x = np.minimum(np.maximum(u * dt(W) - dt(0.5), dt(-1.0)), dt(W))
    y = np.minimum(np.maximum((dt(1.0) - v) * dt(H) - dt(0.5), dt(-1.0)), dt(H))
    xf, yf = np.floor(x), np.floor(y)
    fx, fy = (x - xf)[:, None], (y - yf)[:, None]
    x0, x1 = np.clip(xf.astype(np.int64), 0, W - 1), np.clip(xf.astype(np.int64) + 1, 0, W - 1)
    y0, y1 = np.clip(yf.astype(np.int64), 0, H - 1), np.clip(yf.astype(np.int64) + 1, 0, H - 1)
    c = img.astype(dt)
    top = c[y0, x0] + fx * (c[y0, x1] - c[y0, x0])
    bot = c[y1, x0] + fx * (c[y1, x1] - c[y1, x0])
    return (top + fy * (bot - top)) / dt(255.0)


def eye_of(matrix):
    m = np.asarray(matrix, dtype=np.float64).reshape(4, 4)[[0, 1, 3]]
    return -np.linalg.solve(m[:, :3], m[:, 3])


def gather_samples(case, xy, iw, face_id):
    """The covered samples in row order: dict of s (flat sample index), f, E int64 [S, 3], w float64 [S, 3] (1 / w of the ordered
    corners), vid [S, 3] (their vertices), swapped [S]."""
    Hs, Ws = face_id.shape
    rec, cache = [], {}
    for j in range(Hs):
        for i in range(Ws):
            f = int(face_id[j, i])
            if f < 0:
                continue
            if f not in cache:
                st, c, swapped = R.setup(xy, iw, case["faces"], f)
                assert st == R.OK
                cache[f] = (R.edges(c), c, swapped)
            ed, c, swapped = cache[f]
            E = R.edge_values(ed, i * R.SUB + R.HALF, j * R.SUB + R.HALF)
            rec.append((j * Ws + i, f, E, [p[2] for p in c], [p[3] for p in c], swapped))
    return {"s": np.array([r[0] for r in rec], dtype=np.int64), "f": np.array([r[1] for r in rec], dtype=np.int64),
            "E": np.array([r[2] for r in rec], dtype=np.int64).reshape(-1, 3), "w": np.array([r[3] for r in rec], dtype=np.float64).reshape(-1, 3),
            "vid": np.array([r[4] for r in rec], dtype=np.int64).reshape(-1, 3), "swapped": np.array([r[5] for r in rec], dtype=bool)}


FAULTS = ("fresnel_pow4", "fresnel_pow6", "vh_unclamped", "geo_grey_133", "nv_floor_1e-2", "min_roughness_008", "drop_fourth_light",
          "f0_045", "f0_041", "spec_x095", "spec_x099", "spec_guard_1e-5", "k_direct")
INERT_FAULTS = ("vh_unclamped",)                             # H lies between V and L, so 0 <= V.H <= 1 already: the clamp never acts


def shade_pbr(case, matrix, smp, Ws, Hs, ss, dt=np.float64, fault=None, raw=False):
    """({pass: rgba uint8 [H, W, 4]}, flagged bool [Hs, Ws]) of one view of a case on gathered samples, in the number type dt.
    fault: one of FAULTS, a deliberately wrong light model (the unfaulted path does not read it).  raw=True: instead, a dict of
    the per-sample values before the clamp, "shaded" and "geo" [S, 3] in dt, with "flagged" [S] (the two rules above) and
    "grazing" [S] (|N.L| < EPS_NL for a light, under either normal): what the gain ladder scales."""
    assert fault is None or fault in FAULTS, fault
    S = len(smp["s"])
    verts, faces = _f32(case["verts"], dt).reshape(-1, 3), np.asarray(case["faces"]).reshape(-1, 3)
    shading = case["shading"]
    is_pbr = shading in ("pbr", "pbr_flat")
    m4 = np.asarray(matrix, dtype=np.float64)
    front_sign = -1 if np.linalg.det(m4[[0, 1, 3]][:, :3]) < 0 else 1
    f, vid, swapped = smp["f"], smp["vid"], smp["swapped"]
    n = smp["E"].astype(dt) * smp["w"].astype(np.float32).astype(dt)
    b = n / ((n[:, 0] + n[:, 1]) + n[:, 2])[:, None]
    b0, b1, b2 = b[:, 0:1], b[:, 1:2], b[:, 2:3]
    # the flat normal in the face's own order, towards the camera
    own = faces[f] if S else np.zeros((0, 3), dtype=np.int64)
    nf, has_flat = _normalize(_cross(verts[own[:, 1]] - verts[own[:, 0]], verts[own[:, 2]] - verts[own[:, 0]]))
    nf = np.where(has_flat[:, None], nf, 0)
    front = np.where(swapped, -1, 1) * front_sign > 0
    nf = np.where(front[:, None], nf, -nf)
    N = nf
    flagged = np.zeros(S, dtype=bool)
    if shading in ("smooth", "pbr"):
        vn = vertex_normals(case["verts"], faces, dt).astype(np.float32).astype(dt)
        c0, c1, c2 = vn[vid[:, 0]], vn[vid[:, 1]], vn[vid[:, 2]]
        any_zero = ~c0.any(1) | ~c1.any(1) | ~c2.any(1)
        mix, ok = _normalize(b0 * c0 + b1 * c1 + b2 * c2)
        mix = np.where(front[:, None], mix, -mix)
        d = _dot(mix, nf)
        usable = has_flat & ~any_zero & ok
        N = np.where((usable & (d > 0))[:, None], mix, nf)
        flagged |= usable & (np.abs(d) < EPS_FLIP)
    # the material
    albedo, metal, rough = np.ones((S, 3), dtype=dt), np.zeros(S, dtype=dt), np.full(S, 0.5, dtype=dt)
    mats, uvs = case.get("materials"), case.get("uvs")
    fmat = np.asarray(case["face_mat"])[f] if case.get("face_mat") is not None else np.zeros(S, dtype=np.int64)
    uv = None
    if uvs is not None:
        q = _f32(uvs, dt).reshape(-1, 3, 2)[f]
        k1, k2 = np.where(swapped, 2, 1), np.where(swapped, 1, 2)                # corner k of the ordered triangle in the face's own order
        rows = np.arange(S)
        uv = b0 * q[:, 0] + b1 * q[rows, k1] + b2 * q[rows, k2]
    N_map = N
    if is_pbr:
        tang = face_tangents(case["verts"], faces, uvs, dt).astype(np.float32).astype(dt) if uvs is not None else None
        for mi, mat in enumerate(mats or []):
            sel = fmat == mi
            if not sel.any():
                continue
            albedo[sel] = _f32(mat.get("Kd", (1.0, 1.0, 1.0)), dt)
            metal[sel], rough[sel] = _f32(mat.get("Pm", 0.0), dt), _f32(mat.get("Pr", 0.5), dt)
            if uv is None:
                continue
            if mat.get("image") is not None:
                albedo[sel] = bilinear(mat["image"], uv[sel, 0], uv[sel, 1], dt)
            if mat.get("metallic_image") is not None:
                metal[sel] = bilinear(mat["metallic_image"], uv[sel, 0], uv[sel, 1], dt)[:, 0]
            if mat.get("roughness_image") is not None:
                rough[sel] = bilinear(mat["roughness_image"], uv[sel, 0], uv[sel, 1], dt)[:, 0]
            if mat.get("normal_image") is not None:
                T, B = tang[f[sel], 0], tang[f[sel], 1]
                Ns = N[sel]
                Tp, ok = _normalize(T - Ns * _dot(Ns, T)[:, None])
                Bp = _cross(Ns, Tp)
                sg = np.where(_dot(Bp, B) < 0, dt(-1.0), dt(1.0))[:, None]
                tx = dt(2.0) * bilinear(mat["normal_image"], uv[sel, 0], uv[sel, 1], dt) - dt(1.0)
                Nm, ok2 = _normalize(tx[:, 0:1] * Tp + tx[:, 1:2] * (sg * Bp) + tx[:, 2:3] * Ns)
                use = ok & ok2 & has_flat[sel]
                N_map = N_map.copy()
                N_map[sel] = np.where(use[:, None], Nm, Ns)
    else:
        vcol = case.get("vertex_colors")
        if vcol is not None:
            c = _f32(vcol, dt)
            albedo = b0 * c[vid[:, 0]] + b1 * c[vid[:, 1]] + b2 * c[vid[:, 2]]
        elif mats:
            for mi, mat in enumerate(mats):
                sel = fmat == mi
                if not sel.any():
                    continue
                albedo[sel] = _f32(mat.get("Kd", (1.0, 1.0, 1.0)), dt)
                if mat.get("image") is not None and uv is not None:
                    albedo[sel] = bilinear(mat["image"], uv[sel, 0], uv[sel, 1], dt)
    # the light model
    eye = _f32(eye_of(m4), dt)
    lights = _f32(case["lights"], dt).reshape(-1, 4)
    ambient = _f32(case.get("ambient", AMBIENT), dt)
    P = b0 * verts[vid[:, 0]] + b1 * verts[vid[:, 1]] + b2 * verts[vid[:, 2]]
    pi = dt(3.14159265358979323846)

    if fault == "drop_fourth_light":
        lights = lights[:3]
    nv_floor = dt(1e-2) if fault == "nv_floor_1e-2" else dt(NV_FLOOR)
    min_rough = dt(0.08) if fault == "min_roughness_008" else dt(MIN_ROUGHNESS)
    f0_base = dt({"f0_045": 0.045, "f0_041": 0.041}.get(fault, 0.04))
    spec_guard = dt(1e-5) if fault == "spec_guard_1e-5" else dt(1e-6)
    grazing = np.zeros(S, dtype=bool)

    def lit(Nn, alb, met, rgh):
        nonlocal flagged, grazing
        Vv, ok = _normalize(eye - P)
        Vv = np.where(ok[:, None], Vv, Nn)
        nv_raw = _dot(Nn, Vv)
        flagged = flagged | (np.abs(nv_raw.astype(np.float64) - NV_FLOOR) < EPS_NV)
        NV = np.maximum(nv_raw, nv_floor)
        r = np.minimum(np.maximum(rgh, min_rough), dt(1.0))
        alpha = r * r
        a2, kk = alpha * alpha, dt(0.5) * alpha
        if fault == "k_direct":
            kk = (r + dt(1.0)) * (r + dt(1.0)) / dt(8.0)
        gv = NV / (NV * (dt(1.0) - kk) + kk)
        F0 = f0_base * (dt(1.0) - met)[:, None] + alb * met[:, None]
        out = ambient * alb
        for L in lights:
            nl_raw = _dot(Nn, L[:3])
            grazing = grazing | (np.abs(nl_raw.astype(np.float64)) < EPS_NL)
            NL = np.maximum(nl_raw, dt(0.0))
            Hh, ok = _normalize(L[:3] + Vv)
            Hh = np.where(ok[:, None], Hh, Nn)
            NH, VH = _dot(Nn, Hh), np.minimum(np.maximum(_dot(Vv, Hh), dt(0.0)), dt(1.0))
            if fault == "vh_unclamped":
                VH = _dot(Vv, Hh)
            x = dt(1.0) - VH
            x2 = x * x
            x5 = x2 * x2 * x
            if fault in ("fresnel_pow4", "fresnel_pow6"):
                x5 = x2 * x2 if fault == "fresnel_pow4" else x2 * x2 * x2
            dd = NH * NH * (a2 - dt(1.0)) + dt(1.0)
            D = a2 / (pi * dd * dd)
            G = NL / (NL * (dt(1.0) - kk) + kk) * gv
            spec = pi * D * G / (dt(4.0) * NL * NV + spec_guard)
            if fault in ("spec_x095", "spec_x099"):
                spec = spec * dt(0.95 if fault == "spec_x095" else 0.99)
            w = L[3] * NL
            Fk = F0 + (dt(1.0) - F0) * x5[:, None]
            out = out + w[:, None] * ((dt(1.0) - Fk) * (dt(1.0) - met)[:, None] * alb + spec[:, None] * Fk)
        return out

    grey = lambda x: np.repeat(x[:, None], 3, 1)              # noqa: E731
    geo_grey = 133.0 / 255.0 if fault == "geo_grey_133" else GEO_GREY
    values = {"shaded": lit(N_map, albedo, metal, rough), "albedo": albedo, "metallic": grey(metal), "roughness": grey(rough),
              "normal": dt(0.5) * N_map + dt(0.5),
              "geo": lit(N, np.full((S, 3), geo_grey, dtype=np.float32).astype(dt), np.zeros(S, dtype=dt), np.full(S, 0.5, dtype=dt))}
    if raw:
        assert values["shaded"].dtype == dt and values["geo"].dtype == dt
        return {"shaded": values["shaded"], "geo": values["geo"], "flagged": flagged, "grazing": grazing}
    images = {}
    for name, val in values.items():
        assert val.dtype == dt, (name, val.dtype)
        images[name] = resolve(val, smp, Ws, Hs, ss, dt)
    flag = np.zeros(Hs * Ws, dtype=bool)
    flag[smp["s"][flagged]] = True
    return images, flag.reshape(Hs, Ws)


def resolve(val, smp, Ws, Hs, ss, dt):
    """rgba uint8 [H, W, 4] of per-sample values [S, 3]: clamped to [0, 1], the mean over a pixel's covered samples in row order,
    uint8(255 x + 0.5); alpha the covered share.  The last step of shade_pbr, in the number type dt."""
    H, W = Hs // ss, Ws // ss
    cov = np.zeros(Hs * Ws, dtype=bool)
    cov[smp["s"]] = True
    n_cov = cov.reshape(H, ss, W, ss).sum((1, 3))
    full = np.zeros((Hs * Ws, 3), dtype=dt)
    full[smp["s"]] = np.minimum(np.maximum(val, dt(0.0)), dt(1.0))
    full = full.reshape(H, ss, W, ss, 3)
    acc = np.zeros((H, W, 3), dtype=dt)
    for j in range(ss):                                          # row order; an uncovered sample adds an exact zero
        for i in range(ss):
            acc = acc + full[:, j, :, i]
    mean = np.where(n_cov[..., None] > 0, acc / np.maximum(n_cov, 1)[..., None].astype(dt), dt(0.0))
    rgba = np.zeros((H, W, 4), dtype=np.uint8)
    rgba[..., :3] = np.floor(mean * dt(255.0) + dt(0.5)).astype(np.uint8)
    rgba[..., 3] = np.floor(n_cov.astype(dt) / dt(ss * ss) * dt(255.0) + dt(0.5)).astype(np.uint8)
    return rgba


# ------------------------------------------------------------------ procedural cases
def _unit(rows):
    a = np.asarray(rows, dtype=np.float64)
    return a / np.linalg.norm(a, axis=-1, keepdims=True)


def rig_lights(n=3):
    """the directions of sin3dm_amd.rendering.pbr.three_light_rig (held to it by test_render_pbr_host.py), and a fourth from below"""
    d = _unit([[2.0, 0.0, 10.0], [0.0, 2.0, 6.0], [0.0, -2.0, 10.0], [-3.0, 1.0, -2.0]]) @ np.array([[1.0, 0, 0], [0, 0, -1.0], [0, 1.0, 0]])
    return np.concatenate([d, np.array([[0.5], [0.25], [0.05], [0.3]])], 1)[:n]


def map_images():
    """Four maps of different, non-square sizes (W x H): albedo 5 x 7, metallic 8 x 8, roughness 3 x 4 with a 0, normal 6 x 5 with
    a strong tilt."""
    j, i = np.meshgrid(np.arange(7), np.arange(5), indexing="ij")
    albedo = np.stack([40 + i * 50, 30 + j * 35, 250 - (i + j) * 20], 2).astype(np.uint8)
    j, i = np.meshgrid(np.arange(8), np.arange(8), indexing="ij")
    metallic = ((i * 37 + j * 11) % 256).astype(np.uint8)
    roughness = np.array([[0, 40, 255], [90, 23, 130], [200, 10, 60], [22, 180, 77]], dtype=np.uint8)
    j, i = np.meshgrid(np.arange(5), np.arange(6), indexing="ij")
    t = np.stack([0.75 * np.cos(i * 1.1 + j * 0.4), 0.75 * np.sin(i * 0.7 - j * 0.9), np.full(i.shape, 0.55)], 2)
    normal = np.round((t / np.linalg.norm(t, axis=2, keepdims=True) * 0.5 + 0.5) * 255).astype(np.uint8)
    return albedo, metallic, roughness, normal


def _mapped_material():
    albedo, metallic, roughness, normal = map_images()
    return {"Kd": (0.5, 0.5, 0.5), "image": albedo, "metallic_image": metallic, "roughness_image": roughness, "normal_image": normal}


def _sphere(g, levels, shading, lights, inside_out=False, views=8, mapped=False, angles=None):
    Ws, Hs, ss = g
    v, f = R.icosphere(levels)
    verts = (v * np.array([0.5, 0.4, 0.3]) + np.array([0.2, -0.1, 0.4])).astype(np.float32)
    if inside_out:
        f = np.ascontiguousarray(f[:, ::-1])
    angles = [(45.0 * k, 45.0) for k in range(8)][:views] if angles is None else angles
    case = dict(verts=verts, faces=f, near=R.RIG_NEAR, shading=shading, lights=lights,
                matrices=[R.rig_matrix(verts.astype(np.float64), az, el, Ws // ss, Hs // ss) for az, el in angles])
    if mapped:
        c = v[f.reshape(-1)]
        uv = np.stack([np.arctan2(c[:, 1], c[:, 0]) / (2 * np.pi) + 0.5, c[:, 2] * 0.5 + 0.5], 1)
        case.update(uvs=uv.reshape(-1, 3, 2).astype(np.float32), materials=[_mapped_material()])
    else:
        case["vertex_colors"] = (0.5 + 0.5 * v).astype(np.float32)
    return case


def _quads(g):
    """A quad in perspective with the four maps; beside it a quad of a material with factors only; a third quad of the mapped
    material whose second face has degenerate uvs (det = 0); a face of zero area on vertices of its own; an unreferenced vertex."""
    Ws, Hs, _ = g
    pts = [(8.0, 6.0, 1.0), (36.0, 6.0, 2.0), (36.0, 30.0, 2.0), (8.0, 30.0, 1.0)]
    pts += [(37.5, 8.0, 1.5), (43.5, 8.0, 1.5), (43.5, 28.0, 1.2), (37.5, 28.0, 1.2)]
    pts += [(44.5, 5.0, 1.1), (49.5, 5.0, 1.3), (49.5, 31.0, 1.3), (44.5, 31.0, 1.1)]
    faces = [(0, 1, 2), (0, 2, 3), (4, 5, 6), (4, 6, 7), (8, 9, 10), (8, 10, 11), (12, 13, 14)]
    corner = {0: (0.0, 1.0), 1: (1.0, 1.0), 2: (1.0, 0.0), 3: (0.0, 0.0)}
    uvs = [[corner[v] for v in faces[0]], [corner[v] for v in faces[1]], [(0.3, 0.3)] * 3, [(0.3, 0.3)] * 3,
           [(0.1, 0.9), (0.8, 0.85), (0.9, 0.2)], [(0.2, 0.2), (0.5, 0.5), (0.8, 0.8)], [(0.0, 0.0), (1.0, 0.0), (0.0, 1.0)]]
    verts = np.concatenate([R.screen_verts(pts, Ws, Hs), np.array([[0.0, 0.0, 5.0], [1.0, 0.0, 5.0], [2.0, 0.0, 5.0], [9.0, 9.0, 9.0]], dtype=np.float32)])
    return dict(verts=verts, faces=np.asarray(faces, dtype=np.int32), matrices=[R.SCREEN], near=R.SCREEN_NEAR, shading="pbr",
                uvs=np.asarray(uvs, dtype=np.float32), face_mat=np.asarray([0, 0, 1, 1, 0, 0, 0], dtype=np.int32),
                materials=[_mapped_material(), {"Kd": (0.2, 0.6, 0.9), "Pm": 0.7, "Pr": 0.3}],
                lights=np.concatenate([_unit([[0.2, 0.4, -1.0]]), [[0.9]]], 1), zero_normals=[12, 13, 14, 15])


def _fin(g):
    """Two coincident triangles of opposite winding: the normal sums of their vertices cancel exactly, so the smooth shading falls
    back to the flat normal on every sample; no light, so the ambient term alone."""
    Ws, Hs, _ = g
    pts = [(10.0, 8.0, 1.0), (40.0, 10.0, 1.5), (22.0, 32.0, 1.2)]
    return dict(verts=R.screen_verts(pts, Ws, Hs), faces=np.asarray([(0, 1, 2), (0, 2, 1)], dtype=np.int32), matrices=[R.SCREEN], near=R.SCREEN_NEAR,
                shading="smooth", materials=[{"Kd": (0.9, 0.5, 0.3), "image": None}], lights=np.zeros((0, 4)), ambient=0.6, zero_normals=[0, 1, 2])


CASES = {"a_sphere": lambda g: _sphere(g, 2, "smooth", rig_lights(3)),
         "b_quads": _quads,
         "c_fin": _fin,
         "d_inside_out": lambda g: _sphere(g, 1, "smooth", rig_lights(4), inside_out=True, views=1),
         "e_mapped_sphere": lambda g: _sphere(g, 1, "pbr", rig_lights(3), views=2, mapped=True),
         "f_flat": lambda g: _sphere(g, 1, "flat", rig_lights(1), views=1)}
GRIDS = R.GRIDS


@functools.lru_cache(maxsize=None)
def case(name, grid):
    return CASES[name](GRIDS[grid])


@functools.lru_cache(maxsize=None)
def restated(name, grid, view=0, dt=np.float64):
    """The restatement of one view on its own float64 projection: ({pass: rgba}, flagged [Hs, Ws], raster dict).  Shared, unchanged."""
    c = case(name, grid)
    Ws, Hs, ss = GRIDS[grid]
    smp, r = gathered(name, grid, view)
    images, flagged = shade_pbr(c, c["matrices"][view], smp, Ws, Hs, ss, dt)
    return images, flagged, r


@functools.lru_cache(maxsize=None)
def gathered(name, grid, view=0):
    """(samples, raster dict) of one view on its own float64 projection.  Shared, unchanged."""
    c = case(name, grid)
    Ws, Hs, _ = GRIDS[grid]
    xy, iw = R.project(c["verts"], c["matrices"][view], Ws, Hs, c["near"])
    r = R.raster(xy, iw, c["faces"], Ws, Hs)
    return gather_samples(c, xy, iw, r["face_id"]), r


def all_views():
    return [(n, g, k) for n in CASES for g in GRIDS for k in range(len(case(n, g)["matrices"]))]


def measure():
    """(normal gap, tangent gap, {pass: image gap in levels}, largest flagged share): float32 against float64 over every case."""
    ng = tg = share = 0.0
    ig = {p: 0 for p in PASSES}
    for n in CASES:
        c = case(n, "g64")
        ng = max(ng, relative_gap(vertex_normals(c["verts"], c["faces"], np.float32), vertex_normals(c["verts"], c["faces"])))
        if c.get("uvs") is not None:
            tg = max(tg, relative_gap(face_tangents(c["verts"], c["faces"], c["uvs"], np.float32), face_tangents(c["verts"], c["faces"], c["uvs"])))
    for n, g, k in all_views():
        a, flagged, r = restated(n, g, k)
        b, _, _ = restated(n, g, k, np.float32)
        ss = GRIDS[g][2]
        keep = ~flagged.reshape(flagged.shape[0] // ss, ss, flagged.shape[1] // ss, ss).any((1, 3))
        share = max(share, flagged.sum() / max(1, (r["face_id"] >= 0).sum()))
        for p in PASSES:
            ig[p] = max(ig[p], int(np.abs(a[p].astype(np.int64) - b[p])[keep].max(initial=0)))
    return ng, tg, ig, share


# ------------------------------------------------------------------ the gain ladder: the light model's float value read out of uint8
# With ambient = 0 the model is linear in the light intensities, and scaling them by 2^k is exact in float32: before the clamp the
# value at gain 2^k is 2^k times the value at gain 1.  A pixel-channel is read at the largest gain at which the float64 restatement
# does not clip, where its level is in [128, 255) whatever its magnitude (down to 2^-24 of full scale): its leading 7 to 8 bits, so
# the comparison is relative, 0.2 to 0.8 %, where the images at gain 1 are absolute, 0.4 % of full scale.
LADDER_GAINS = tuple(2.0 ** k for k in range(25))
LADDER_PASSES = ("shaded", "geo")
LADDER_FLOOR = 64                                            # a readout below this level is not compared (the value is under 2^-23, or clipped early)
LADDER_VIEWS = ((0.0, 45.0), (135.0, 45.0), (225.0, 45.0))
LADDER_MATERIALS = {"m0_black_dielectric": {"Kd": (0.0, 0.0, 0.0), "Pm": 0.0, "Pr": 0.5},
                    "m1_near_mirror": {"Kd": (0.0, 0.0, 0.0), "Pm": 0.0, "Pr": 0.05},
                    "m2_polished_metal": {"Kd": (0.9, 0.6, 0.2), "Pm": 1.0, "Pr": 0.0},
                    "m3_metal": {"Kd": (0.9, 0.6, 0.2), "Pm": 1.0, "Pr": 0.3},
                    "m4_half_metal": {"Kd": (0.3, 0.5, 0.7), "Pm": 0.5, "Pr": 0.25},
                    "m5_rough_white": {"Kd": (1.0, 1.0, 1.0), "Pm": 0.0, "Pr": 1.0}}
# measured by measure_ladder() (profiles/render_pbr.txt): float32 against float64 at the readout, in levels
LADDER_GAP = {"shaded": 1, "geo": 0}
LADDER_BOUND = {p: max(1, 2 * int(math.ceil(g))) for p, g in LADDER_GAP.items()}


def _ladder(grid, material=None, angles=LADDER_VIEWS, lights=None):
    """The ellipsoid of _sphere at 320 faces, smooth normals, four rig lights, no ambient; material None: the four maps."""
    c = _sphere(GRIDS[grid], 2, "pbr", rig_lights(4) if lights is None else lights, angles=list(angles), mapped=material is None)
    if material is not None:
        del c["vertex_colors"]
        c["materials"] = [dict(material)]
    c.update(ambient=0.0, grid=grid)
    return c


LADDER_CASES = {name: (lambda m=m: _ladder("g50", m)) for name, m in LADDER_MATERIALS.items()}
# the tilted normals of the map turn up to a quarter of what some views see away from every light (exact zeros, which no gain
# reads): the mapped case takes three views on which the restatement meets the caps of test_render_pbr_host.py with room to spare
LADDER_CASES.update({"n_mapped": lambda: _ladder("g50", angles=((135.0, 30.0), (180.0, 45.0), (180.0, 30.0))),
                     "s_supersampled": lambda: _ladder("g64", LADDER_MATERIALS["m4_half_metal"]),
                     # one light, seen from near its own direction so that it reaches most of what the camera sees
                     "o_one_light": lambda: _ladder("g50", LADDER_MATERIALS["m4_half_metal"], angles=((90.0, 20.0),), lights=rig_lights(4)[1:2])})


@functools.lru_cache(maxsize=None)
def ladder_case(name):
    return LADDER_CASES[name]()


def ladder_views():
    return [(n, k) for n in LADDER_CASES for k in range(len(ladder_case(n)["matrices"]))]


_LADDER_SAMPLES = {}


def ladder_samples(c, view, xy=None, iw=None):
    """(samples, raster dict) of one view of a ladder case on the given projection (None: its own float64 one); kept by content,
    since the ladder cases share one mesh and their views."""
    Ws, Hs, _ = GRIDS[c["grid"]]
    if xy is None:
        xy, iw = R.project(c["verts"], c["matrices"][view], Ws, Hs, c["near"])
    key = (Ws, Hs, np.asarray(xy).tobytes(), np.asarray(iw).tobytes(), np.asarray(c["faces"]).tobytes())
    if key not in _LADDER_SAMPLES:
        r = R.raster(xy, iw, c["faces"], Ws, Hs)
        _LADDER_SAMPLES[key] = (gather_samples(c, xy, iw, r["face_id"]), r)
    return _LADDER_SAMPLES[key]


def ladder_levels(val, smp, Ws, Hs, ss, dt):
    """(levels uint8 [G, H, W, 3], unclipped bool [G, H, W, 3]) of per-sample values [S, 3] at gain 1: the value times each gain
    (exact) through resolve(); unclipped: no sample of the pixel exceeds 1 in that channel at that gain."""
    assert val.dtype == dt
    H, W = Hs // ss, Ws // ss
    full = np.zeros((Hs * Ws, 3), dtype=dt)
    full[smp["s"]] = val
    top = full.reshape(H, ss, W, ss, 3).max((1, 3))
    levels = np.stack([resolve(val * dt(g), smp, Ws, Hs, ss, dt)[..., :3] for g in LADDER_GAINS])
    unclipped = np.stack([top * dt(g) <= dt(1.0) for g in LADDER_GAINS])
    return levels, unclipped


def ladder_readout(levels_by_gain, reference_by_gain, unclipped=None):
    """(got, want, read, gain index), each [...]: every pixel-channel at the largest gain at which the reference [G, ...] is below
    255 (and, with unclipped [G, ...], none of the pixel's samples clips); read where there is such a gain and the reference's
    level at it is at least LADDER_FLOOR.  levels_by_gain [G, ...] is read at the reference's choice of gain."""
    ref, lev = np.asarray(reference_by_gain).astype(np.int64), np.asarray(levels_by_gain).astype(np.int64)
    assert ref.shape == lev.shape and ref.shape[0] == len(LADDER_GAINS)
    ok = ref < 255
    if unclipped is not None:
        ok = ok & np.asarray(unclipped)
    k = len(ref) - 1 - np.argmax(ok[::-1], 0)                    # the largest gain index with ok (meaningless where none is)
    want, got = np.take_along_axis(ref, k[None], 0)[0], np.take_along_axis(lev, k[None], 0)[0]
    return got, want, ok.any(0) & (want >= LADDER_FLOOR), k


def ladder_reference(name, view, dt=np.float64, fault=None, xy=None, iw=None):
    """One view of a ladder case in the number type dt: dict of levels / unclipped {pass: [G, H, W, 3]}, left_out bool [H, W] (a
    sample of the pixel is flagged by EPS_FLIP, EPS_NV or EPS_NL), covered bool [H, W], n_flagged / n_covered (samples), raster."""
    c = ladder_case(name)
    Ws, Hs, ss = GRIDS[c["grid"]]
    smp, r = ladder_samples(c, view, xy, iw)
    raw = shade_pbr(c, c["matrices"][view], smp, Ws, Hs, ss, dt, fault=fault, raw=True)
    out = {"levels": {}, "unclipped": {}, "raster": r}
    for p in LADDER_PASSES:
        out["levels"][p], out["unclipped"][p] = ladder_levels(raw[p], smp, Ws, Hs, ss, dt)
    per_pixel = lambda a: a.reshape(Hs // ss, ss, Ws // ss, ss).any((1, 3))          # noqa: E731
    flag = np.zeros(Hs * Ws, dtype=bool)
    flag[smp["s"][raw["flagged"] | raw["grazing"]]] = True
    out.update(left_out=per_pixel(flag), covered=per_pixel(r["face_id"] >= 0), n_flagged=int(flag.sum()), n_covered=int((r["face_id"] >= 0).sum()))
    return out


@functools.lru_cache(maxsize=None)
def ladder_restated(name, view, dt=np.float64, fault=None):
    """ladder_reference on the view's own float64 projection.  Shared, unchanged."""
    return ladder_reference(name, view, dt, fault)


def ladder_compare(got_levels, ref, agree=None):
    """{pass: (largest |got - reference| in levels over the read pixel-channels that are not left out, read share of the covered
    pixel-channels, gain indices read)} of levels {pass: [G, H, W, 3]} against a ladder_reference(); agree bool [H, W]: the
    pixels to compare at all (those whose samples agree in face_id)."""
    res = {}
    for p in LADDER_PASSES:
        got, want, read, k = ladder_readout(got_levels[p], ref["levels"][p], ref["unclipped"][p])
        keep = read & ~ref["left_out"][..., None] & (True if agree is None else agree[..., None])
        res[p] = (int(np.abs(got - want)[keep].max(initial=0)), float(read[ref["covered"]].mean()), np.unique(k[keep]))
    return res


def measure_ladder(fault=None, dt=np.float32):
    """({pass: largest difference in levels}, {(case, view): {pass: difference}}): the float64 restatement against the evaluation
    in dt with a fault, at the readout, over every ladder case.  fault None and float32: LADDER_GAP."""
    worst, each = {p: 0 for p in LADDER_PASSES}, {}
    for n, k in ladder_views():
        ref, other = ladder_restated(n, k), ladder_restated(n, k, dt, fault)
        res = ladder_compare(other["levels"], ref)
        each[(n, k)] = {p: res[p][0] for p in LADDER_PASSES}
        for p in LADDER_PASSES:
            worst[p] = max(worst[p], res[p][0])
    return worst, each
