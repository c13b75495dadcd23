"""The yardstick of the ray query and the shadow mask (s3d_ray.hip): a brute-force float64 restatement over all
triangles without a grid, a NumPy float32 replay of the kernel's written order of operations, a Python copy of the grid walk
that takes injected faults, and the procedural cases.  Projection, the integer raster stage and the samples' edge values are
those of tests/render_cases.py and tests/render_pbr_cases.py.

The pair terms.  For a ray (o, d) and a triangle (a, b, c), in the order of include/sin3dm_hip.h: e1 = b - a, e2 = c - a,
p = d x e2, s = o - a, q = s x e1, det = e1 . p, u = s . p, v = d . q, w = e2 . q, all four negated when det < 0;
hit = det > 0 and u >= 0 and v >= 0 and u + v <= det and t_min <= w / det <= t_max.  With m = max(|e1|, |e2|, |s|), the four
values det, u, v, det - u - v are bounded by S = |d| m^2 and w, t_min det, t_max det by Sw = m^2 max(m, t_min |d|, t_max |d|):
divided by these they are pure numbers, and the float32 evaluation moves each of them by an absolute amount that the gap below
measures.

Near a tie.  A pair's outcome is clear when float32 cannot change it: a clear miss when one of u, v, det - u - v lies below
-BAND S, or when det > BAND S and the crossing lies outside [t_min, t_max] by more than BAND Sw; a clear hit when all of det, u,
v, det - u - v exceed BAND S and the crossing lies inside by more than BAND Sw.  Every other pair is a tie — it has a crossing
parameter within the band of t_min or t_max, or a smallest barycentric within the band of 0, or a determinant within the band of
0, while nothing else decides it — and a ray with a tied pair (other than its skipped face) is left out of the comparison.
(The three criteria of the issue, restricted to pairs they can decide: a zero-area triangle has det = 0 for EVERY ray, and is a
clear miss for all of them but those through its line.)  For the mask a fourth tie joins them: |N . L| <= BAND |N| |L|, the
facing test — unless float32 has nothing to round there: the edge differences and the six products of the face's cross product
are exact in float32 (the normal is then the same number fused or not) and every product N_k L_k is zero (an axis-aligned face
under a light with a zero component), which is bit 0 in float32 as well.

The band is measured, not chosen (measure(), as render_cases.measure_depth_gap): RAY_GAP is the largest difference of the pure
numbers between the float32 replay — the sample point b0 P0 + b1 P1 + b2 P2 from float32 barycentrics included, for that is where
the mask's rays start — and float64, over all rays and triangles of all cases; RAY_BAND is ten times that.  The share of a case's
rays left out is capped at render_cases.MAX_LEFT_OUT; test_render_shadow_host.py holds the restatement alone to the cap.

Exact rays.  GENERIC's coordinates are small multiples of 1 / 4: every product of the test is exact in float32, float32 and
float64 agree bit for bit, and these rays are compared in full, ties included — that is what sees an exclusive edge rule and a
hit clipped to its cell, which no comparison that leaves the ties out can see."""
import functools
import math

import numpy as np

import render_cases as R
import render_pbr_cases as P

GRID = (64, 48)                                              # the sample grid of every view; the images: supersample 1 and 2
SUPERSAMPLES = (1, 2)
RAY_GAP = 8.2e-07                                            # measured by measure() (profiles/render_shadow.txt): 8.18e-07
RAY_BAND = 10 * RAY_GAP
T_MIN_REL = 1e-4                                             # rasterizer.SHADOW_T_MIN_REL
WALK_GRIDS = ((1, 1, 1), (2, 3, 5), (17, 17, 17), None)      # None: the default resolution
FAULTS = ("skip_last_cell", "exclusive_edges", "ignore_skip_face", "t_min_zero", "clip_to_cell")


# ------------------------------------------------------------------ the pair terms, written once for a number type
def pair_terms(o, d, tri9, dt):
    """(det, u, v, w) [n, F] before the sign flip, in the kernel's order of operations, evaluated in dt."""
    o, d, t = np.asarray(o).astype(dt)[:, None, :], np.asarray(d).astype(dt)[:, None, :], np.asarray(tri9, dtype=np.float32).astype(dt)[None]
    a, b, c = t[..., 0:3], t[..., 3:6], t[..., 6:9]
    e1, e2 = b - a, c - a

    def cross(x, y):
        return (x[..., 1] * y[..., 2] - x[..., 2] * y[..., 1], x[..., 2] * y[..., 0] - x[..., 0] * y[..., 2], x[..., 0] * y[..., 1] - x[..., 1] * y[..., 0])

    def dot(x, y):
        return (x[0] * y[0] + x[1] * y[1]) + x[2] * y[2]
    p = cross(d, e2)
    s = o - a
    q = cross(s, e1)
    c3 = lambda x: (x[..., 0], x[..., 1], x[..., 2])         # noqa: E731
    det, u, v, w = dot(c3(e1), p), dot(c3(s), p), dot(c3(d), q), dot(c3(e2), q)
    assert det.dtype == dt
    return det, u, v, w


def _flip(det, u, v, w):
    sg = np.where(det < 0, -1.0, 1.0).astype(det.dtype)
    return det * sg, u * sg, v * sg, w * sg


def hits_of(det, u, v, w, t_min, t_max, exclusive=False):
    """bool [n, F]: the kernel's decision on terms of any number type."""
    det, u, v, w = _flip(det, u, v, w)
    with np.errstate(all="ignore"):
        t = w / det
        if exclusive:
            inside = (det > 0) & (u > 0) & (v > 0) & (u + v < det)
        else:
            inside = (det > 0) & (u >= 0) & (v >= 0) & (u + v <= det)
        return inside & (t >= t_min) & (t <= t_max)


def _scales(o, d, tri9, t_min, t_max):
    o, d, t = np.asarray(o, dtype=np.float64)[:, None, :], np.asarray(d, dtype=np.float64)[:, None, :], np.asarray(tri9, dtype=np.float32).astype(np.float64)[None]
    n = lambda x: np.sqrt((x * x).sum(-1))                   # noqa: E731
    m = np.maximum(np.maximum(n(t[..., 3:6] - t[..., 0:3]), n(t[..., 6:9] - t[..., 0:3])), n(o - t[..., 0:3]))
    m = np.where(m > 0, m, 1.0)
    ld = n(d)
    reach = np.maximum(m, t_min * ld)
    if math.isfinite(t_max):
        reach = np.maximum(reach, t_max * ld)
    return ld * m * m, m * m * reach


def restate(o, d, skip, tri9, t_min, t_max, band=RAY_BAND):
    """(hit bool [n], tie bool [n], status int [n]) of the brute force in float64: every triangle but the skipped one, no grid."""
    o, d = np.asarray(o, dtype=np.float64).reshape(-1, 3), np.asarray(d, dtype=np.float64).reshape(-1, 3)
    n, F = len(o), len(tri9)
    with np.errstate(all="ignore"):
        bad = ~(np.isfinite(o).all(1) & np.isfinite(d).all(1)) | ~(d != 0).any(1)
    status = np.where(bad, 2, 0)
    if F == 0 or n == 0:
        return np.zeros(n, dtype=bool), np.zeros(n, dtype=bool), status
    oo, dd = np.where(bad[:, None], 0.0, o), np.where(bad[:, None], 1.0, d)
    det, u, v, w = _flip(*pair_terms(oo, dd, tri9, np.float64))
    S, Sw = _scales(oo, dd, tri9, t_min, t_max)
    hit = hits_of(det, u, v, w, t_min, t_max)
    r = det - u - v
    lo = w - t_min * det
    hi = (t_max * det - w) if math.isfinite(t_max) else np.full_like(w, np.inf)
    out_bary = (u < -band * S) | (v < -band * S) | (r < -band * S)
    clear_miss = out_bary | ((det > band * S) & ((lo < -band * Sw) | (hi < -band * Sw)))
    clear_hit = (det > band * S) & (u > band * S) & (v > band * S) & (r > band * S) & (lo > band * Sw) & (hi > band * Sw)
    tie = ~(clear_miss | clear_hit)
    assert not (hit & clear_miss).any() and not (~hit & clear_hit).any()
    if skip is not None:
        sk = np.asarray(skip).reshape(-1)
        own = np.arange(F)[None, :] == sk[:, None]
        hit, tie = hit & ~own, tie & ~own
    return hit.any(1) & ~bad, tie.any(1) & ~bad, status


def pair_gap(o64, o32, d, skip, tri9, t_min, t_max):
    """The largest difference of the pure numbers between the float32 replay (from the float32 origin o32) and float64 (from o64)."""
    if len(tri9) == 0 or len(o64) == 0:
        return 0.0
    a = _flip(*pair_terms(o64, d, tri9, np.float64))
    b32 = pair_terms(np.asarray(o32, dtype=np.float32), np.asarray(d, dtype=np.float32), tri9, np.float32)
    sg = np.where(pair_terms(o64, d, tri9, np.float64)[0] < 0, -1.0, 1.0)       # the float64 sign for both: a flip of a tiny det is no gap
    b = [x.astype(np.float64) * sg for x in b32]
    r32 = (b32[0] - (b32[1] + b32[2])).astype(np.float64) * sg                  # (u + v <= det, as the kernel adds them)
    S, Sw = _scales(o64, d, tri9, t_min, t_max)
    g = np.maximum.reduce([np.abs(a[0] - b[0]) / S, np.abs(a[1] - b[1]) / S, np.abs(a[2] - b[2]) / S, np.abs((a[0] - a[1] - a[2]) - r32) / S,
                           np.abs(a[3] - b[3]) / Sw])
    if skip is not None:
        g = np.where(np.arange(len(tri9))[None, :] == np.asarray(skip).reshape(-1)[:, None], 0.0, g)
    return float(g.max())


# ------------------------------------------------------------------ the mask's rays, from the raster buffers of a view
def tri9_of(case):
    return np.asarray(case["verts"], dtype=np.float32)[np.asarray(case["faces"]).reshape(-1)].reshape(-1, 9)


def t_min_of(case):
    if case.get("t_min") is not None:
        return float(case["t_min"])
    c = tri9_of(case).reshape(-1, 3).astype(np.float64)
    return T_MIN_REL * float(np.linalg.norm(c.max(0) - c.min(0))) if len(c) else 0.0


def mask_rays(case, xy, iw, face_id, dt=np.float64):
    """Per covered sample (row order): dict of s (flat index), f, P [S, 3] (the point, in dt: float32 multiplies float32
    barycentrics as the kernel does), N [S, 3] (float64: the face's own normal turned to the camera by the integer rule)."""
    smp = P.gather_samples(case, xy, iw, face_id)
    verts = np.asarray(case["verts"], dtype=np.float32)
    if len(smp["s"]) == 0:
        return dict(smp, P=np.zeros((0, 3), dtype=dt), N=np.zeros((0, 3)), exact_normal=np.zeros(0, dtype=bool))
    if dt == np.float32:
        num = smp["E"].astype(np.float32) * smp["w"].astype(np.float32)
    else:
        num = smp["E"].astype(np.float64) * smp["w"]
    b = num / (num[:, 0] + num[:, 1] + num[:, 2])[:, None]
    c = verts[smp["vid"]].astype(dt)                                              # [S, 3 corners, 3]
    pt = b[:, 0, None] * c[:, 0] + b[:, 1, None] * c[:, 1] + b[:, 2, None] * c[:, 2]
    assert pt.dtype == dt
    m = np.asarray(case["matrix"], dtype=np.float64)
    front_sign = -1 if np.linalg.det(m[[0, 1, 3]][:, :3]) < 0 else 1
    fv = verts[np.asarray(case["faces"])[smp["f"]]].astype(np.float64)            # the face's own order
    nrm = np.cross(fv[:, 1] - fv[:, 0], fv[:, 2] - fv[:, 0])
    front = np.where(smp["swapped"], -1, 1) * front_sign > 0
    u, w = fv[:, 1] - fv[:, 0], fv[:, 2] - fv[:, 0]                               # (differences of float32 values: taken as exact here, checked below)
    prods = np.stack([u[:, 1] * w[:, 2], u[:, 2] * w[:, 1], u[:, 2] * w[:, 0], u[:, 0] * w[:, 2], u[:, 0] * w[:, 1], u[:, 1] * w[:, 0]], 1)
    exact = ((prods.astype(np.float32).astype(np.float64) == prods).all(1) & (u.astype(np.float32) == u).all(1) & (w.astype(np.float32) == w).all(1))
    return dict(smp, P=pt, N=np.where(front[:, None], nrm, -nrm), exact_normal=exact)


def restate_mask(case, xy, iw, face_id, band=RAY_BAND):
    """(lit uint8 [Hs, Ws], left_out bool [Hs, Ws]): the float64 mask of a view on given raster buffers, and the samples with a
    tie for some light."""
    Hs, Ws = face_id.shape
    lit, left = np.zeros(Hs * Ws, dtype=np.uint8), np.zeros(Hs * Ws, dtype=bool)
    rays = mask_rays(case, xy, iw, face_id)
    tri9, t_min = tri9_of(case), t_min_of(case)
    for k, light in enumerate(np.asarray(case["lights"], dtype=np.float64).reshape(-1, 4)):
        L = np.asarray(np.asarray(light[:3], dtype=np.float32), dtype=np.float64)
        nl = rays["N"] @ L
        nn = np.sqrt((rays["N"] ** 2).sum(1)) * np.linalg.norm(L)
        facing = nl > 0
        left[rays["s"]] |= (np.abs(nl) <= band * nn) & ~(rays["exact_normal"] & (rays["N"] * L == 0).all(1))
        idx = np.nonzero(facing)[0]
        hit, tie, _ = restate(rays["P"][idx], np.broadcast_to(L, (len(idx), 3)), rays["f"][idx], tri9, t_min, math.inf, band)
        lit[rays["s"][idx[~hit]]] |= np.uint8(1 << k)
        left[rays["s"][idx[tie]]] = True
    return lit.reshape(Hs, Ws), left.reshape(Hs, Ws)


# ------------------------------------------------------------------ a Python copy of the grid walk, with injected faults
def walk_grid(tri9, dims, slack=None):
    """(origin [3], cell, dims, lists {cell index: [faces]}): rasterizer.ray_grid_box's box and the conservative lists in float64."""
    from sin3dm_amd.rendering import rasterizer
    c = np.asarray(tri9, dtype=np.float64).reshape(-1, 3)
    lo, hi = (c.min(0), c.max(0)) if len(c) else (np.zeros(3), np.ones(3))
    origin, cell, dims, sl = rasterizer.ray_grid_box(lo, hi, len(tri9), dims)
    slack = sl if slack is None else slack
    origin = origin.astype(np.float64)
    lists = {}
    for f, t in enumerate(np.asarray(tri9, dtype=np.float64).reshape(-1, 3, 3)):
        a = [np.clip(np.floor((t[:, k].min() - slack - origin[k]) / cell), 0, dims[k] - 1).astype(int) for k in range(3)]
        b = [np.clip(np.floor((t[:, k].max() + slack - origin[k]) / cell), 0, dims[k] - 1).astype(int) for k in range(3)]
        for ix in range(a[0], b[0] + 1):
            for iy in range(a[1], b[1] + 1):
                for iz in range(a[2], b[2] + 1):
                    lists.setdefault((ix * dims[1] + iy) * dims[2] + iz, []).append(f)
    return origin, cell, dims, lists


def walk(o, d, skip, t_min, t_max, tri9, grid, fault=None):
    """(hit, status) of one ray: the traversal of s3d_ray.hip statement by statement, in float64, with one fault of FAULTS."""
    origin, cell, dims, lists = grid
    o, d = np.asarray(o, dtype=np.float64), np.asarray(d, dtype=np.float64)
    if not (np.isfinite(o).all() and np.isfinite(d).all()) or not (d != 0).any():
        return 0, 2
    if fault == "t_min_zero":
        t_min = 0.0
    if fault == "ignore_skip_face":
        skip = -1
    t0, t1 = t_min, t_max
    for k in range(3):
        lo, hi = origin[k], origin[k] + dims[k] * cell
        if d[k] == 0:
            if not lo <= o[k] <= hi:
                return 0, 1
        else:
            a, b = (lo - o[k]) / d[k], (hi - o[k]) / d[k]
            t0, t1 = max(t0, min(a, b)), min(t1, max(a, b))
    if not t0 <= t1:
        return 0, 1
    i = [int(min(dims[k] - 1, max(0, math.floor((o[k] + t0 * d[k] - origin[k]) / cell)))) for k in range(3)]
    st = [1 if d[k] > 0 else (-1 if d[k] < 0 else 0) for k in range(3)]
    border = lambda k: ((origin[k] + (i[k] + (1 if st[k] > 0 else 0)) * cell) - o[k]) / d[k] if st[k] else math.inf      # noqa: E731
    tn = [border(k) for k in range(3)]
    t_enter = t0
    for _ in range(dims[0] + dims[1] + dims[2] + 1):
        k = 0 if (tn[0] <= tn[1] and tn[0] <= tn[2]) else (1 if tn[1] <= tn[2] else 2)
        last = not tn[k] <= t1 or not 0 <= i[k] + st[k] < dims[k]
        if not (fault == "skip_last_cell" and last):
            fs = [f for f in lists.get((i[0] * dims[1] + i[1]) * dims[2] + i[2], []) if f != skip]
            if fs:
                det, u, v, w = pair_terms(o[None], d[None], tri9[fs], np.float64)
                h = hits_of(det, u, v, w, t_min, t_max, exclusive=fault == "exclusive_edges")[0]
                if fault == "clip_to_cell":
                    with np.errstate(all="ignore"):
                        t = (w / det)[0]
                    h = h & (t >= t_enter) & (t < min(tn[k], t1))
                if h.any():
                    return 1, 0
        if last:
            break
        t_enter = tn[k]
        i[k] += st[k]
        tn[k] = border(k)
    return 0, 0


# ------------------------------------------------------------------ procedural cases
def _box(lo, hi):
    x0, y0, z0 = lo
    x1, y1, z1 = hi
    v = [(x0, y0, z0), (x1, y0, z0), (x1, y1, z0), (x0, y1, z0), (x0, y0, z1), (x1, y0, z1), (x1, y1, z1), (x0, y1, z1)]
    f = [(0, 2, 1), (0, 3, 2), (4, 5, 6), (4, 6, 7), (0, 1, 5), (0, 5, 4), (2, 3, 7), (2, 7, 6), (1, 2, 6), (1, 6, 5), (3, 0, 4), (3, 4, 7)]
    return v, f


def _join(parts):
    verts, faces = [], []
    for v, f in parts:
        faces += [tuple(i + len(verts) for i in t) for t in f]
        verts += list(v)
    return np.asarray(verts, dtype=np.float32), np.asarray(faces, dtype=np.int32).reshape(-1, 3)


def _lights(dirs, intensities=(0.5, 0.25, 0.3, 0.2)):
    d = P._unit(np.asarray(dirs, dtype=np.float64).reshape(-1, 3))
    return np.concatenate([d, np.asarray(intensities[:len(d)], dtype=np.float64)[:, None]], 1)


def _case(verts, faces, lights, az=45.0, el=45.0, **extra):
    verts = np.asarray(verts, dtype=np.float32)
    ref = verts.astype(np.float64) if len(verts) else np.array([[0.0, 0, 0], [1.0, 1, 1]])
    return dict(verts=verts, faces=np.asarray(faces, dtype=np.int32).reshape(-1, 3), lights=np.asarray(lights, dtype=np.float64).reshape(-1, 4),
                matrix=R.rig_matrix(ref, az, el, *GRID), near=R.RIG_NEAR, **extra)


SLAB = ((-0.4, 0.5, -0.3), (0.4, 0.625, 0.3))                 # the floating slab; the floor is y = 0, the light straight down (up is +y)


def _slab():
    floor = ([(-1.0, 0.0, -1.0), (1.0, 0.0, -1.0), (1.0, 0.0, 1.0), (-1.0, 0.0, 1.0)], [(0, 2, 1), (0, 3, 2)])
    v, f = _join([floor, _box(*SLAB)])
    return _case(v, f, _lights([(0.0, 1.0, 0.0)]), az=35.0, el=50.0)


def _convex():
    v, f = R.icosphere(2)
    return _case(v * np.array([0.5, 0.4, 0.3]) + np.array([0.2, -0.1, 0.4]), f, P.rig_lights(3), vertex_colors=(0.5 + 0.5 * v).astype(np.float32))


def torus(nu=16, nv=8, R0=0.6, r=0.25):
    u, v = np.meshgrid(np.arange(nu) / nu * 2 * np.pi, np.arange(nv) / nv * 2 * np.pi, indexing="ij")
    p = np.stack([(R0 + r * np.cos(v)) * np.cos(u), r * np.sin(v), (R0 + r * np.cos(v)) * np.sin(u)], 2).reshape(-1, 3)
    i, j = np.meshgrid(np.arange(nu), np.arange(nv), indexing="ij")
    q = lambda a, b: ((a % nu) * nv + (b % nv)).reshape(-1)  # noqa: E731
    f = np.concatenate([np.stack([q(i, j), q(i + 1, j), q(i + 1, j + 1)], 1), np.stack([q(i, j), q(i + 1, j + 1), q(i, j + 1)], 1)])
    return p, f


def _concave():
    v, f = torus()
    tilt = np.array([[1.0, 0, 0], [0, math.cos(0.5), -math.sin(0.5)], [0, math.sin(0.5), math.cos(0.5)]])
    return _case(v @ tilt.T, f, _lights([(1.0, 1.2, 0.4), (-0.8, 0.9, 0.1), (0.1, 0.7, -1.0)]), vertex_colors=np.full((len(v), 3), 0.8, dtype=np.float32))


def _overhang(lights):
    """Two stacked boxes on integer coordinates (cell borders of the 2 x 3 x 5 grid and others fall on them), the upper one
    overhanging along +x and +z; a duplicated face, a zero-area triangle and a sliver through the whole box."""
    lower, upper = _box((0, 0, 0), (2, 2, 2)), _box((1, 2, 1), (3, 3, 3))
    extra = ([(2.0, 0.0, 0.0), (2.0, 2.0, 0.0), (2.0, 2.0, 2.0),                   # a copy of a triangle of the lower box's +x face
              (3.0, 1.0, 0.0), (3.5, 1.0, 0.5), (3.5, 1.0, 0.5),                   # zero area: two corners coincide
              (-0.5, -0.5, -0.5), (3.5, 3.5, 3.5), (3.5, 3.5, 3.4)],               # a sliver from corner to corner of the box
             [(0, 1, 2), (3, 4, 5), (6, 7, 8)])
    v, f = _join([lower, upper, extra])
    return _case(v, f, lights, az=-35.0, el=68.0)


def _thin():
    """A bumpy sheet 2 x 2 wide and 0.02 high: the default grid and every coarse one has one cell across it."""
    n = 9
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    y = 0.01 * np.sin(2.3 * i) * np.cos(1.7 * j)
    p = np.stack([i / (n - 1) * 2 - 1, y, j / (n - 1) * 2 - 1], 2).reshape(-1, 3)
    q = lambda a, b: (a * n + b).reshape(-1)                 # noqa: E731
    a, b = i[:-1, :-1], j[:-1, :-1]
    f = np.concatenate([np.stack([q(a, b), q(a + 1, b), q(a + 1, b + 1)], 1), np.stack([q(a, b), q(a + 1, b + 1), q(a, b + 1)], 1)])
    return _case(p, f, _lights([(1.0, 0.02, 0.3), (-0.4, 0.05, 1.0)]), az=60.0, el=40.0)


def _nothing(empty):
    v, f = _box((0, 0, 0), (1, 1, 1))
    c = _case(np.asarray(v, dtype=np.float32), np.zeros((0, 3), dtype=np.int32) if empty else f, P.rig_lights(3))
    if not empty:                                              # a camera that looks away from the box: no covered sample
        m = np.array(c["matrix"])
        m[3] = -m[3]
        m[2] = m[3]
        c["matrix"] = m
    return c


CASES = {"a_slab": _slab, "b_convex": _convex, "c_concave": _concave,
         "d_overhang_axes": lambda: _overhang(_lights([(1.0, 0, 0), (0, 1.0, 0), (0, 0, 1.0)])),
         "d_overhang_zero": lambda: _overhang(_lights([(1.0, 0.5, 0), (0, 1.0, 0.5), (0.7, 0, 1.0)])),
         "e_thin": _thin, "f_empty": lambda: _nothing(True), "f_off": lambda: _nothing(False)}
IMAGE_CASES = ("b_convex", "c_concave", "d_overhang_zero")   # three lights each: the eight subsets


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


@functools.lru_cache(maxsize=None)
def restated(name):
    """The restatement on its own float64 projection and raster stage: (xy, iw, face_id, lit, left_out).  Shared, left unchanged."""
    c = case(name)
    Ws, Hs = GRID
    xy, iw = R.project(c["verts"], c["matrix"], Ws, Hs, c["near"])
    face_id = R.raster(xy, iw, c["faces"], Ws, Hs)["face_id"]
    lit, left = restate_mask(c, xy, iw, face_id)
    return xy, iw, face_id, lit, left


# ------------------------------------------------------------------ generic rays on exact coordinates
def generic():
    """dict: verts, faces, and rays = [(origin, direction, skip_face, t_min, t_max, hit, status, why)]: a triangle in z = 0 (face 0),
    a quad in z = 1 above part of it (faces 1, 2).  Coordinates are multiples of 1 / 4 below 8: exact in float32."""
    verts = np.array([(0, 0, 0), (4, 0, 0), (0, 4, 0), (0, 0, 1), (2, 0, 1), (2, 2, 1), (0, 2, 1)], dtype=np.float32)
    faces = np.array([(0, 1, 2), (3, 4, 5), (3, 5, 6)], dtype=np.int32)
    inf, nan = math.inf, math.nan
    rays = [((1, 0.5, -1), (0, 0, 1), -1, 0, inf, 1, 0, "from below, inside the grid's column"),
            ((1, 0.5, -8), (0, 0, 2), -1, 0, inf, 1, 0, "from outside the grid, pointing in"),
            ((1, 0.5, -8), (0, 0, -1), -1, 0, inf, 0, 1, "from outside, pointing away"),
            ((9, 9, 9), (1, 0, 0), -1, 0, inf, 0, 1, "outside, parallel to an axis: never enters"),
            ((3, 0.5, 0.5), (0, 0, 1), -1, 0, inf, 0, 0, "inside the grid, beside the quad"),
            ((1, 0.5, 0.5), (0, 0, 1), -1, 0, inf, 1, 0, "inside the grid, under the quad"),
            ((1, 0.5, 0.5), (0, 0, 1), -1, 0, 0.25, 0, 0, "t_max just short of the quad"),
            ((1, 0.5, 0.5), (0, 0, 1), -1, 0, 0.75, 1, 0, "t_max just beyond the quad"),
            ((1, 0.5, 0.5), (0, 0, 1), -1, 0, 0.5, 1, 0, "t_max exactly at the quad: the bound is inclusive"),
            ((1, 0.5, 0.5), (0, 0, 1), -1, 0.5, inf, 1, 0, "t_min exactly at the quad: inclusive"),
            ((1, 0.5, 0.5), (0, 0, 1), -1, 0.75, inf, 0, 0, "t_min beyond the quad"),
            ((1, 0.5, 0.5), (0, 0, 1), 1, 0, inf, 0, 0, "skip_face is the only occluder"),
            ((1, 0.5, 0.5), (0, 0, 1), 2, 0, inf, 1, 0, "skip_face is another face"),
            ((3, 0.5, 0.5), (0, 0, -1), 0, 0, inf, 0, 0, "down to the triangle, which is skipped"),
            ((3, 0.5, 0.5), (0, 0, -1), -1, 0, inf, 1, 0, "down to the triangle"),
            ((2, 0, 2), (0, 0, -1), 1, 0, inf, 1, 0, "through the edge y = 0 of the triangle: edges are inclusive"),
            ((4, 0, 2), (0, 0, -1), -1, 0, inf, 1, 0, "through a corner of the triangle"),
            ((2, 2, 2), (0, 0, -1), 1, 0, 1.5, 1, 0, "through a corner of the quad's second face"),
            ((1, 1, 2), (0, 0, -1), 2, 0, 1.5, 1, 0, "through the quad's diagonal, one of its two faces skipped"),
            ((2, 2, -1), (0, 0, 1), -1, 0, 1.5, 1, 0, "through the hypotenuse of the triangle"),
            ((-1, 0.5, 0), (1, 0, 0), -1, 0, inf, 0, 0, "in the plane of the triangle: det = 0, a miss"),
            ((-1, 1, 0.5), (1, 0, 0.25), -1, 0, inf, 1, 0, "slanted, across several cells"),
            ((1, 0.5, 0.5), (0, 0, 0), -1, 0, inf, 0, 2, "zero direction"),
            ((1, 0.5, 0.5), (nan, 0, 1), -1, 0, inf, 0, 2, "NaN direction"),
            ((1, 0.5, 0.5), (0, inf, 1), -1, 0, inf, 0, 2, "infinite direction"),
            ((1, nan, 0.5), (0, 0, 1), -1, 0, inf, 0, 2, "NaN origin"),
            ((-inf, 0.5, 0.5), (1, 0, 0), -1, 0, inf, 0, 2, "infinite origin")]
    return dict(verts=verts, faces=faces, rays=rays)


def random_rays(name, n=400, seed=3):
    """(origins, dirs, skip) float32 / int32: rays around a case's mesh, the first half starting on it (skip = their face; meant for
    t_min = t_min_of(case), which keeps a duplicated face from being a tie at t = 0), the second half from anywhere around it, every
    fifth of those with a zero component."""
    c = case(name)
    rng = np.random.default_rng(seed)
    t9 = tri9_of(c).astype(np.float64)
    lo, hi = t9.reshape(-1, 3).min(0), t9.reshape(-1, 3).max(0)
    o = rng.uniform(lo - 0.6 * (hi - lo), hi + 0.6 * (hi - lo), (n, 3))
    d = rng.normal(size=(n, 3))
    d[n // 2::5, rng.integers(0, 3)] = 0.0
    skip = np.full(n, -1, dtype=np.int32)
    f = rng.integers(0, len(t9), n // 2)
    b = rng.dirichlet((1.0, 1.0, 1.0), n // 2)
    o[:n // 2] = (b[:, :, None] * t9[f].reshape(-1, 3, 3)).sum(1)
    skip[:n // 2] = f
    return o.astype(np.float32), d.astype(np.float32), skip


def measure():
    """(gap, {case: share of rays left out}): the float32 / float64 gap of the pure numbers over every ray of every case (the
    mask's rays of each light with their float32 points, the random rays and the generic ones), and the restatement's left-out
    shares."""
    gap, shares = 0.0, {}
    for name in CASES:
        c = case(name)
        xy, iw, face_id, lit, left = restated(name)
        covered = face_id >= 0
        shares[name] = float(left[covered].mean()) if covered.any() else 0.0
        tri9, t_min = tri9_of(c), t_min_of(c)
        if not len(tri9):
            continue
        r64, r32 = mask_rays(c, xy, iw, face_id), mask_rays(c, xy, iw, face_id, np.float32)
        for light in np.asarray(c["lights"], dtype=np.float64):
            L = np.asarray(light[:3], dtype=np.float32).astype(np.float64)
            idx = np.nonzero(r64["N"] @ L > 0)[0]
            gap = max(gap, pair_gap(r64["P"][idx], r32["P"][idx], np.broadcast_to(L, (len(idx), 3)), r64["f"][idx], tri9, t_min, math.inf))
        o, d, skip = random_rays(name)
        gap = max(gap, pair_gap(o.astype(np.float64), o, d.astype(np.float64), skip, tri9, t_min, math.inf))
    return gap, shares
