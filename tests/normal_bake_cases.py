"""The yardstick of the baked normal map (s3d_tex_normal_texels, s3d_tex_dilate_nearest): a NumPy restatement of the
bake's seven steps and of the dilation, written from their specification for a number type `dt` (float64: the reference; float32:
what that arithmetic alone costs), injectable faults, the designed cases, and the checks as functions of arrays.  The conditions
on all of it are held by tests/test_normal_bake_host.py.

Steps (entry i, texel idx[i] = y * T + x): 1 face k and barycentrics from (x, y) by the expressions of s3d_tex_texel_positions
(float32, whatever `dt`: they are inputs of what follows); 2 g^ = g / |g|, status 2 when g is not finite or |g|^2 < 1e-20; 3 the
face normal Nf, status 3 without one; 4 s = +1 if Nf.g^ >= 0 else -1, Nf_o = s Nf; 5 N = s normalize(b0 n0 + b1 n1 + b2 n2), or
Nf_o with status 4 (no base normals, a zero corner normal, a mix that is not finite, N.Nf_o <= 0); 6 T' = normalize(T - N (N.T)),
B' = cross(N, T') sign(cross(N, T').B), status 3 when T = B = 0 or T' has no direction; 7 t = (g^.T', g^.B', g^.N), byte =
floor(clamp((t + 1) 127.5, 0, 255) + 0.5).  Status 2 and 3 write the flat texel (128, 128, 255).

FLOAT32 BOUND (float32_delta).  With u = 2^-24 and first-order terms only, for unit results: |dg^| <= 4u (three products, two
sums, a root, a quotient); the cross product of two rounded edges errs by 8u |e1||e2|, so |dNf| <= (8 kF + 4)u with
kF = |e1||e2| / |e1 x e2|; the mix errs by 3 sqrt(3) u sum(b_i |n_i|), so |dN| <= (3 sqrt(3) kM + 4)u with kM = sum(b_i |n_i|) /
|mix| (|dNf| where N is Nf_o); T - N (N.T) errs by |T| (6.5u + 2 |dN|), so |dT'| <= kT (6.5u + 2 |dN|) + 4u with kT = |T| /
|T - N (N.T)|; |dB'| <= |dN| + |dT'| + 6u; a dot product with g^ adds 3u, and (t + 1) 127.5 two roundings of at most 255u each.
delta_c = 127.5 (|dg^| + |dX_c| + 3u) + 510u for X = (T', B', N).  A byte may differ by one only where the float64 value lies
within delta of a rounding boundary k + 0.5; such texels may be at most MAX_CLOSE_SHARE of a case's encoded texels."""
import functools
import math

import numpy as np

import render_pbr_cases as P

FLAT = np.array([128, 128, 255], dtype=np.uint8)
ORDER = ((0, -1), (-1, 0), (1, 0), (0, 1), (-1, -1), (1, -1), (-1, 1), (1, 1))            # (dx, dy)
FAULTS = ("b_sign", "no_gram_schmidt", "no_orient", "swap_b", "trunc", "scale128")
DILATE_FAULTS = ("max", "four")
U32 = 2.0 ** -24
MAX_ANGLE_DEG = 0.40            # |dt_c| <= 1/255, |d| <= sqrt(3)/255, asin of it = 0.389 degrees; the rest is float32 slack
MAX_CLOSE_SHARE = 0.01
SHAPES = {"one": (1, 8), "two": (2, 8), "edge": (5, 37), "patch": (33, 100)}


# ------------------------------------------------------------------ the atlas
def atlas_layout(F, T):
    """(n cells per row, c texels per cell): n = ceil(sqrt(ceil(F / 2))), c = T // n"""
    half = (F + 1) // 2
    n = max(1, math.isqrt(half))
    if n * n < half:
        n += 1
    return n, T // n


def charts(F, T, n, c):
    """For every texel y * T + x: (face k or -1, u, v, upper) — lower chart lx >= 1, ly >= 1, lx + ly <= c - 4 with (u, v) =
    (lx, ly); upper chart lx <= c - 2, ly <= c - 2, lx + ly >= c + 2 with (u, v) = (c - 1 - lx, c - 1 - ly)."""
    p = np.arange(T * T, dtype=np.int64)
    x, y = p % T, p // T
    col, row = x // c, y // c
    lx, ly = x - col * c, y - row * c
    cell = row * n + col
    inside = (col < n) & (row < n)
    lower = inside & (lx >= 1) & (ly >= 1) & (lx + ly <= c - 4)
    upper = inside & ~lower & (lx <= c - 2) & (ly <= c - 2) & (lx + ly >= c + 2)
    k = np.where(lower, 2 * cell, np.where(upper, 2 * cell + 1, -1))
    k = np.where(k >= F, -1, k)
    u = np.where(upper, c - 1 - lx, lx)
    v = np.where(upper, c - 1 - ly, ly)
    return k, u, v, upper & (k >= 0)


def atlas_uvs(F, T, n, c, corner0):
    """float32 [F, 3, 2]: vertex j of face k sits on chart corner (j - corner0[k]) mod 3; corners in texels / T"""
    k = np.arange(F)
    cell = k // 2
    org = np.stack([(cell % n) * c, (cell // n) * c], 1)
    lower = np.asarray([[1, 1], [c - 4, 1], [1, c - 4]])
    upper = np.asarray([[c - 1, c - 1], [4, c - 1], [c - 1, 4]])
    corners = org[:, None, :] + np.where((k % 2 == 0)[:, None, None], lower[None], upper[None])
    which = (np.arange(3)[None, :] - np.asarray(corner0).reshape(-1, 1)) % 3
    return (np.take_along_axis(corners, which[:, :, None], 1) / float(T)).astype(np.float32)


# ------------------------------------------------------------------ restatement: the bake
def _dot(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def _normalize(v):
    """(v / |v| or v itself, ok): ok = the squared length is positive and finite"""
    l2 = _dot(v, v)
    ok = (l2 > 0) & np.isfinite(l2)
    ln = np.sqrt(np.where(ok, l2, 1))
    return np.where(ok[..., None], v / ln[..., None], v), ok


def bake(case, dt=np.float64, fault=None):
    """(image uint8 [T*T, 3], status uint8 [T*T], x): the undilated map of a case.  x holds, per entry that reached a face (x["p"]
    = its texel): val [E, 3] = (t + 1) 127.5 before clamping, ghat, frame [E, 3, 3] = (T', B', N), and kF, kM, kT, fallback of
    float32_delta."""
    assert fault is None or fault in FAULTS, fault
    with np.errstate(all="ignore"):
        return _bake(case, dt, fault)


def _bake(case, dt, fault):
    T, n, c, F = case["T"], case["n"], case["c"], case["F"]
    TT = T * T
    image, status = np.tile(FLAT, (TT, 1)), np.zeros(TT, dtype=np.uint8)
    idx = np.asarray(case["idx"], dtype=np.int64)
    assert len(np.unique(idx)) == len(idx)
    verts32, tris = np.asarray(case["verts"], dtype=np.float32), np.asarray(case["tris"], dtype=np.int64)
    k_all, u_all, v_all, up_all = charts(F, T, n, c)
    # ---- 1
    ent = np.flatnonzero((idx >= 0) & (idx < TT))
    ent = ent[k_all[idx[ent]] >= 0]
    p = idx[ent]
    k = k_all[p]
    r = np.clip(np.asarray(case["corner0"], dtype=np.int64)[k], 0, 2)
    vi = np.stack([tris[k, (r + j) % 3] for j in range(3)], 1)
    good = ((vi >= 0) & (vi < len(verts32))).all(1)
    ent, p, k, vi = ent[good], p[good], k[good], vi[good]
    L = np.float32(c - 5)
    b1 = (u_all[p].astype(np.float32) - np.float32(0.5)) / L
    b2 = (v_all[p].astype(np.float32) - np.float32(0.5)) / L
    b0 = np.float32(1.0) - b1 - b2
    if fault == "swap_b":
        b1, b2 = np.where(up_all[p], b2, b1), np.where(up_all[p], b1, b2)
    b0, b1, b2 = (b.astype(dt)[:, None] for b in (b0, b1, b2))
    # ---- 2
    g32 = np.asarray(case["grad"], dtype=np.float32)[ent]
    g = g32.astype(dt)
    l2 = _dot(g, g)
    st2 = ~np.isfinite(g32).all(1) | (l2 < dt(1e-20))
    ghat = g / np.sqrt(l2)[:, None]
    # ---- 3, 4
    V = verts32.astype(dt)
    e1, e2 = V[vi[:, 1]] - V[vi[:, 0]], V[vi[:, 2]] - V[vi[:, 0]]
    raw = _cross(e1, e2)
    Nf, ok_f = _normalize(raw)
    s = np.where(_dot(Nf, ghat) >= 0, dt(1.0), dt(-1.0))[:, None]
    if fault == "no_orient":
        s = np.ones_like(s)
    Nfo = s * Nf
    # ---- 5
    N, fallback = Nfo, np.ones(len(ent), dtype=bool)
    kM = np.ones(len(ent))
    if case.get("base") is not None:
        base32 = np.asarray(case["base"], dtype=np.float32)
        n0, n1, n2 = (base32[vi[:, j]] for j in range(3))
        any_zero = ~n0.any(1) | ~n1.any(1) | ~n2.any(1)
        mixed = b0 * n0.astype(dt) + b1 * n1.astype(dt) + b2 * n2.astype(dt)
        mix, ok_m = _normalize(mixed)
        mix = s * mix
        use = ~any_zero & ok_m & (_dot(mix, Nfo) > 0)
        N, fallback = np.where(use[:, None], mix, Nfo), ~use
        size = (np.abs(b0) * np.linalg.norm(n0, axis=1, keepdims=True) + np.abs(b1) * np.linalg.norm(n1, axis=1, keepdims=True) +
                np.abs(b2) * np.linalg.norm(n2, axis=1, keepdims=True))[:, 0]
        kM = np.where(use, size / np.where(use, np.linalg.norm(mixed, axis=1), 1), 1).astype(np.float64)
    # ---- 6
    tang = np.asarray(case["tangents"], dtype=np.float32)[k]
    Tg, Bg = tang[:, 0].astype(dt), tang[:, 1].astype(dt)
    none = ~tang.reshape(-1, 6).any(1)
    t_raw = Tg if fault == "no_gram_schmidt" else Tg - N * _dot(N, Tg)[:, None]
    Tp, ok_t = _normalize(t_raw)
    Bp = _cross(N, Tp)
    sg = np.where(_dot(Bp, Bg) < 0, dt(-1.0), dt(1.0))[:, None]
    if fault == "b_sign":
        sg = np.ones_like(sg)
    Bp = sg * Bp
    st3 = ~ok_f | none | ~ok_t
    # ---- 7
    val = (np.stack([_dot(ghat, Tp), _dot(ghat, Bp), _dot(ghat, N)], 1) + dt(1.0)) * dt(128.0 if fault == "scale128" else 127.5)
    q = np.minimum(np.maximum(val, dt(0.0)), dt(255.0))
    q = np.floor(q) if fault == "trunc" else np.floor(q + dt(0.5))
    st = np.where(st2, 2, np.where(st3, 3, np.where(fallback, 4, 1))).astype(np.uint8)
    enc = (st == 1) | (st == 4)
    image[p[enc]] = q[enc].astype(np.uint8)
    status[p] = st
    e1n, e2n, rawn = (np.linalg.norm(a.astype(np.float64), axis=1) for a in (e1, e2, raw))
    trn, tgn = np.linalg.norm(t_raw.astype(np.float64), axis=1), np.linalg.norm(Tg.astype(np.float64), axis=1)
    x = dict(p=p, entry=ent, k=k, status=st, val=val, ghat=ghat, frame=np.stack([Tp, Bp, N], 1), fallback=fallback, kM=kM,
             kF=np.where(rawn > 0, e1n * e2n / np.where(rawn > 0, rawn, 1), np.inf), kT=np.where(trn > 0, tgn / np.where(trn > 0, trn, 1), np.inf))
    return image, status, x


def float32_delta(x):
    """[E, 3]: the float32 bound of the module docstring on (t + 1) 127.5, from the float64 restatement's x"""
    u = U32
    d_nf = (8 * x["kF"] + 4) * u
    d_n = np.where(x["fallback"], d_nf, (3 * math.sqrt(3) * x["kM"] + 4) * u)
    d_t = x["kT"] * (6.5 * u + 2 * d_n) + 4 * u
    d_b = d_n + d_t + 6 * u
    return 127.5 * (4 * u + np.stack([d_t, d_b, d_n], 1) + 3 * u) + 510 * u


# ------------------------------------------------------------------ restatement: the dilation
def dilate_nearest(image, mask, fault=None):
    """image [T, T, C] (row y, column x), mask bool [T, T]: covered texels keep theirs, an uncovered one takes the texel of its
    first covered neighbour inside the image in ORDER, its own without one."""
    assert fault is None or fault in DILATE_FAULTS, fault
    img = np.asarray(image)
    T = img.shape[0]
    out = img.copy()
    for y, x in np.argwhere(~np.asarray(mask)):
        if fault == "max":
            out[y, x] = img[max(0, y - 1):y + 2, max(0, x - 1):x + 2].reshape(-1, img.shape[2]).max(0)
            continue
        for dx, dy in ORDER[:4] if fault == "four" else ORDER:
            xx, yy = x + dx, y + dy
            if 0 <= xx < T and 0 <= yy < T and mask[yy, xx]:
                out[y, x] = img[yy, xx]
                break
    return out


def bake_dilated(case, dt=np.float64):
    """(image [T, T, 3], status [T, T]) as isosurface.bake_normal_map returns them"""
    image, status, _ = bake(case, dt)
    T = case["T"]
    k_all = charts(case["F"], T, case["n"], case["c"])[0]
    return dilate_nearest(image.reshape(T, T, 3), (k_all >= 0).reshape(T, T)), status.reshape(T, T)


# ------------------------------------------------------------------ the checks
def check_bake(image, status, case, reference=None):
    """(problems: a list of strings, empty for none; the share of close texels; the number of bytes off by one) of an undilated
    result against the float64 restatement (`reference`: bake(case) of a case that is not one of BUILDERS): status equal
    everywhere; bytes equal, but for one level where the float64 value lies within float32_delta of k + 0.5."""
    ref_img, ref_st, x = ref(case["name"]) if reference is None else reference
    img, st = np.asarray(image).reshape(-1, 3), np.asarray(status).reshape(-1)
    problems = []
    bad = np.flatnonzero(st != ref_st)
    if len(bad):
        problems.append(f"status differs on {len(bad)} texels, first {bad[:4].tolist()}: {st[bad[:4]].tolist()} against {ref_st[bad[:4]].tolist()}")
    enc = (x["status"] == 1) | (x["status"] == 4)
    close_e = np.zeros((len(x["p"]), 3), dtype=bool)
    v = np.minimum(np.maximum(x["val"], 0.0), 255.0)
    close_e[enc] = (np.abs(v - (np.floor(v) + 0.5)) <= float32_delta(x))[enc]
    close = np.zeros((len(ref_img), 3), dtype=bool)
    close[x["p"]] = close_e
    diff = np.abs(img.astype(np.int64) - ref_img.astype(np.int64))
    wrong = (diff > 1) | ((diff == 1) & ~close)
    if wrong.any():
        w = np.argwhere(wrong)
        problems.append(f"bytes differ on {len(w)} entries, first (texel, channel) {w[:4].tolist()}: {img[wrong][:4].tolist()} against "
                        f"{ref_img[wrong][:4].tolist()}")
    share = close_e.any(1).sum() / max(1, enc.sum())
    if share > MAX_CLOSE_SHARE:
        problems.append(f"{close_e.any(1).sum()} of {enc.sum()} encoded texels lie within delta of a rounding boundary (at most {MAX_CLOSE_SHARE})")
    return problems, float(share), int((diff == 1).sum())


def decode_shader(bytes3, frame):
    """s3d_pbr_shade's rule on a texel: tx = 2 byte / 255 - 1, normalize(tx0 T' + tx1 B' + tx2 N) with B' signed"""
    tx = 2.0 * (np.asarray(bytes3, dtype=np.float64) / 255.0) - 1.0
    return _normalize(tx[:, 0:1] * frame[:, 0] + tx[:, 1:2] * frame[:, 1] + tx[:, 2:3] * frame[:, 2])[0]


def angle_deg(a, b):
    return np.degrees(np.arctan2(np.linalg.norm(_cross(a, b), axis=-1), _dot(a, b)))


def check_round_trip(image, case):
    """(problems, largest angle in degrees): the bytes decoded by the shader's rule in the restatement's frame against g^, on
    every texel of status 1 or 4"""
    _, _, x = ref(case["name"])
    enc = (x["status"] == 1) | (x["status"] == 4)
    img = np.asarray(image).reshape(-1, 3)[x["p"]]
    ang = angle_deg(decode_shader(img[enc], x["frame"][enc].astype(np.float64)), x["ghat"][enc].astype(np.float64))
    worst = float(ang.max(initial=0.0))
    problems = [] if worst <= MAX_ANGLE_DEG else [f"{(ang > MAX_ANGLE_DEG).sum()} texels decode more than {MAX_ANGLE_DEG} degrees away, worst {worst:.3f}"]
    return problems, worst


def check_dilate(out, image, mask):
    want = dilate_nearest(image, mask)
    bad = np.argwhere((np.asarray(out) != want).any(2))
    return [] if not len(bad) else [f"{len(bad)} texels differ, first (y, x) {bad[:4].tolist()}"]


# ------------------------------------------------------------------ the designed cases
def _unit(v):
    v = np.asarray(v, dtype=np.float64)
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _face_normals(verts, tris):
    v = np.asarray(verts, dtype=np.float64)
    n = np.cross(v[tris[:, 1]] - v[tris[:, 0]], v[tris[:, 2]] - v[tris[:, 0]])
    ln = np.linalg.norm(n, axis=1, keepdims=True)
    return np.where(ln > 0, n / np.where(ln > 0, ln, 1), 0)


def _finish(name, verts, tris, corner0, base, rng, side=None, extra_idx=(), tilt=0.4):
    """The case's dict: tangents of the atlas' own uvs, all covered texels (shuffled) and `extra_idx` as entries, gradients =
    (side[k] face normal + tilt noise) times a magnitude in [0.3, 3]."""
    F, T = SHAPES[name]
    n, c = atlas_layout(F, T)
    verts, tris = np.asarray(verts, dtype=np.float32), np.asarray(tris, dtype=np.int32)
    assert tris.shape == (F, 3) and c >= 8
    corner0 = np.asarray(corner0, dtype=np.int32)
    tangents = P.face_tangents(verts, tris, atlas_uvs(F, T, n, c, corner0)).astype(np.float32)
    k_all = charts(F, T, n, c)[0]
    covered = rng.permutation(np.flatnonzero(k_all >= 0))
    idx = np.concatenate([covered, np.asarray(extra_idx, dtype=np.int64)]).astype(np.int64)
    k = np.where((idx >= 0) & (idx < T * T), k_all[np.clip(idx, 0, T * T - 1)], -1)
    side = np.ones(F) if side is None else np.asarray(side, dtype=np.float64)
    fn = _face_normals(verts, tris)
    fn = np.where(np.abs(fn).sum(1, keepdims=True) > 0, fn, np.array([0.0, 0.0, 1.0]))
    grad = (side[k, None] * fn[k] + tilt * rng.standard_normal((len(idx), 3))) * rng.uniform(0.3, 3.0, size=(len(idx), 1))
    return dict(name=name, F=F, T=T, n=n, c=c, verts=verts, tris=tris, corner0=corner0, base=None if base is None else np.asarray(base, dtype=np.float32),
                tangents=tangents, idx=idx, grad=grad.astype(np.float32), face_of_entry=k)


def _one(rng):
    """one face, corner0 = 1, no base normals; entries outside [0, T^2) and on texels that no chart covers (texel 0; the upper
    chart of the cell, whose face 1 does not exist)"""
    T = SHAPES["one"][1]
    verts = [(0.1, 0.2, 0.3), (1.3, 0.1, 0.5), (0.2, 1.1, 0.9)]
    return _finish("one", verts, [(0, 1, 2)], [1], None, rng, extra_idx=[-1, -5, T * T, T * T + 7, 2 ** 40, 0, 6 * T + 6, 5 * T + 6])


def _two(rng):
    """both charts of one cell on vertices at offset 1000, corner0 = 2 and 0, smooth base normals; the field points against the
    winding of face 1"""
    verts = rng.uniform(-1, 1, size=(1004, 3))
    verts[1000:] = [(0.0, 0.1, 0.2), (1.1, 0.0, 0.3), (0.1, 1.2, 0.1), (1.2, 1.1, 0.6)]
    tris = np.asarray([(1000, 1001, 1002), (1002, 1001, 1003)])
    base = rng.standard_normal((1004, 3))
    fn = _face_normals(verts, tris)
    base[1000:] = _unit(_unit(fn[0] + fn[1])[None] + 0.25 * rng.standard_normal((4, 3)))
    return _finish("two", verts, tris, [2, 0], base, rng, side=[1, -1])


def _edge(rng):
    """five faces on vertices of their own: 0 an axis-aligned face with exact normals (its first entries: g = 0, NaN, inf,
    1e-11 e_z, and g parallel to T); 1 without area; 2 without tangent (a uv triangle without area); 3 with a zero base normal on
    a corner; 4 whose base normals point away from the field's side of the face"""
    verts = np.zeros((15, 3))
    verts[0:3] = [(0, 0, 1), (2, 0, 1), (0, 2, 1)]
    verts[3:6] = [(3, 0, 0), (4, 0, 0), (5, 0, 0)]
    verts[6:9] = [(0.2, 3.0, 0.1), (1.4, 3.1, 0.3), (0.3, 4.2, 0.5)]
    verts[9:12] = [(3.0, 3.0, 0.2), (4.1, 3.2, 0.0), (3.2, 4.3, 0.4)]
    verts[12:15] = [(6.0, 0.1, 0.3), (7.2, 0.0, 0.1), (6.1, 1.3, 0.6)]
    tris = np.arange(15).reshape(5, 3)
    fn = _face_normals(verts, tris)
    base = np.repeat(fn, 3, axis=0) + 0.2 * rng.standard_normal((15, 3))
    base[0:3] = (0, 0, 1)
    base[3:6] = (0, 0, 1)
    base = _unit(base)
    base[10] = 0
    base[12:15] = -base[12:15]
    case = _finish("edge", verts, tris, [0, 1, 2, 1, 0], base, rng)
    case["tangents"][2] = 0
    first = np.flatnonzero(case["face_of_entry"] == 0)
    assert len(first) > 12
    g = case["grad"]
    g[first[0]] = 0
    g[first[1]] = (np.nan, 1, 0)
    g[first[2]] = (0, np.inf, 1)
    g[first[3]] = (0, 0, 1e-11)
    g[first[4]] = (1e-11, 0, 0)
    g[first[5]] = np.float32(40.0) * case["tangents"][0, 0]            # (its t is (1, 0, 0) exactly: two values ON a rounding boundary)
    return case


def _patch(rng):
    """33 faces of a bumpy 5 x 5 height field (the last a repeat of the first the other way round), every corner0 value, a third of
    the windings against the field, smooth base normals with one zero and one NaN vertex: several blocks of entries"""
    F = SHAPES["patch"][0]
    j, i = np.meshgrid(np.arange(5), np.arange(5), indexing="ij")
    x, y = 0.5 * i.reshape(-1) - 1.0, 0.5 * j.reshape(-1) - 1.0
    verts = np.stack([x, y, 0.35 * np.sin(2.1 * x + 0.3) * np.cos(1.7 * y)], 1) + 0.02 * rng.standard_normal((25, 3))
    q = (j[:4, :4] * 5 + i[:4, :4]).reshape(-1)
    tris = np.concatenate([np.stack([q, q + 1, q + 6], 1), np.stack([q, q + 6, q + 5], 1)])
    tris = np.concatenate([tris[rng.permutation(32)], tris[:1, ::-1]])
    flip = np.arange(F) % 3 == 1
    tris[flip] = tris[flip][:, ::-1]
    up = np.where(_face_normals(verts, tris)[:, 2] > 0, 1.0, -1.0)          # the field's side: +z, whatever the winding
    dzdx = 0.35 * 2.1 * np.cos(2.1 * x + 0.3) * np.cos(1.7 * y)
    dzdy = -0.35 * 1.7 * np.sin(2.1 * x + 0.3) * np.sin(1.7 * y)
    base = _unit(np.stack([-dzdx, -dzdy, np.ones(25)], 1) + 0.1 * rng.standard_normal((25, 3)))
    base[7] = 0
    base[17] = (np.nan, 0, 1)
    return _finish("patch", verts, tris, np.arange(F) % 3, base, rng, side=up)


BUILDERS = {"one": (_one, 11), "two": (_two, 12), "edge": (_edge, 13), "patch": (_patch, 14)}


@functools.lru_cache(maxsize=None)
def case(name):
    build, seed = BUILDERS[name]
    return build(np.random.Generator(np.random.PCG64(seed)))


@functools.lru_cache(maxsize=None)
def ref(name):
    """the float64 restatement of a case: computed once, shared, never written to"""
    out = bake(case(name))
    for a in out[:2]:
        a.setflags(write=False)
    return out


def dilate_case(channels, seed=5, T=17):
    """(image [T, T, C], mask [T, T]): the mask on all four corners and on stretches of every border, isolated covered texels
    whose neighbours see them only across a corner, uncovered texels between covered ones of different values, and an empty
    region that no covered texel touches"""
    rng = np.random.Generator(np.random.PCG64(seed))
    image = rng.integers(0, 256, size=(T, T, channels), dtype=np.uint8)
    mask = rng.random((T, T)) < 0.3
    mask[9:15, 9:15] = False
    mask[12, 12] = True                                       # alone: all eight neighbours take it
    mask[[0, 0, -1, -1], [0, -1, 0, -1]] = True
    mask[0, 3:6] = mask[-1, 8:12] = mask[4:7, 0] = mask[10:13, -1] = True
    mask[0, 1:3] = mask[1:3, 0] = mask[-1, -3:-1] = mask[-3:-1, -1] = False
    return image, mask


# ------------------------------------------------------------------ the analytic sphere
def octasphere(levels):
    """(verts float32 [V, 3] on the unit sphere, faces int32 [8 * 4^levels, 3], outward): an octahedron, every face cut in four
    `levels` times, the new vertices pushed onto the sphere"""
    v = [np.asarray(p, dtype=np.float64) for p in ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1))]
    f = [(0, 2, 4), (2, 1, 4), (1, 3, 4), (3, 0, 4), (2, 0, 5), (1, 2, 5), (3, 1, 5), (0, 3, 5)]
    for _ in range(levels):
        mid, nf = {}, []

        def midpoint(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                m = v[a] + v[b]
                v.append(m / np.linalg.norm(m))
                mid[key] = len(v) - 1
            return mid[key]
        for a, b, c in f:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return np.asarray(v, dtype=np.float32), np.asarray(f, dtype=np.int32)


def normal_pass_vectors(rgba):
    """(unit vectors [..., 3], covered [...]) of a `normal` pass: rgb = 0.5 N + 0.5, alpha 255 = fully covered"""
    a = np.asarray(rgba)
    vec = a[..., :3].astype(np.float64) / 255.0 * 2.0 - 1.0
    return vec / np.maximum(np.linalg.norm(vec, axis=-1, keepdims=True), 1e-12), a[..., 3] == 255


def mean_angle_deg(rgba, rgba_ref, keep):
    a, b = normal_pass_vectors(rgba)[0][keep], normal_pass_vectors(rgba_ref)[0][keep]
    return float(angle_deg(a, b).mean())
