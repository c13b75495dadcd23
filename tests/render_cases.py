"""The yardstick of the mesh rasteriser (s3d_render.hip): a plain Python / NumPy restatement and the procedural
cases.  Coverage is decided with Python integers on the snapped coordinates by the fill rule of include/sin3dm_hip.h; depth,
barycentrics, texture lookup and shading are float64.

The depth band.  face_id is compared wherever depth decides clearly: a sample is left out only when the restatement's two nearest
covering triangles have 1 / w within DEPTH_BAND (relative).  The band is measured, not guessed: the depth formula (edge values as
weights of the corners' 1 / w, divided by the doubled area) evaluated in float32 and in float64 on every covering (sample,
triangle) of every case below differs by at most DEPTH_GAP relative (measure_depth_gap(), held by test_render_host.py);
the band is ten times that, the project's custom."""
import functools
import math

import numpy as np

SUB, HALF, MAX_COORD, TILE = 256, 128, 1 << 20, 16
AMBIENT, DIFFUSE = 0.35, 0.65
GRIDS = {"g64": (64, 48, 2), "g50": (50, 37, 1)}             # sample grid Ws x Hs and the supersampling factor
DEPTH_GAP = 1.8e-07                                          # the largest measured relative float32 / float64 gap (measure_depth_gap: 1.76e-07)
DEPTH_BAND = 10 * DEPTH_GAP
MAX_LEFT_OUT = 0.005                                         # share of a case's covered samples the band may leave out
OK, NEAR, RANGE, DEGENERATE = 0, 1, 2, 3

SCREEN = np.array([[1.0, 0, 0, 0], [0, 1.0, 0, 0], [0, 0, 1.0, 0], [0, 0, 1.0, 0]])      # clip = (X, Y, Z, Z): camera along +z
SCREEN_LIGHT = np.array([0.2, 0.4, -1.0]) / math.sqrt(0.2 ** 2 + 0.4 ** 2 + 1.0)
SCREEN_NEAR = 0.01


# ------------------------------------------------------------------ the rig, restated (blender_render_multiview.py:43-52, 92-104)
def rig_camera_position(azimuth, elevation, d=3.0):
    phi, theta = azimuth / 180 * math.pi, elevation / 180 * math.pi
    return np.array([d * math.sin(theta) * math.cos(phi), d * math.sin(theta) * math.sin(phi), d * math.cos(theta)])


def rig_normalize(points):
    """The reference's normalisation of points [N, 3]: rotate 90 degrees about x, centre the bounding box, scale."""
    p = np.stack([points[:, 0], -points[:, 2], points[:, 1]], 1)
    lo, hi = p.min(0), p.max(0)
    return (p - (lo + hi) / 2) / ((hi - lo).max() / 2 * 1.03)


def rig_project(points_world, eye, W, H):
    """(ndc x, ndc y, distance along the view) of normalised points for the camera at `eye`: 45 mm lens, 36 mm sensor on the
    larger image side, looking at the origin, z up."""
    f = -eye / np.linalg.norm(eye)
    r = np.cross(f, [0.0, 0.0, 1.0])
    r /= np.linalg.norm(r)
    u = np.cross(r, f)
    q = points_world - eye
    w = q @ f
    s = 2 * 45.0 / 36.0 * max(W, H)
    return (q @ r) * s / W / w, (q @ u) * s / H / w, w


def rig_matrix(points, azimuth, elevation, W, H):
    """Object-to-clip matrix of one view: rig_project after rig_normalize as one matrix (test_render_host.py holds it to them)."""
    p = np.asarray(points, dtype=np.float64)
    rot = np.stack([p[:, 0], -p[:, 2], p[:, 1]], 1)
    lo, hi = rot.min(0), rot.max(0)
    scale = 1.0 / ((hi - lo).max() / 2 * 1.03)
    R = np.array([[1.0, 0, 0], [0, 0, -1.0], [0, 1.0, 0]])
    A, b = R * scale, -(lo + hi) / 2 * scale
    eye = rig_camera_position(azimuth, elevation)
    f = -eye / np.linalg.norm(eye)
    r = np.cross(f, [0.0, 0.0, 1.0])
    r /= np.linalg.norm(r)
    u = np.cross(r, f)
    s = 2 * 45.0 / 36.0 * max(W, H)
    view = np.zeros((4, 4))
    view[0, :3], view[0, 3] = r * s / W, -r @ eye * s / W
    view[1, :3], view[1, 3] = u * s / H, -u @ eye * s / H
    view[3, :3], view[3, 3] = f, -f @ eye
    view[2] = view[3]
    model = np.eye(4)
    model[:3, :3], model[:3, 3] = A, b
    return view @ model


RIG_LIGHT = np.array([0.0, 1.0, 0.0])                        # +z after the rotation, in the stored mesh's axes
RIG_NEAR = 0.1


# ------------------------------------------------------------------ restatement
def project(verts, matrix, Ws, Hs, near):
    """(xy: int64 [V, 2] snapped sample coordinates, iw: float64 [V], 0 = flagged) of float32 vertices by a float64 matrix."""
    v = np.asarray(verts, dtype=np.float32).astype(np.float64).reshape(-1, 3)
    m = np.asarray(matrix, dtype=np.float64)
    clip = v @ m[:, :3].T + m[:, 3]
    w = clip[:, 3]
    ok = w > near
    ws = np.where(ok, w, 1.0)
    sx, sy = (clip[:, 0] / ws * 0.5 + 0.5) * Ws, (0.5 - clip[:, 1] / ws * 0.5) * Hs
    xy = np.stack([np.rint(sx * SUB), np.rint(sy * SUB)], 1)
    xy = np.where(ok[:, None], np.clip(xy, -2.0 ** 30, 2.0 ** 30), 0).astype(np.int64)
    return xy, np.where(ok, 1.0 / ws, 0.0)


def setup(xy, iw, faces, f):
    """(status, corners, swapped): corners = three (x, y, 1 / w, vertex) with Python integer coordinates, ordered so that the
    doubled area is positive."""
    V = len(xy)
    idx = [int(i) for i in faces[f]]
    if any(i < 0 or i >= V for i in idx):
        return RANGE, None, False
    if any(not iw[i] > 0 for i in idx):
        return NEAR, None, False
    c = [(int(xy[i][0]), int(xy[i][1]), float(iw[i]), i) for i in idx]
    if any(abs(p[0]) > MAX_COORD or abs(p[1]) > MAX_COORD for p in c):
        return RANGE, None, False
    area2 = (c[1][0] - c[0][0]) * (c[2][1] - c[0][1]) - (c[1][1] - c[0][1]) * (c[2][0] - c[0][0])
    if area2 == 0:
        return DEGENERATE, None, False
    if area2 < 0:
        return OK, [c[0], c[2], c[1]], True
    return OK, c, False


def edges(c):
    """[(A, B, C, top_left)] of the edges 1->2, 2->0, 0->1 (the weights of corners 0, 1, 2), inside positive."""
    out = []
    for a, b in ((1, 2), (2, 0), (0, 1)):
        dx, dy = c[b][0] - c[a][0], c[b][1] - c[a][1]
        A, B = -dy, dx
        out.append((A, B, -(A * c[a][0] + B * c[a][1]), dy > 0 or (dy == 0 and dx < 0)))
    return out


def edge_values(ed, px, py):
    return [A * px + B * py + C for A, B, C, _ in ed]


def covers(ed, E):
    return all(e > 0 or (e == 0 and tl) for e, (_, _, _, tl) in zip(E, ed))


def raster(xy, iw, faces, Ws, Hs, band=DEPTH_BAND):
    """dict: count int [Hs, Ws] (not clamped), face_id [Hs, Ws] (nearest, the lower index on equal depth; -1 none), depth float64,
    unclear bool [Hs, Ws] (the two nearest covering triangles differ by no more than band, relative, and are not equal),
    status [F], gap (the largest relative float32 / float64 gap of the depth formula over every covering pair)."""
    F = len(faces)
    count = np.zeros((Hs, Ws), dtype=np.int64)
    status = np.zeros(F, dtype=np.int64)
    rec = []                                               # (sample index, face, E0, E1, E2, iw0, iw1, iw2, area2)
    for f in range(F):
        st, c, _ = setup(xy, iw, faces, f)
        status[f] = st
        if st != OK:
            continue
        ed = edges(c)
        xs, ys = [p[0] for p in c], [p[1] for p in c]
        i0, i1 = max(0, -((-(min(xs) - HALF)) // SUB)), min(Ws - 1, (max(xs) - HALF) // SUB)
        j0, j1 = max(0, -((-(min(ys) - HALF)) // SUB)), min(Hs - 1, (max(ys) - HALF) // SUB)
        for j in range(j0, j1 + 1):
            for i in range(i0, i1 + 1):
                E = edge_values(ed, i * SUB + HALF, j * SUB + HALF)
                if covers(ed, E):
                    count[j, i] += 1
                    rec.append((j * Ws + i, f, E[0], E[1], E[2], c[0][2], c[1][2], c[2][2], sum(E)))
    face_id = np.full(Hs * Ws, -1, dtype=np.int64)
    depth = np.zeros(Hs * Ws)
    unclear = np.zeros(Hs * Ws, dtype=bool)
    gap = 0.0
    if rec:
        s = np.array([r[0] for r in rec])
        fc = np.array([r[1] for r in rec])
        E = np.array([r[2:5] for r in rec], dtype=np.int64)
        w = np.array([r[5:8] for r in rec], dtype=np.float64)
        a2 = np.array([r[8] for r in rec], dtype=np.int64)
        z = (E[:, 0] * w[:, 0] + E[:, 1] * w[:, 1] + E[:, 2] * w[:, 2]) / a2
        E32, w32 = E.astype(np.float32), w.astype(np.float32)
        z32 = (E32[:, 0] * w32[:, 0] + E32[:, 1] * w32[:, 1] + E32[:, 2] * w32[:, 2]) / a2.astype(np.float32)
        assert z32.dtype == np.float32
        gap = float(np.max(np.abs(z32.astype(np.float64) - z) / z))
        order = np.lexsort((fc, -z, s))                    # by sample, then nearest first, then the lower face
        s, fc, z = s[order], fc[order], z[order]
        first = np.ones(len(s), dtype=bool)
        first[1:] = s[1:] != s[:-1]
        face_id[s[first]], depth[s[first]] = fc[first], z[first]
        second = np.zeros(len(s), dtype=bool)
        second[1:] = first[:-1] & ~first[1:]
        k = np.nonzero(second)[0]
        d = z[k - 1] - z[k]
        unclear[s[k]] = (d > 0) & (d <= band * z[k - 1])
    return {"count": count, "face_id": face_id.reshape(Hs, Ws), "depth": depth.reshape(Hs, Ws), "unclear": unclear.reshape(Hs, Ws),
            "status": status, "gap": gap}


def tex_bilinear(img, u, v):
    """float64 [3] in [0, 1]: the GL convention of include/sin3dm_hip.h on a uint8 [H, W, 3] image with row 0 on top."""
    H, W = img.shape[:2]
    x, y = min(max(u * W - 0.5, -1.0), float(W)), min(max((1.0 - v) * H - 0.5, -1.0), float(H))
    xf, yf = math.floor(x), math.floor(y)
    fx, fy = x - xf, y - yf
    x0, x1 = min(max(int(xf), 0), W - 1), min(max(int(xf) + 1, 0), W - 1)
    y0, y1 = min(max(int(yf), 0), H - 1), min(max(int(yf) + 1, 0), H - 1)
    c = img.astype(np.float64)
    top = c[y0, x0] + fx * (c[y0, x1] - c[y0, x0])
    bot = c[y1, x0] + fx * (c[y1, x1] - c[y1, x0])
    return (top + fy * (bot - top))[:3] / 255.0


def shade(case, xy, iw, face_id, Ws, Hs, ss):
    """(rgba uint8 [H, W, 4], base float64 [Hs, Ws, 3] the unlit base colour per sample, NaN where nothing covers)."""
    verts = np.asarray(case["verts"], dtype=np.float32).astype(np.float64)
    faces, m, light = case["faces"], np.asarray(case["matrix"]), np.asarray(case["light"], dtype=np.float64)
    front_sign = -1 if np.linalg.det(m[[0, 1, 3]][:, :3]) < 0 else 1
    vcol, uvs, mats, fmat = case.get("vertex_colors"), case.get("uvs"), case.get("materials"), case.get("face_mat")
    lit = np.zeros((Hs, Ws, 3))
    base = np.full((Hs, Ws, 3), np.nan)
    for j in range(Hs):
        for i in range(Ws):
            f = int(face_id[j, i])
            if f < 0:
                continue
            st, c, swapped = setup(xy, iw, faces, f)
            assert st == OK
            E = edge_values(edges(c), i * SUB + HALF, j * SUB + HALF)
            n = [E[k] * c[k][2] for k in range(3)]
            b = [x / sum(n) for x in n]
            corner = (0, 2, 1) if swapped else (0, 1, 2)    # corner k of the ordered triangle in the face's own order
            col = np.ones(3)
            if vcol is not None:
                col = sum(b[k] * np.asarray(vcol, dtype=np.float32).astype(np.float64)[c[k][3]] for k in range(3))
            elif mats:
                mat = mats[int(fmat[f]) if fmat is not None else 0]
                col = np.asarray(mat.get("Kd", (1.0, 1.0, 1.0)), dtype=np.float32).astype(np.float64)
                if mat.get("image") is not None and uvs is not None:
                    q = np.asarray(uvs, dtype=np.float32).astype(np.float64)[f]
                    uv = sum(b[k] * q[corner[k]] for k in range(3))
                    col = tex_bilinear(mat["image"], uv[0], uv[1])
            a, p, q = (verts[int(v)] for v in faces[f])
            nrm = np.cross(p - a, q - a)
            ln = np.linalg.norm(nrm)
            lam = 0.0
            if ln > 0:
                d = float(nrm @ light) / ln
                lam = max(d if (-1 if swapped else 1) * front_sign > 0 else -d, 0.0)
            base[j, i] = col
            lit[j, i] = np.clip(col * (AMBIENT + DIFFUSE * lam), 0.0, 1.0)
    H, W = Hs // ss, Ws // ss
    rgba = np.zeros((H, W, 4), dtype=np.uint8)
    cov = (face_id >= 0).reshape(H, ss, W, ss)
    n_cov = cov.sum((1, 3))
    total = lit.reshape(H, ss, W, ss, 3).sum((1, 3))
    mean = np.where(n_cov[..., None] > 0, total / np.maximum(n_cov, 1)[..., None], 0.0)
    rgba[..., :3] = np.floor(mean * 255.0 + 0.5).astype(np.uint8)
    rgba[..., 3] = np.floor(n_cov / float(ss * ss) * 255.0 + 0.5).astype(np.uint8)
    return rgba, base


# ------------------------------------------------------------------ procedural cases
def screen_verts(points, Ws, Hs):
    """float32 [N, 3] vertices that SCREEN projects to the sample coordinates (sx, sy) at depth w of points [(sx, sy, w)]."""
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    return np.stack([(2 * p[:, 0] / Ws - 1) * p[:, 2], (1 - 2 * p[:, 1] / Hs) * p[:, 2], p[:, 2]], 1).astype(np.float32)


def _screen_case(points, faces, Ws, Hs, **extra):
    return dict(verts=screen_verts(points, Ws, Hs), faces=np.asarray(faces, dtype=np.int32).reshape(-1, 3), matrix=SCREEN, light=SCREEN_LIGHT,
                near=SCREEN_NEAR, **extra)


def icosphere(levels):
    t = (1 + math.sqrt(5)) / 2
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8), (3, 9, 4), (3, 4, 2),
         (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.asarray(p, dtype=np.float64) / np.linalg.norm(p) for p in v]
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
    return np.asarray(v), np.asarray(f, dtype=np.int32)


def _fan_quad(Ws, Hs):
    cx, cy, R = 14.5, 18.5, 12.0
    rim = [(cx + R, cy)] + [(round((cx + R * math.cos(a)) * 4) / 4, round((cy + R * math.sin(a)) * 4) / 4)
                            for a in (0.9, 1.7, 2.6)] + [(cx - R, cy), (cx - 7.0, cy - 7.0), (cx, cy - R), (cx + 6.0, cy - 6.0)]
    pts = [(cx, cy, 1.5)] + [(x, y, 1.0 + 0.1 * k) for k, (x, y) in enumerate(rim)]
    n = len(rim)
    faces = [(0, 1 + k, 1 + (k + 1) % n) for k in range(n)]
    outer = [(1,)] * n
    q = len(pts)
    pts += [(30.5, 4.5, 1.0), (44.5, 4.5, 1.2), (44.5, 18.5, 1.4), (30.5, 18.5, 1.1)]
    faces += [(q, q + 1, q + 2), (q, q + 2, q + 3)]
    outer += [(0, 1), (1, 2)]
    return _screen_case(pts, faces, Ws, Hs, outer=outer)


def _sphere(Ws, Hs, ss, levels=2, duplicate=False):
    v, f = icosphere(levels)
    verts = (v * np.array([0.5, 0.4, 0.3]) + np.array([0.2, -0.1, 0.4])).astype(np.float32)
    cols = (0.5 + 0.5 * v).astype(np.float32)
    if duplicate:
        f = np.concatenate([f, f])
    return dict(verts=verts, faces=f, matrix=rig_matrix(verts.astype(np.float64), 45.0, 45.0, Ws // ss, Hs // ss), light=RIG_LIGHT, near=RIG_NEAR,
                vertex_colors=cols)


def _slivers(Ws, Hs):
    pts, faces = [], []

    def tri(a, b, c, w):
        k = len(pts)
        pts.extend([(a[0], a[1], w), (b[0], b[1], w + 0.2), (c[0], c[1], w + 0.1)])
        faces.append((k, k + 1, k + 2))
    tri((2.1, 5.3), (40.7, 5.45), (2.1, 5.6), 1.0)                  # thinner than a sample, along a row of centres
    tri((3.0, 9.2), (45.0, 20.3), (3.2, 9.5), 1.3)                  # thin and slanted
    tri((20.45, 2.0), (20.55, 33.0), (20.6, 2.0), 1.1)              # along a column of centres
    tri((10.6, 10.6), (10.9, 10.7), (10.7, 10.9), 1.0)              # between four centres: no sample
    tri((30.55, 12.55), (31.45, 12.6), (30.9, 13.45), 1.0)          # between four centres: no sample
    tri((25.4, 25.4), (25.6, 25.45), (25.5, 25.6), 1.0)             # around one centre
    tri((12.5, 28.5), (13.5, 28.5), (12.5, 29.5), 1.0)              # corners on centres
    tri((5.0, 30.0), (48.0, 30.4), (5.0, 30.8), 2.0)                # a long wedge
    return _screen_case(pts, faces, Ws, Hs)


def _clamped(Ws, Hs):
    pts = [(-200.0, -150.0, 2.0), (300.0, -100.0, 2.5), (20.0, 400.0, 3.0), (-20.0, 10.0, 1.5), (25.0, 5.0, 1.2), (10.0, 30.0, 1.4)]
    return _screen_case(pts, [(0, 1, 2), (3, 4, 5)], Ws, Hs)


def _crowd(Ws, Hs, n=600):
    rng = np.random.default_rng(5)
    p = rng.uniform(16.2, 31.8, (n, 1, 2)) + rng.uniform(-2.0, 2.0, (n, 3, 2))
    p = np.clip(p, 16.05, 31.95)                                    # every box inside tile (1, 1)
    w = rng.uniform(1.0, 3.0, (n, 3, 1))
    return _screen_case(np.concatenate([p, w], 2).reshape(-1, 3), np.arange(3 * n).reshape(-1, 3), Ws, Hs)


def _nothing(Ws, Hs, empty):
    pts = [(-50.0, 5.0, 1.0), (-10.0, 8.0, 1.0), (-30.0, 30.0, 1.0)]
    return _screen_case(pts, np.zeros((0, 3), dtype=np.int32) if empty else [(0, 1, 2)], Ws, Hs)


def _behind(Ws, Hs):
    pts = [(5.0, 5.0, 1.0), (25.0, 6.0, 1.0), (8.0, 25.0, 1.0), (30.0, 10.0, 1.0), (45.0, 12.0, 0.001), (33.0, 30.0, 1.0)]
    return _screen_case(pts, [(0, 1, 2), (3, 4, 5)], Ws, Hs)


def _stack(Ws, Hs, n=300):
    pts = [(20.0, 20.0, 1.0), (26.0, 21.0, 1.0), (22.0, 27.0, 1.0)]
    return _screen_case(pts, [(0, 1, 2)] * n, Ws, Hs)


def texture_image():
    j, i = np.meshgrid(np.arange(8), np.arange(8), indexing="ij")
    return np.stack([i * 32 + 8, j * 32 + 8, (i * 8 + j) * 4], 2).astype(np.uint8)       # [row j from the top][column i]


def _textured(Ws, Hs):
    pts = [(8.0, 6.0, 1.0), (40.0, 6.0, 2.0), (40.0, 30.0, 2.0), (8.0, 30.0, 1.0)]       # top-left, top-right, bottom-right, bottom-left
    pts += [(41.5, 8.0, 1.5), (48.5, 8.0, 1.5), (48.5, 28.0, 1.2), (41.5, 28.0, 1.2)]    # a second material without image beside it
    uv = {0: (0.0, 1.0), 1: (1.0, 1.0), 2: (1.0, 0.0), 3: (0.0, 0.0)}
    faces = [(0, 1, 2), (0, 2, 3), (4, 5, 6), (4, 6, 7)]
    uvs = np.asarray([[uv.get(v, (0.3, 0.3)) for v in f] for f in faces], dtype=np.float32)
    return _screen_case(pts, faces, Ws, Hs, uvs=uvs, face_mat=np.asarray([0, 0, 1, 1], dtype=np.int32),
                        materials=[{"Kd": (0.5, 0.5, 0.5), "image": texture_image()}, {"Kd": (0.2, 0.6, 0.9), "image": None}])


CASES = {"a_fan": lambda g: _fan_quad(*g[:2]), "b_sphere": lambda g: _sphere(*g), "c_slivers": lambda g: _slivers(*g[:2]),
         "d_clamped": lambda g: _clamped(*g[:2]), "e_crowd": lambda g: _crowd(*g[:2]), "f_twice": lambda g: _sphere(*g, levels=1, duplicate=True),
         "g_off": lambda g: _nothing(*g[:2], False), "g_empty": lambda g: _nothing(*g[:2], True), "h_behind": lambda g: _behind(*g[:2]),
         "i_textured": lambda g: _textured(*g[:2]), "k_stack": lambda g: _stack(*g[:2])}
COMPARED_IN_FULL = ("f_twice", "k_stack")                             # equal inputs give exactly equal depths: no sample is left out


@functools.lru_cache(maxsize=None)
def case(name, grid):
    return CASES[name](GRIDS[grid])


@functools.lru_cache(maxsize=None)
def restated(name, grid):
    """The restatement on its own float64 projection: (xy, iw, raster dict).  Shared by the tests and left unchanged."""
    c = case(name, grid)
    Ws, Hs, _ = GRIDS[grid]
    xy, iw = project(c["verts"], c["matrix"], Ws, Hs, c["near"])
    return xy, iw, raster(xy, iw, c["faces"], Ws, Hs)


def measure_depth_gap():
    return max(restated(n, g)[2]["gap"] for n in CASES for g in GRIDS)
