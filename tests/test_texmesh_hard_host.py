"""CPU-only: the restatements, inputs and checks of the textured export's hard cases (tests/texmesh_cases.py), before
any device sees them:

  * the restatements give the hand-computed answers on small cases;
  * the inputs have the properties the GPU tests rely on (three different grid sizes, vertices on cell faces, a band of at
    most 1 % of the random faces, ...);
  * every check of tests/test_texmesh_hard_gpu.py passes on the clean NumPy model of the device and reports the model with one
    fault put in, for every listed fault.  One fault is asserted to be none: a dilation that lets neighbours outside the image
    take part as 0."""
import numpy as np
import pytest

import texmesh_cases as M
from test_texmesh_host import rasterise


def caught(check, *args):
    try:
        check(*args)
    except AssertionError:
        return True
    return False


# ------------------------------------------------------------------ keys
def test_keys_by_hand():
    """box 8 x 5 x 3 from the origin, s = 1: (3, 2, 1) lies on three cell faces and belongs to the cell above them; one ulp below 3
    it is the cell before; the box maximum is clamped into the last cell; below the origin into the first"""
    v = np.asarray([[3, 2, 1], [np.nextafter(np.float32(3), np.float32(0)), 2, 1], [8, 5, 3], [-1e-30, 0, 0], [2.999, 4.5, 2.5]], np.float32)
    want = [(3 * 5 + 2) * 3 + 1, (2 * 5 + 2) * 3 + 1, (7 * 5 + 4) * 3 + 2, 0, (2 * 5 + 4) * 3 + 2]
    assert M.np_keys(v, [0, 0, 0], 1.0, [8, 5, 3]).tolist() == want
    assert M.np_grid([8, 5, 3], 8) == (np.float32(1), [8, 5, 3]) and M.np_grid([8, 5, 0], 7)[1] == [7, 5, 1]
    from sin3dm_amd.encoding.isosurface import cluster_grid
    for ext in ([8, 5, 3], [8, 5, 0], [0.3, 12, 9]):
        for R in (1, 2, 7, 8, 13, 1000, 1 << 20):
            s, dims = cluster_grid(np.asarray(ext, np.float32), R)
            assert (np.float32(s), dims) == M.np_grid(ext, R)


# the sets on which a fault of the keys must show: a reciprocal and a double division only where s is inexact
KEY_FAULT_SHOWS = {"reciprocal": ("box_R7", "box_R13", "offset_R13"), "float64": ("box_R7", "box_R13"), "no_clamp": M.KEY_CASES,
                   "swapped_dims": M.KEY_CASES}


@pytest.mark.parametrize("name", M.KEY_CASES)
def test_key_cases(name):
    c = M.key_case(name)
    assert len(set(c.dims)) == 3, c.dims                                     # a swapped linearisation shows
    assert (name == "sheet_R8") == (c.dims[2] == 1)
    q = (c.verts.astype(np.float64) - c.origin) / float(c.s)
    on_face = np.abs(q - np.round(q)).min(1)
    assert c.unmoved >= 400
    if c.s == 1:
        assert (on_face[:c.unmoved] == 0).all()                              # the unmoved ones: every vertex really on a cell face
        assert (c.verts[:c.unmoved] == c.origin + c.extent).all(1).any()     # the box maximum is there
    else:
        assert (on_face < 1e-6).sum() >= 3 * sum(c.dims)                     # fp32(k s) and its neighbours
    M.check_keys(c, c.keys())
    for fault in M.KEY_FAULTS:
        assert caught(M.check_keys, c, c.keys(fault)) == (name in KEY_FAULT_SHOWS[fault]), fault
    assert set(M.KEY_FAULTS) == set(KEY_FAULT_SHOWS)


# ------------------------------------------------------------------ means
@pytest.mark.parametrize("name,C", M.MEAN_CASES)
def test_mean_cases(name, C):
    c = M.mean_case(name, C)
    assert c.vals.shape[1] == 3 + C and np.abs(c.vals[:, :3] - 1000).max() < 0.01
    n = np.diff(c.seg)
    assert (n.max() == 50000 and len(n) == 1) if name == "one_cluster" else (set(n.tolist()) == {0, 1, 2, 3})
    assert not np.array_equal(c.order, np.sort(c.order))
    clean = M.np_means(c.vals, c.order, c.seg)
    print(f"{c.name}: double accumulator, worst ratio to the bound {M.check_means(c, clean):.3f}")
    for fault, where in M.MEAN_FAULTS.items():
        if where == name:
            assert caught(M.check_means, c, M.np_means(c.vals, c.order, c.seg, fault)), fault
    if name == "small_clusters":
        bad = clean.copy()
        bad[np.flatnonzero(n == 0)[0]] = 1e-30
        assert caught(M.check_means, c, bad)


def test_means_by_hand():
    vals = np.asarray([[16777216.0], [1.0], [1.0], [2.0], [3.0], [4.0]], np.float32)
    order, seg = [0, 1, 2, 3, 5, 4], [0, 4, 4, 6]
    assert M.np_means(vals, order, seg).tolist() == [[4194305.0], [0.0], [3.5]]          # (2^24 + 4) / 4: the double sum keeps the ones
    assert M.np_means(vals, order, seg, "float32_accumulator")[0, 0] == 4194304.5        # 2^24 + 1 -> 2^24, twice
    mixed = [5, 1, 2, 3, 0, 4]                                                           # clusters {4, 1, 1, 2} and {2^24, 3}
    assert M.np_means(vals, mixed, seg).tolist() == [[2.0], [0.0], [8388610.0]]          # (2^24 + 3) / 2 = 8388609.5 -> even
    assert M.np_means(vals, mixed, seg, "unsorted").tolist() == [[4194305.0], [0.0], [3.5]]        # vals[b:e], not vals[order[b:e]]
    assert M.ulp32(1.0) == 2.0 ** -23 and M.ulp32(0.99) == 2.0 ** -24 and M.ulp32(1000.0) == 2.0 ** -14 and M.ulp32(0.0) == 2.0 ** -149


# ------------------------------------------------------------------ faces
def test_faces_by_hand():
    t = np.asarray([[0, 1, 2], [1, 2, 0], [2, 1, 0], [3, 2, 1], [0, 0, 1], [1, 2, 3], [4, 3, 2]])
    ident = np.arange(5)
    assert M.np_faces(t, ident).tolist() == [[0, 1, 2], [3, 2, 1], [4, 3, 2]]
    assert M.np_faces(t, ident, "keep_last").tolist() == [[2, 1, 0], [1, 2, 3], [4, 3, 2]]
    assert M.np_faces(t, ident, "sorted_triple").tolist() == [[0, 1, 2], [1, 2, 3], [2, 3, 4]]
    assert M.np_faces(t, np.asarray([0, 0, 1, 2, 2])).tolist() == [[2, 1, 0]]      # (3,2,1) -> (2,1,0) first; (1,2,3) -> (0,1,2) is its set
    assert len(M.np_faces(t, np.zeros(5, np.int64))) == 0


@pytest.mark.parametrize("name", M.FACE_CASES)
def test_face_cases(name):
    c = M.face_case(name)
    F = c.n_first
    assert len(c.tris) > c.n_faces and len(c.tris) % F == 0
    for rep in range(1, len(c.tris) // F):                                   # every face again, as another ordering of the same set
        assert np.array_equal(np.sort(c.tris[rep * F:(rep + 1) * F], 1), np.sort(c.tris[:F], 1))
        assert (c.tris[rep * F:(rep + 1) * F] != c.tris[:F]).any(1).all()
    if name.startswith("double_sided"):
        assert np.array_equal(c.tris[F:], c.tris[:F, ::-1])
        assert c.long_bisection or c.n_faces < len(c.tris) // 2             # a budget below half the face count
    assert c.long_bisection == (F <= c.n_faces)                              # no grid is over the budget iff the distinct sets fit it
    R = M.np_bisect(c.verts, c.tris, c.n_faces)
    M.check_invariant(c, R)
    clean = M.np_simplified(c, R)
    print(f"{name}: {len(c.tris)} faces, budget {c.n_faces}: R = {R}, {len(clean[1])} faces, dims {clean[4]}, "
          f"means' worst ratio to the bound {M.check_simplified(c, R, *clean):.3f}")
    if c.long_bisection:
        assert len(clean[1]) == F and len(clean[0]) == len(c.verts)          # the deduplicated mesh, every vertex a cluster of its own
        assert not caught(M.check_invariant, c, R) and caught(M.check_invariant, c, R // 2)
    else:
        assert caught(M.check_invariant, c, R - 1) and caught(M.check_invariant, c, R + 1)
    for fault in M.FACE_FAULTS:
        assert caught(M.check_simplified, c, R, *M.np_simplified(c, R, fault)), fault


# ------------------------------------------------------------------ corner0
def test_corner0_ties_by_hand():
    v, t, names = M.tie_faces()
    assert np.abs(v).max() < 2 ** 24 and (v == np.round(v)).all()
    d32, d64 = M.np_edge2(v, t), M.np_edge2(v, t, np.float64)
    assert np.array_equal(d32, d64) and d64.max() < 2 ** 24                  # small integers: exact however the sums are formed
    got = M.np_corner0(v, t)
    for name, r in zip(names, got):
        assert M.TIE_WANT[name.split("[")[0]] == r, name
    tie = (np.sort(d64, 1)[:, 2] == np.sort(d64, 1)[:, 1])
    assert tie.sum() >= 3 * 11 and (~tie).sum() >= 3 * 3
    M.check_corner0_ties(got)
    for fault in M.CORNER_FAULTS:
        assert caught(M.check_corner0_ties, M.np_corner0(v, t, fault)), fault
    assert (M.np_corner0(v, t, "last_max") != got)[tie].all() and not (M.np_corner0(v, t, "last_max") != got)[~tie].any()


def test_corner0_generic_faces():
    v, t = M.generic_faces()
    assert len(t) == 2000 and (np.abs(v[t[1500:]]).min() > 999) and np.abs(v[t[:1500]]).max() <= 1
    _, band = M.corner0_band(v, t)
    assert band.mean() <= 0.01                                               # the restatement alone, with this seed
    share = M.check_corner0_generic(v, t, M.np_corner0(v, t))
    print(f"corner0 on 2000 random faces: {share:.4f} of them inside the band of {M.EDGE_BOUND:.3e}")
    for fault in M.CORNER_FAULTS:
        assert caught(M.check_corner0_generic, v, t, M.np_corner0(v, t, fault)) == (fault == "plus_one"), fault      # no ties here


# ------------------------------------------------------------------ texel positions
def test_atlas_3_19_by_hand():
    """F = 3, T = 19: n = 2 cells per row of c = 9 texels, L = 4: 10 texels per chart; column and row 18 belong to no cell"""
    v, t = M.texel_mesh(3, False)
    fid, pos = M.np_texels(v, t, [0, 1, 2], 19)
    fid = fid.reshape(19, 19)
    assert M.atlas_nc(3, 19) == (2, 9)
    assert np.bincount(fid[fid >= 0]).tolist() == [10, 10, 10] and (fid >= 0).sum() == 30
    assert (fid[18] == -1).all() and (fid[:, 18] == -1).all() and (fid[9:] == -1).all()
    assert sorted(zip(*np.nonzero(fid == 0))) == [(y, x) for y in range(1, 5) for x in range(1, 6 - y)]
    assert sorted(zip(*np.nonzero(fid == 1))) == [(y, x) for y in range(4, 8) for x in range(11 - y, 8)]
    assert sorted(zip(*np.nonzero(fid == 2))) == [(y, 9 + x) for y in range(1, 5) for x in range(1, 6 - y)]
    p = v.astype(np.float64)[t]
    # texel (1, 1) of face 0 with corner0 = 0: b1 = b2 = 1/8; texel (x, y) = (7, 4) of face 1: (u, v) = (1, 4), corner0 = 1
    assert np.allclose(pos[19 + 1], 0.75 * p[0, 0] + 0.125 * p[0, 1] + 0.125 * p[0, 2], rtol=0, atol=1e-15)
    assert np.allclose(pos[4 * 19 + 7], 0.0 * p[1, 1] + 0.125 * p[1, 2] + 0.875 * p[1, 0], rtol=0, atol=1e-15)
    assert (pos[fid.reshape(-1) < 0] == 0).all()


@pytest.mark.parametrize("F,T", M.ATLAS_LAYOUTS)
def test_texel_cases(F, T):
    n, c = M.atlas_nc(F, T)
    L = c - 5
    face = rasterise(F, T)[0]
    assert c >= 8 and np.bincount(face[face >= 0], minlength=F).tolist() == [L * (L + 1) // 2] * F
    if (F, T) == (1, 8):
        assert (c, L) == (8, 3)
    for far in (False, True):
        v, t = M.texel_mesh(F, far)
        r = M.np_corner0(v, t)
        assert set(np.unique(r)) <= {0, 1, 2} and (F < 30 or len(np.unique(r)) == 3)
        fid, pos = M.np_texels(v, t, r, T, dtype=np.float32)
        assert np.array_equal(fid.reshape(T, T), face)                       # the formula and the edge functions agree
        ratio = M.check_texels(v, t, r, T, fid.astype(np.int32), pos)
        print(f"F={F} T={T} n={n} c={c} {'far' if far else 'near'}: float32 model, worst ratio to the position bound {ratio:.3f}")
        if far:
            continue                                                         # (the bound is 8 u 1000 there: half a texel of a 0.01 face)
        for fault in M.TEXEL_FAULTS:
            shows = {"k_past_F": 2 * n * n > F, "uv_swapped_upper": F >= 2}.get(fault, True)
            g = M.np_texels(v, t, r, T, fault, np.float32)
            assert caught(M.check_texels, v, t, r, T, g[0].astype(np.int32), g[1]) == shows, fault


def test_uvs_by_hand():
    from sin3dm_amd.encoding.isosurface import triangle_atlas
    uv = M.np_uvs([0, 1, 2], 3, 19).reshape(3, 3, 2) * 19
    assert np.allclose(uv[0], [[1, 1], [5, 1], [1, 5]]) and np.allclose(uv[1], [[8, 4], [8, 8], [4, 8]]) and np.allclose(uv[2], [[14, 1], [10, 5], [10, 1]])
    for F, T in M.ATLAS_LAYOUTS:
        r = np.arange(F) % 3
        assert np.array_equal(triangle_atlas(F, T).uvs(r), M.np_uvs(r, F, T))


# ------------------------------------------------------------------ quantise
def test_quantize_by_hand():
    tab = M.quant_table()
    assert len(tab) == 3 * 256 + 8 and np.isnan(tab[-1]) and np.isnan(tab).sum() == 1
    q = M.np_quantize(tab[:, None], np.arange(len(tab)), 32)[:len(tab), 0].astype(int)
    # fp32(k / 255) * 255 rounds back to k for these three; one ulp below k / 255 the product is below k: truncation gives k - 1
    assert q[[127, 128, 255]].tolist() == [127, 128, 255]
    assert q[[256 + 127, 256 + 128, 256 + 255]].tolist() == [126, 127, 254] and q[[512 + 127, 512 + 128, 512 + 255]].tolist() == [127, 128, 255]
    assert q[-8:].tolist() == [0, 0, 255, 255, 255, 255, 0, 0]               # -0, -1e-3, 1, 1 + ulp, 2, inf, -inf, NaN
    r = M.np_quantize(tab[:, None], np.arange(len(tab)), 32, "round")[:len(tab), 0].astype(int)
    assert r[256 + 127] == 127 and M.np_quantize(tab[:, None], np.arange(len(tab)), 32, "clamp_after_cast")[len(tab) - 4, 0] == 254


@pytest.mark.parametrize("C", [1, 3, 8])
def test_quantize_cases(C):
    cols, idx = M.quant_case(C)
    T = M.QUANT_T
    tab = M.quant_table()
    for ch in range(C):                                                      # every channel sees every value of the table
        assert np.array_equal(np.sort(cols[:-4, ch].view(np.uint32)), np.sort(tab.view(np.uint32)))
    inside = (idx >= 0) & (idx < T * T)
    assert (~inside).sum() == 4 and len(np.unique(idx)) == len(idx) < T * T and not np.array_equal(idx, np.sort(idx))
    clean = M.np_quantize(cols, idx, T)
    M.check_quantize(cols, idx, T, clean)
    for fault in M.QUANT_FAULTS:
        assert caught(M.check_quantize, cols, idx, T, M.np_quantize(cols, idx, T, fault)), fault
    stray = clean.copy()
    stray[np.flatnonzero(~np.isin(np.arange(T * T), idx))[0], 0] = 255       # a write through a wrapped index
    assert caught(M.check_quantize, cols, idx, T, stray)


# ------------------------------------------------------------------ dilation
def test_dilate_by_hand():
    q = np.zeros((3, 3, 1), np.uint8)
    q[0, 0], q[1, 1], q[2, 1] = 7, 9, 200
    cov = np.zeros((3, 3), bool)
    cov[1, 1] = True
    assert M.np_dilate(q, cov)[:, :, 0].tolist() == [[9, 9, 9], [200, 9, 200], [200, 200, 200]]
    assert M.np_dilate(q, cov, "four_neighbours")[:, :, 0].tolist() == [[7, 9, 0], [9, 9, 9], [200, 200, 200]]
    assert M.np_dilate(q, cov, "covered_too")[1, 1, 0] == 200
    assert M.np_dilate(q, cov, "cascade")[0].reshape(-1).tolist() == [M.PREFILL] * 3


@pytest.mark.parametrize("C", [1, 3, 8])
def test_dilate_cases(C):
    q, cov = M.dilate_case(C)
    T = M.DILATE_T
    assert q.shape == (T, T, C) and 0.25 < cov.mean() < 0.45 and not (q == M.PREFILL).any()
    assert cov[0, 0] and cov[0, -1] and cov[-1, 0] and cov[-1, -1]
    for edge in (cov[0], cov[-1], cov[:, 0], cov[:, -1]):
        assert "11111" in "".join("1" if b else "0" for b in edge) and not edge.all()
    zero = cov & (q == 0).all(2)
    pad = np.zeros((T + 2, T + 2), bool)
    pad[1:-1, 1:-1] = ~cov & (q == 255).all(2)
    beside = np.max([pad[1 + dy:T + 1 + dy, 1 + dx:T + 1 + dx] for dy in (-1, 0, 1) for dx in (-1, 0, 1)], 0)
    assert (zero & beside).sum() >= 20                                       # covered zeros with an uncovered 255 beside them
    clean = M.np_dilate(q, cov)
    M.check_dilate(q, cov, clean)
    for fault in M.DILATE_FAULTS:
        assert caught(M.check_dilate, q, cov, M.np_dilate(q, cov, fault)), fault
    # Not a fault: neighbours outside the image taking part as 0.  The maximum of unsigned values never picks a 0 over the texel's
    # own value, so "do not take part" and "take part as 0" are the same function; the check cannot and need not tell them apart.
    assert np.array_equal(M.np_dilate(q, cov, "zero_border"), clean)
    M.check_dilate(q, cov, M.np_dilate(q, cov, "zero_border"))
