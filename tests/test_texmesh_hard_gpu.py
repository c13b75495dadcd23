"""GPU: the seven kernels of s3d_tex.hip and simplify_mesh's bookkeeping on the inputs the first draft (tests/test_texmesh_gpu.py)
does not have: vertices on cell faces and one ulp beside them, an inexact cell side, a flat sheet, a box far from the origin; a
50 000-member cluster; duplicated, cyclic and reversed faces and the bisection that finds no grid over the budget; exact ties of
the longest edge; odd face counts, the smallest cell and empty chart slots in the atlas; colours at every k / 255, outside [0, 1]
and NaN; a dilation mask on the image border (tests/texmesh_cases.py builds the inputs, the NumPy restatements and the checks;
tests/test_texmesh_hard_host.py shows that each check reports the faults it is there for).

Keys, face ids, corner0 on ties, faces, quantised and dilated images are compared with array_equal.  Means and positions are held
to the two derived bounds of texmesh_cases.py; the worst ratios are printed (profiles/texmesh_hard.txt).  Every device call is
made twice and must give the same bits."""
import time

import numpy as np
import pytest
import torch

import texmesh_cases as M

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def twice(fn):
    """fn() -> tuple of tensors; run two times, same bits"""
    a, b = fn(), fn()
    assert len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))
    return a


# ------------------------------------------------------------------ k_cluster_keys
@pytest.mark.parametrize("name", M.KEY_CASES)
def test_cluster_keys_exact(name):
    from sin3dm_amd.encoding.isosurface import _cluster_keys, cluster_grid
    c = M.key_case(name)
    s, dims = cluster_grid(c.extent, c.R)
    assert np.float32(s) == c.s and dims == c.dims and len(set(dims)) == 3
    v = dev(c.verts)
    keys, = twice(lambda: (_cluster_keys(v, c.origin, s, dims),))
    M.check_keys(c, keys.cpu().numpy())
    print(f"{name}: {len(c.verts)} vertices, s = {float(s):.9g}, dims {dims}: keys equal the float32 restatement")


# ------------------------------------------------------------------ k_cluster_means
@pytest.mark.parametrize("name,ch", M.MEAN_CASES)
def test_cluster_means_bound(name, ch):
    from sin3dm_amd.encoding.isosurface import _cluster_means
    c = M.mean_case(name, ch)
    vals, order, seg = dev(c.vals), dev(c.order), dev(c.seg)
    pos, attrs = vals[:, :3].contiguous(), vals[:, 3:].contiguous()          # two calls, as simplify_mesh makes them: C = 3 and C = ch
    got = twice(lambda: (_cluster_means(pos, order, seg, len(c.seg) - 1), _cluster_means(attrs, order, seg, len(c.seg) - 1)))
    assert got[1].shape[1] == ch
    ratio = M.check_means(c, torch.cat(got, 1).cpu().numpy())
    n = np.diff(c.seg)
    print(f"{c.name}: {len(n)} segments of {n.min()} to {n.max()} members, 3 + {ch} channels: worst |mean error| / bound = {ratio:.3f}")


# ------------------------------------------------------------------ k_remap_faces, the dedupe and the bisection: simplify_mesh
def _simplify(c, tris=None, n_faces=None):
    from sin3dm_amd.encoding.isosurface import simplify_mesh
    v, t, at = dev(c.verts), dev(c.tris) if tris is None else tris, dev(c.attrs)
    found = []

    def run():
        v2, t2, info = simplify_mesh(v, t, c.n_faces if n_faces is None else n_faces, attrs=at)
        found.append(info)
        return v2, t2, info["vmap"], info["keys"], info["attrs"]
    out = twice(run)
    assert found[0]["R"] == found[1]["R"] == found[0]["lo"] and found[0]["dims"] == found[1]["dims"]
    return out, found[0]


@pytest.mark.parametrize("name", M.FACE_CASES)
def test_simplify_repeated_faces(name):
    """Every face of the sheet two or three times (reversed; rotated and reversed): the first copy is kept in its own winding.
    In the *_long cases the distinct vertex sets fit the budget although the faces do not, so no grid is over the budget and the
    bisection's invariant count(R) <= n_faces < count(R + 1) cannot be met: hi doubles past 2^20 and R = 2^20, the finest grid
    the function uses, is returned with count(R) <= n_faces (simplify_mesh's docstring); here that is the deduplicated mesh
    with every vertex kept.  About 20 counts: a fraction of a second."""
    c = M.face_case(name)
    t0 = time.perf_counter()
    (v2, t2, vmap, keys, attrs), info = _simplify(c)
    dt = time.perf_counter() - t0
    R = info["R"]
    M.check_invariant(c, R)
    ratio = M.check_simplified(c, R, v2.cpu().numpy(), t2.cpu().numpy(), vmap.cpu().numpy(), keys.cpu().numpy(), info["dims"], info["s"],
                               attrs.cpu().numpy())
    if c.long_bisection:
        assert R == M.R_LIMIT and len(t2) == c.n_first and len(v2) == len(c.verts)
    print(f"{name}: {len(c.tris)} faces, budget {c.n_faces}: R = {R}, dims {info['dims']}, {len(t2)} faces; faces equal the restatement; "
          f"worst |mean error| / bound = {ratio:.3f}; two calls {dt:.2f} s")


def test_simplify_budget_zero():
    c = M.face_case("double_sided")
    (v2, t2, vmap, keys, attrs), info = _simplify(c, n_faces=0)
    assert v2.shape == (0, 3) and t2.shape == (0, 3) and attrs.shape == (0, 2) and t2.dtype == torch.int32 and v2.dtype == torch.float32
    assert info["R"] == 1 and M.np_count(c.verts, c.tris, 1) == 0 < M.np_count(c.verts, c.tris, 2)
    assert (vmap == 0).all() and (keys == 0).all()


def test_simplify_index_types():
    """int64 faces and a non-contiguous view give the bits of contiguous int32"""
    c = M.face_case("repeats")
    want, info = _simplify(c)
    wide = torch.zeros((len(c.tris), 6), dtype=torch.int32, device="cuda")
    wide[:, ::2] = dev(c.tris)
    view = wide[:, ::2]
    assert not view.is_contiguous()
    vt = dev(np.concatenate([c.verts, c.verts], 1))[:, :3]
    assert not vt.is_contiguous()
    from sin3dm_amd.encoding.isosurface import simplify_mesh
    for t, v in ((dev(c.tris).long(), dev(c.verts)), (view, dev(c.verts)), (view.long(), vt)):
        v2, t2, info2 = simplify_mesh(v, t, c.n_faces, attrs=dev(c.attrs))
        assert t2.dtype == torch.int32 and info2["R"] == info["R"]
        assert all(torch.equal(a, b) for a, b in zip(want, (v2, t2, info2["vmap"], info2["keys"], info2["attrs"])))


@pytest.mark.parametrize("bad", [float("inf"), float("-inf"), float("nan")])
def test_simplify_non_finite_vertex(bad):
    from sin3dm_amd.encoding.isosurface import simplify_mesh
    c = M.face_case("double_sided")
    v = c.verts.copy()
    v[57, 1] = bad
    with pytest.raises(ValueError):
        simplify_mesh(dev(v), dev(c.tris), c.n_faces)


# ------------------------------------------------------------------ k_face_corner0
def test_corner0_exact_ties():
    from sin3dm_amd.encoding.isosurface import atlas_texels
    v, t, names = M.tie_faces()
    vd, td = dev(v), dev(t)
    corner0 = twice(lambda: atlas_texels(vd, td, 64)[:3])[2]
    M.check_corner0_ties(corner0.cpu().numpy())
    print(f"corner0 on {len(t)} faces with integer coordinates ({len(names) // 3} shapes at three offsets): the first-maximum rule exactly")


def test_corner0_generic_faces():
    from sin3dm_amd.encoding.isosurface import atlas_texels
    v, t = M.generic_faces()
    vd, td = dev(v), dev(t)
    corner0 = twice(lambda: atlas_texels(vd, td, 256)[:3])[2]
    share = M.check_corner0_generic(v, t, corner0.cpu().numpy())
    print(f"corner0 on {len(t)} random faces: chosen edge within {M.EDGE_BOUND:.3e} of the longest; {share:.4f} of the faces in the band, "
          f"the others equal the float64 choice")


# ------------------------------------------------------------------ k_texel_positions
@pytest.mark.parametrize("far", [False, True], ids=["near", "far"])
@pytest.mark.parametrize("F,T", M.ATLAS_LAYOUTS)
def test_texel_positions(F, T, far):
    from sin3dm_amd.encoding.isosurface import atlas_texels, bake_texture
    v, t = M.texel_mesh(F, far)
    vd, td = dev(v), dev(t)
    fid, pos, corner0 = twice(lambda: atlas_texels(vd, td, T)[:3])
    atlas = atlas_texels(vd, td, T)[3]
    assert (atlas.n, atlas.c) == M.atlas_nc(F, T)
    r = corner0.cpu().numpy()
    assert r.shape == (F,) and r.min() >= 0 and r.max() <= 2
    ratio = M.check_texels(v, t, r, T, fid.cpu().numpy(), pos.cpu().numpy())
    print(f"F={F} T={T} n={atlas.n} c={atlas.c} {'far' if far else 'near'}: face ids equal rasterise; worst |position error| / bound = {ratio:.3f}")
    image, mask, gb_pos, uvs, corner0b = twice(lambda: bake_texture(vd, td, T, lambda p: 0.25 + 0.0 * p[:, :2]))
    assert torch.equal(corner0b, corner0) and torch.equal(gb_pos.reshape(-1, 3), pos) and torch.equal(mask.reshape(-1), fid >= 0)
    assert image.shape == (T, T, 2)
    assert np.array_equal(uvs.cpu().numpy(), M.np_uvs(r, F, T))               # every face, every vertex


# ------------------------------------------------------------------ k_tex_quantize
@pytest.mark.parametrize("ch", [1, 3, 8])
def test_quantize_table(ch):
    """every k / 255 with its float32 neighbours, values outside [0, 1], infinities and NaN (-> 0: fmaxf returns the other operand),
    scattered through a shuffled index with four entries outside the image, into a buffer that is not zero beforehand"""
    from sin3dm_amd import _lib
    cols, idx = M.quant_case(ch)
    T = M.QUANT_T
    cd, idd = dev(cols), dev(idx)

    def run():
        img = torch.full((T * T, ch), M.PREFILL, dtype=torch.uint8, device="cuda")
        _lib.check(_lib.load().s3d_tex_quantize(_lib.ptr(cd), _lib.ptr(idd), len(idx), ch, T, _lib.ptr(img), _lib.stream_ptr()))
        torch.cuda.synchronize()
        return (img,)
    img, = twice(run)
    M.check_quantize(cols, idx, T, img.cpu().numpy())
    print(f"quantise C={ch}: {len(idx)} colours ({len(M.quant_table())} table values per channel): equal to the float32 statement, NaN -> 0")


@pytest.mark.parametrize("ch", [1, 3, 8])
def test_quantize_and_dilate_through_bake_texture(ch):
    """the same table as the decoder's answer: covered texels are its float32 statement, the others the dilation of that"""
    from sin3dm_amd.encoding.isosurface import bake_texture
    T, F = 64, 8
    v, t = M.texel_mesh(F, False)
    vd, td = dev(v), dev(t)
    tab = M.quant_table()
    g = M.rng(50 + ch)
    seen = []

    def decode(p):
        cols = np.stack([np.resize(tab[g.permutation(len(tab))], p.shape[0]) for _ in range(ch)], 1)
        seen.append(cols)
        return dev(cols)
    image, mask, _, _, _ = bake_texture(vd, td, T, decode)
    m = mask.cpu().numpy()
    assert len(seen) == 1 and seen[0].shape[0] == m.sum() >= len(tab)
    q = M.np_quantize(seen[0], np.flatnonzero(m.reshape(-1)), T).reshape(T, T, ch)
    img = image.cpu().numpy()
    assert np.array_equal(img[m], q[m])
    assert np.array_equal(img, M.np_dilate(q, m))


# ------------------------------------------------------------------ k_tex_dilate
@pytest.mark.parametrize("ch", [1, 3, 8])
def test_dilate_mask_on_the_border(ch):
    from sin3dm_amd import _lib
    q, cov = M.dilate_case(ch)
    T = M.DILATE_T
    ids = np.where(cov, M.rng(60).integers(0, 1 << 30, cov.shape), -1).astype(np.int32)
    ids[0, 0] = 0
    qd, fd = dev(q), dev(ids)

    def run():
        out = torch.full((T, T, ch), M.PREFILL, dtype=torch.uint8, device="cuda")
        _lib.check(_lib.load().s3d_tex_dilate(_lib.ptr(qd), _lib.ptr(fd), T, ch, _lib.ptr(out), _lib.stream_ptr()))
        torch.cuda.synchronize()
        return (out,)
    out, = twice(run)
    M.check_dilate(q, cov, out.cpu().numpy())
    print(f"dilate C={ch}: T={T}, {cov.mean():.2f} covered: equal to the padded 3 x 3 maximum")
