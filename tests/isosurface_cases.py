"""Inputs and float64 references for the hard iso-surface tests (tests/test_isosurface_hard_host.py on the CPU against the C
restatement and a NumPy float32 model of the kernel's formulas, tests/test_isosurface_hard_gpu.py against the device).  Nothing
here reads the generated case table: the cut edges follow from the marching-cubes definition alone, and their ORDER from what the
kernel promises — (edge axis, linear index of the edge's lower end in the padded grid) — so vertex n of a mesh IS edge n, also
where the vertex has no fractional part left to name its edge (an end value equal to the level, t rounded to 1).

Bounds (derived, not measured; u = 2^-24, the unit round-off of float32):
  position    the kernel computes t = fl(fl(iso - v0) / fl(v1 - v0)) and p = fl(x + t) with correctly rounded division and no fast
              math: |p - p64| <= u (|p64| + 4) per coordinate — the final rounding, and three roundings of t <= 1 with one to spare.
  attribute   both ends inside the grid: a64 = A[a] + mu (A[b] - A[a]), |a - a64| <= 16 u max(|A[a]|, |A[b]|) per channel (the
              roundings of t, the difference, the product and the sum: about 13 units, rounded up).
              one end in the virtual border: the inside end's attribute BIT FOR BIT (pa == pb gives pa + t * 0)."""
from collections import namedtuple

import numpy as np

U = 2.0 ** -24
ATTR_SCALE = (1.0, 1e3, 1e-3)            # a swapped end, a wrong channel or a wrong stride shows at full size

Cut = namedtuple("Cut", "keys pos mu a b a_in b_in axis")
Case = namedtuple("Case", "name grid iso pad n_attr small")


# ------------------------------------------------------------------ the float64 definition
def _f32(x):
    return float(np.float32(x))


def expected_cut_edges(grid, iso=0.0, pad_value=1.0):
    """The cut edges of the value channel of `grid` ([X,Y,Z] or [X,Y,Z,S]) in the kernel's vertex order.  Works from the float32
    grid values promoted to float64, with `iso` and `pad_value` rounded to float32 first (the kernel receives floats).
    Cut(keys [n,4] int64 (axis, i, j, k) with i, j, k in the PADDED grid, pos [n,3] float64 in the index frame of the unpadded grid,
    mu [n] float64, a / b [n,3] the unpadded indices of the lower / upper end, a_in / b_in whether that end lies inside the grid,
    axis [n])."""
    g = np.asarray(grid, np.float32)
    val = (g[..., 0] if g.ndim == 4 else g).astype(np.float64)
    iso = _f32(iso)
    off = 0
    if pad_value is not None:
        val = np.pad(val, 1, mode="constant", constant_values=_f32(pad_value))
        off = 1
    shape = np.asarray(g.shape[:3])
    keys, pos, mus = [], [], []
    for axis in range(3):
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[axis], hi[axis] = slice(0, -1), slice(1, None)
        v0, v1 = val[tuple(lo)], val[tuple(hi)]
        idx = np.argwhere((v0 < iso) != (v1 < iso))                    # C order = ascending linear index of the lower end
        a0, a1 = v0[tuple(idx.T)], v1[tuple(idx.T)]
        mu = (iso - a0) / (a1 - a0)
        p = idx.astype(np.float64) - off
        p[:, axis] += mu
        keys.append(np.concatenate([np.full((len(idx), 1), axis, np.int64), idx.astype(np.int64)], 1))
        pos.append(p)
        mus.append(mu)
    keys, pos, mu = np.concatenate(keys), np.concatenate(pos), np.concatenate(mus)
    axis = keys[:, 0]
    a = keys[:, 1:] - off
    b = a.copy()
    b[np.arange(len(b)), axis] += 1
    a_in = ((a >= 0) & (a < shape)).all(1)
    b_in = ((b >= 0) & (b < shape)).all(1)
    return Cut(keys, pos, mu, a, b, a_in, b_in, axis)


def key_list(cut):
    """the keys as mc_independent.check_mesh(keys=...) takes them"""
    return [tuple(int(x) for x in k) for k in cut.keys]


def position_bound(cut):
    return U * (np.abs(cut.pos) + 4.0)


def check_positions(cut, verts):
    """vertex n against edge n; returns the worst error over its bound"""
    verts = np.asarray(verts)
    assert verts.dtype == np.float32 and verts.shape == cut.pos.shape, (verts.dtype, verts.shape, cut.pos.shape)
    if not len(verts):
        return 0.0
    ratio = np.abs(verts.astype(np.float64) - cut.pos) / position_bound(cut)
    n = int(np.argmax(ratio.max(1)))
    assert ratio.max() <= 1.0, (f"vertex {n} on edge {cut.keys[n].tolist()}: {verts[n].tolist()} against {cut.pos[n].tolist()}, "
                                f"{ratio.max():.3f} of the bound")
    return float(ratio.max())


def _ends(grid, cut, n_attr):
    """float32 attributes of both ends [n, n_attr] (an end in the border reads the other end's, as the kernel does)"""
    g = np.asarray(grid, np.float32)
    ia = np.where(cut.a_in[:, None], cut.a, cut.b)
    ib = np.where(cut.b_in[:, None], cut.b, cut.a)
    return g[ia[:, 0], ia[:, 1], ia[:, 2], 1:1 + n_attr], g[ib[:, 0], ib[:, 1], ib[:, 2], 1:1 + n_attr]


def check_attributes(grid, cut, attrs, n_attr):
    """interior edges within the bound of the float64 interpolation, border edges equal to the inside end in bits; returns the
    worst interior error over its bound"""
    attrs = np.asarray(attrs)
    assert attrs.dtype == np.float32 and attrs.shape == (len(cut.mu), n_attr), (attrs.dtype, attrs.shape)
    assert cut.a_in.any() and (cut.a_in | cut.b_in).all()               # an edge has at most one end in the border
    Aa, Ab = _ends(grid, cut, n_attr)
    border = ~(cut.a_in & cut.b_in)
    got, want = attrs[border].view(np.uint32), Aa[border].view(np.uint32)
    bad = np.flatnonzero((got != want).any(1))
    assert len(bad) == 0, (f"{len(bad)} border vertices do not carry the inside end's attributes bit for bit, the first: vertex "
                           f"{np.flatnonzero(border)[bad[0]]}: {attrs[border][bad[0]].tolist()} against {Aa[border][bad[0]].tolist()}")
    inner = ~border
    if not inner.any():
        return 0.0
    a64, b64 = Aa[inner].astype(np.float64), Ab[inner].astype(np.float64)
    ref = a64 + cut.mu[inner, None] * (b64 - a64)
    bound = 16.0 * U * np.maximum(np.abs(a64), np.abs(b64))
    err = np.abs(attrs[inner].astype(np.float64) - ref)
    ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
    n = int(np.argmax(ratio.max(1)))
    assert ratio.max() <= 1.0, (f"vertex {np.flatnonzero(inner)[n]} on edge {cut.keys[inner][n].tolist()}: attributes "
                                f"{attrs[inner][n].tolist()} against {ref[n].tolist()}, {ratio.max():.3f} of the bound")
    return float(ratio.max())


# ------------------------------------------------------------------ the kernel's formulas in NumPy float32 (host tests only)
def model_vertices(grid, cut, iso=0.0, pad_value=1.0, n_attr=0, iso_double=False):
    """(verts float32 [n,3], attrs float32 [n,n_attr] or None): t = fl(fl(iso - v0) / fl(v1 - v0)), p = fl(x + t),
    a = fl(pa + fl(t * fl(pb - pa))), every operation rounded to float32.  iso_double: the fault of using the level as a double
    (t computed in float64 from the unrounded level, then rounded once)."""
    g = np.asarray(grid, np.float32)
    val = g[..., 0] if g.ndim == 4 else g
    off = 0
    if pad_value is not None:
        val = np.pad(val, 1, mode="constant", constant_values=np.float32(pad_value))
        off = 1
    k = cut.keys
    lo = k[:, 1:]
    hi = lo.copy()
    hi[np.arange(len(hi)), cut.axis] += 1
    v0, v1 = val[lo[:, 0], lo[:, 1], lo[:, 2]], val[hi[:, 0], hi[:, 1], hi[:, 2]]
    if iso_double:
        t = ((float(iso) - v0.astype(np.float64)) / (v1.astype(np.float64) - v0.astype(np.float64))).astype(np.float32)
    else:
        t = ((np.float32(iso) - v0) / (v1 - v0)).astype(np.float32)
    verts = (lo - off).astype(np.float32)
    verts[np.arange(len(verts)), cut.axis] += t
    attrs = None
    if n_attr:
        Aa, Ab = _ends(g, cut, n_attr)
        attrs = (Aa + t[:, None] * (Ab - Aa)).astype(np.float32)
    return verts, attrs


# ------------------------------------------------------------------ the cases
def _with_attrs(val, channels, seed):
    """[X,Y,Z,1+channels]: per-voxel random attributes, the channels scaled 1, 1e3, 1e-3, 1, ..."""
    rng = np.random.Generator(np.random.PCG64(seed))
    a = rng.uniform(-1.0, 1.0, val.shape + (channels,)) * np.asarray([ATTR_SCALE[c % 3] for c in range(channels)])
    return np.concatenate([val[..., None], a], -1).astype(np.float32)


def _sphere12(radius):
    ax = np.linspace(-1, 1, 12)
    x, y, z = np.meshgrid(ax, ax * 0.9, ax * 1.1, indexing="ij")
    return (np.sqrt(x * x + y * y + z * z) - radius).astype(np.float32)


def _noise(shape, seed):
    return np.random.Generator(np.random.PCG64(seed)).standard_normal(shape).astype(np.float32)


def ties_half_grid():
    """114 of the 504 values equal the level 0.  (Seed 102 is avoided: without the border the C restatement's mesh of it has 21 of
    979 triangles on the wrong side of check_mesh's orientation heuristic, whose cap is 2 % — the heuristic takes the gradient at
    the centroid of a quantised field; it and its cap stay as they are.)"""
    return (np.round(2.0 * _noise((9, 8, 7), 109)) / 2.0).astype(np.float32)


def ties_one_grid():
    return np.round(_noise((8, 9, 6), 103)).astype(np.float32)


def t_to_one_grid():
    g = np.ones((6, 6, 6), np.float32)
    g[2:4, 2:4, 2:4] = np.float32(-1e-9)
    return g


def long_grid():
    return _noise((300, 5, 4), 108)


_cases = None


def cases():
    """every case once; `small`: few enough cells for mc_independent.check_mesh (python loops over cells)"""
    global _cases
    if _cases is not None:
        return _cases
    sphere = _with_attrs(_sphere12(1.15), 3, 100)
    pbr = _with_attrs(_noise((9, 8, 7), 101), 8, 111)
    half = _with_attrs(ties_half_grid(), 1, 112)
    thin = _noise((1, 9, 8), 105)
    out = [
        Case("border_sphere_pad", sphere, 0.0, 1.0, 3, False),
        Case("border_sphere_open", sphere, 0.0, None, 3, False),
        Case("pbr_stride_3", pbr, 0.0, 1.0, 3, True),
        Case("pbr_stride_8", pbr, 0.0, 1.0, 8, True),
        Case("ties_half_pad", half, 0.0, 1.0, 1, True),
        Case("ties_half_open", half, 0.0, None, 1, True),
        Case("ties_one", ties_one_grid(), 0.0, 1.0, 0, True),
        Case("t_to_one", t_to_one_grid(), 0.0, 1.0, 0, True),
        Case("level_noise", _noise((7, 9, 6), 104), -0.7, 2.5, 0, True),
        Case("level_sphere", _sphere12(0.7), 0.3, 1.0, 0, False),
        Case("thin_pad", thin, 0.0, 1.0, 0, True),
        Case("thin_open", thin, 0.0, None, 0, True),
        Case("two_cubed", _noise((2, 2, 2), 106), 0.0, 1.0, 0, True),
        Case("one_voxel", np.full((1, 1, 1), -1.0, np.float32), 0.0, 1.0, 0, True),
        Case("full", np.full((5, 4, 3), -1.0, np.float32), 0.0, 1.0, 0, True),
        Case("long", long_grid(), 0.0, 1.0, 0, False),
    ]
    for c in out:
        c.grid.setflags(write=False)
    _cases = out
    return out


def case(name):
    return next(c for c in cases() if c.name == name)


_cuts = {}


def cut_of(c):
    """the float64 reference of a case, computed once and left unchanged"""
    if c.name not in _cuts:
        cut = expected_cut_edges(c.grid, c.iso, c.pad)
        for x in cut:
            x.setflags(write=False)
        _cuts[c.name] = cut
    return _cuts[c.name]


# ------------------------------------------------------------------ meshes for the component tests
def strip_permuted(n=5000, seed=120):
    """the 5000-triangle strip with its vertex indices randomly permuted: the minimum label no longer travels in index order"""
    strip = np.stack([np.arange(n), np.arange(n) + 1, np.arange(n) + 2], 1)
    perm = np.random.Generator(np.random.PCG64(seed)).permutation(n + 2)
    return perm[strip].astype(np.int32), n + 2
