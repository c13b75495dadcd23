"""Fields, a NumPy restatement of the narrow-band rule and the checkers of its two guarantees, for
tests/test_sparse_mc_host.py (CPU: the restatement against the dense definition, and the proof that each checker can fail) and
tests/test_sparse_mc_gpu.py (the device against the same checkers).

The rule, in the padded vertex space of the dense path (P = dims + 2, vertex p holds sample p - 1 or pad_value): brick b holds the
vertices [b B, b B + B) per axis; the field on the brick-corner lattice (index coordinates b B - 1.5, pad_value outside
[-0.5, dims - 0.5]) makes a brick a seed iff its eight corners do not compare the same way against iso; a cell is extracted iff
the bricks of all eight of its corners are active; while a cut edge has an extracted and a non-extracted cell around it, the
bricks of those cells' corners are activated.  The result is the dense mesh without the triangles of the cells not extracted.

Every field here is a stored grid; the lattice reads it by `value(c) = grid[clip(floor(c), 0, dims - 1)]`, the same expression for
the integer coordinates of the samples and the x.5 of the lattice, so the host restatement and the device see the same numbers.
A triangle's cell comes from the case index of the cells (the counts of s3d_mc_tables.h) and is then checked against the table-free
edge keys of isosurface_cases.py: every vertex of a triangle must lie on an edge of that cell."""
import os
import re
from collections import namedtuple

import numpy as np

import isosurface_cases as IC
from conftest import REPO

SCase = namedtuple("SCase", "name grid iso pad n_attr blocks")
Dense = namedtuple("Dense", "verts tris attrs keys tri_cell labels")
Rule = namedtuple("Rule", "B nb seed active ext0 ext rounds closed n_samples P corner")


# ------------------------------------------------------------------ fields
def _coords(dims):
    return np.meshgrid(*[np.arange(d, dtype=np.float64) for d in dims], indexing="ij")


def torus(dims, R=0.30, r=0.12):
    """exact distance to a torus around the z axis through the grid's centre, radii as fractions of the smallest of dims[:2]"""
    x, y, z = _coords(dims)
    s = min(dims[0], dims[1])
    cx, cy, cz = [(d - 1) / 2.0 for d in dims]
    q = np.sqrt((x - cx) ** 2 + (y - cy) ** 2) - R * s
    return (np.sqrt(q * q + (z - cz) ** 2) - r * s).astype(np.float32)


def border_sphere(dims):
    """a sphere around a point near the (0, 0, .) edge of the box: two faces of the box cut it"""
    x, y, z = _coords(dims)
    return (np.sqrt((x - 2.0) ** 2 + (y - 3.0) ** 2 + (z - dims[2] / 2.0) ** 2) - 0.4 * min(dims)).astype(np.float32)


def fourier(dims, seed=7, waves=6):
    rng = np.random.Generator(np.random.PCG64(seed))
    x, y, z = _coords(dims)
    f = np.zeros(dims)
    for _ in range(waves):
        k = rng.uniform(-0.45, 0.45, 3)
        f += rng.uniform(0.5, 1.0) * np.sin(k[0] * x + k[1] * y + k[2] * z + rng.uniform(0, 2 * np.pi))
    return f.astype(np.float32)


POLE = (slice(31, 32), slice(18, 19), slice(14, 26))         # a one-voxel column standing on the torus' tube
SPECK = (4, 4, 4)                                            # one voxel far from the torus and from every lattice point


def torus_pole_speck(dims=(40, 36, 28)):
    g = torus(dims).copy()
    g[POLE] = np.float32(-0.5)
    g[SPECK] = np.float32(-0.5)
    return g


# no lattice point sees anything: the empty field, and a grid of 5 samples against bricks of 8 — its lattice planes along x lie at
# -1.5 and 6.5, both outside [-0.5, 4.5], so every lattice point takes pad_value (the rule's blind spot)
NO_SEEDS = {("empty", 4), ("all_negative_thin", 8)}

_cases = None


def cases():
    global _cases
    if _cases is not None:
        return _cases
    out = [
        SCase("torus_40", torus((40, 36, 28)), 0.0, 1.0, 0, (4, 8)),
        SCase("torus_37_attrs", IC._with_attrs(torus((37, 33, 29)), 3, 130), 0.0, 1.0, 3, (8, 16)),
        SCase("border_sphere", border_sphere((21, 19, 18)), 0.0, 1.0, 0, (4, 8)),
        SCase("all_negative", np.full((21, 19, 18), -1.0, np.float32), 0.0, 1.0, 0, (4,)),
        SCase("all_negative_thin", np.full((5, 40, 3), -1.0, np.float32), 0.0, 1.0, 0, (4, 8)),
        SCase("empty", np.full((21, 19, 18), 2.0, np.float32), 0.0, 1.0, 0, (4,)),
        SCase("fourier", fourier((37, 33, 29)), 0.1, 1.0, 0, (4, 8)),
        SCase("fourier_thin", fourier((5, 40, 3), seed=8), 0.0, 2.5, 0, (4,)),
        SCase("pole_speck", torus_pole_speck(), 0.0, 1.0, 0, (4, 8)),
        SCase("ties_half", IC.ties_half_grid(), 0.0, 1.0, 0, (4,)),
        SCase("t_to_one", IC.t_to_one_grid(), 0.0, 1.0, 0, (4,)),
    ]
    for c in out:
        c.grid.setflags(write=False)
    _cases = out
    return out


def case(name):
    return next(c for c in cases() if c.name == name)


def case_blocks():
    return [(c.name, B) for c in cases() for B in c.blocks]


def value_of(c):
    return c.grid[..., 0] if c.grid.ndim == 4 else c.grid


def lookup(grid, coords):
    """the field of a stored grid at index coordinates [M,3] (integers or x.5): grid[clip(floor(c), 0, dims - 1)]"""
    g = np.asarray(grid)
    idx = np.clip(np.floor(np.asarray(coords, np.float64)).astype(np.int64), 0, np.asarray(g.shape[:3]) - 1)
    return g[idx[:, 0], idx[:, 1], idx[:, 2]]


# ------------------------------------------------------------------ the dense mesh with the cell of every triangle
def ntri_table():
    with open(os.path.join(REPO, "sin3dm_amd", "csrc", "s3d_mc_tables.h")) as fh:
        body = re.search(r"MC_NTRI\[256\]\s*=\s*\{([^}]*)\}", fh.read()).group(1)
    t = np.asarray([int(x) for x in body.split(",") if x.strip()], np.int64)
    assert t.shape == (256,)
    return t


def cell_case_index(val, iso, pad_value):
    """[P-1]^3 case index of every cell of the padded grid: bit c = value < iso at corner (c & 1, (c >> 1) & 1, (c >> 2) & 1)"""
    pv = np.pad(np.asarray(val, np.float32), 1, mode="constant", constant_values=np.float32(pad_value))
    ins = pv < np.float32(iso)
    P = ins.shape
    cs = np.zeros((P[0] - 1, P[1] - 1, P[2] - 1), np.int64)
    for c in range(8):
        dx, dy, dz = c & 1, (c >> 1) & 1, (c >> 2) & 1
        cs |= ins[dx:P[0] - 1 + dx, dy:P[1] - 1 + dy, dz:P[2] - 1 + dz].astype(np.int64) << c
    return cs


def dense_mesh(c, verts, tris, attrs, components):
    """Dense(...) of a case from a dense mesh (the C restatement's or the device's): keys [nv,4] (axis, padded i, j, k) from the
    vertex order, tri_cell [nt,3] the padded cell of every triangle, labels [nv] (components(tris, nv))."""
    val = value_of(c)
    cut = IC.expected_cut_edges(val, c.iso, c.pad)
    assert len(cut.keys) == len(verts), (len(cut.keys), len(verts))
    nt = ntri_table()[cell_case_index(val, c.iso, c.pad)]
    cells = np.argwhere(nt > 0)                                                  # C order = ascending linear cell index
    tri_cell = np.repeat(cells, nt[nt > 0], axis=0)
    assert len(tri_cell) == len(tris), (len(tri_cell), len(tris))
    if len(tris):
        k = cut.keys[np.asarray(tris, np.int64)]                                 # [nt,3,4]: every corner on an edge of the triangle's cell
        d = k[:, :, 1:] - tri_cell[:, None, :]
        on_axis = np.arange(3)[None, None, :] == k[:, :, :1]
        assert (np.where(on_axis, d == 0, (d == 0) | (d == 1))).all()
    labels = components(np.asarray(tris, np.int32), len(verts)) if len(verts) else np.zeros(0, np.int32)
    return Dense(np.asarray(verts), np.asarray(tris), attrs, cut.keys, tri_cell, labels)


def select_cells(dense, ext):
    """(verts, tris, attrs) of the dense mesh restricted to the cells of the mask `ext`: the other triangles removed, the vertices
    nothing references dropped, the order kept"""
    keep_t = ext[tuple(dense.tri_cell.T)] if len(dense.tris) else np.zeros(0, bool)
    t = dense.tris[keep_t]
    used = np.zeros(len(dense.verts), bool)
    used[t.reshape(-1)] = True
    remap = np.cumsum(used) - 1
    return (dense.verts[used], remap[t].astype(np.int32).reshape(-1, 3), dense.attrs[used] if dense.attrs is not None else None)


def component_union(dense, cells):
    """the dense mesh restricted to the connected components that have a triangle in a cell of the mask `cells`"""
    if not len(dense.tris):
        return select_cells(dense, np.zeros_like(cells))
    face_label = dense.labels[dense.tris[:, 0]]
    touched = np.unique(face_label[cells[tuple(dense.tri_cell.T)]])
    keep_t = np.isin(face_label, touched)
    t = dense.tris[keep_t]
    used = np.zeros(len(dense.verts), bool)
    used[t.reshape(-1)] = True
    remap = np.cumsum(used) - 1
    return (dense.verts[used], remap[t].astype(np.int32).reshape(-1, 3), dense.attrs[used] if dense.attrs is not None else None)


# ------------------------------------------------------------------ the rule
def lattice_axes(dims, B):
    nb = [-(-(d + 2) // B) for d in dims]
    return [np.arange(n + 1, dtype=np.float64) * B - 1.5 for n in nb], nb


def _dilate26(a):
    p = np.pad(a, 1)
    out = np.zeros_like(a)
    for dx in range(3):
        for dy in range(3):
            for dz in range(3):
                out |= p[dx:dx + a.shape[0], dy:dy + a.shape[1], dz:dz + a.shape[2]]
    return out


def _vertex_active(active, P, B):
    ix = [np.arange(p) // B for p in P]
    return active[np.ix_(*ix)]


def _extracted(active, P, B):
    av = _vertex_active(active, P, B)
    ext = np.ones((P[0] - 1, P[1] - 1, P[2] - 1), bool)
    for c in range(8):
        dx, dy, dz = c & 1, (c >> 1) & 1, (c >> 2) & 1
        ext &= av[dx:P[0] - 1 + dx, dy:P[1] - 1 + dy, dz:P[2] - 1 + dz]
    return ext


def _boundary_edges(ins, ext):
    """per axis the mask of the cut edges (indexed by their lower end) that have an extracted and a non-extracted cell among the
    up-to-four cells around them"""
    out = []
    for axis in range(3):
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[axis], hi[axis] = slice(0, -1), slice(1, None)
        cut = ins[tuple(lo)] != ins[tuple(hi)]
        pad = [(1, 1)] * 3
        pad[axis] = (0, 0)
        E, N = np.pad(ext, pad), np.pad(~ext, pad)                               # cells that do not exist are neither
        any_e = np.zeros_like(cut)
        any_n = np.zeros_like(cut)
        o = [a for a in range(3) if a != axis]
        for d0 in (0, 1):
            for d1 in (0, 1):
                s = [slice(None)] * 3
                s[o[0]] = slice(1 - d0, 1 - d0 + cut.shape[o[0]])
                s[o[1]] = slice(1 - d1, 1 - d1 + cut.shape[o[1]])
                any_e |= E[tuple(s)]
                any_n |= N[tuple(s)]
        out.append(cut & any_e & any_n)
    return out


def _cells_around(bnd, ext):
    """the non-extracted cells that have one of the boundary edges `bnd` among their twelve"""
    m = np.zeros_like(ext)
    for axis in range(3):
        o = [a for a in range(3) if a != axis]
        for d0 in (0, 1):
            for d1 in (0, 1):
                s = [slice(None)] * 3
                s[o[0]] = slice(d0, d0 + ext.shape[o[0]])
                s[o[1]] = slice(d1, d1 + ext.shape[o[1]])
                m |= bnd[axis][tuple(s)]
    return m & ~ext


def rule(val, iso, pad_value, B, dilate=0, max_rounds=64, all_active=False, fault=None, lattice_fn=None):
    """The narrow-band rule on a stored grid.  fault: None, "no_growth" (the seeds are taken for the answer), "pad_unknown" (a cell
    with a corner in the pad shell is not extracted) or "lattice_unpadded" (lattice points outside the box read the field).
    lattice_fn(coords [M,3]) -> values [M]: the field on the lattice where it is not the grid's lookup (a decoder)."""
    val = np.asarray(val, np.float32)
    dims = val.shape
    P = tuple(d + 2 for d in dims)
    axes, nb = lattice_axes(dims, B)
    ins = np.pad(val, 1, mode="constant", constant_values=np.float32(pad_value)) < np.float32(iso)
    n_samples = 0
    if all_active:
        seed = np.ones(nb, bool)
        active = seed.copy()
        corner = np.zeros(nb, bool)
    else:
        co = np.stack(np.meshgrid(*axes, indexing="ij"), -1).reshape(-1, 3)
        clamped = np.clip(co, -0.5, np.asarray(dims) - 0.5)
        lat = np.asarray(lattice_fn(clamped) if lattice_fn is not None else lookup(val, clamped), np.float32)
        n_samples += len(co)
        if fault != "lattice_unpadded":
            outside = ((co < -0.5) | (co > np.asarray(dims) - 0.5)).any(1)
            lat = np.where(outside, np.float32(pad_value), lat)
        lin = (lat < np.float32(iso)).reshape([n + 1 for n in nb])
        n_in = np.zeros(nb, np.int64)
        for c in range(8):
            dx, dy, dz = c & 1, (c >> 1) & 1, (c >> 2) & 1
            n_in += lin[dx:nb[0] + dx, dy:nb[1] + dy, dz:nb[2] + dz]
        seed = (n_in != 0) & (n_in != 8)
        corner = lin[:-1, :-1, :-1].copy()                                       # value < iso at every brick's first corner
        active = seed.copy()
        for _ in range(dilate):
            active = _dilate26(active)

    def extracted(a):
        ext = _extracted(a, P, B)
        if fault == "pad_unknown":
            ext[0], ext[-1], ext[:, 0], ext[:, -1], ext[:, :, 0], ext[:, :, -1] = False, False, False, False, False, False
        return ext
    ext0 = extracted(active)
    ext, rounds, closed = ext0, 0, True
    if not all_active and fault != "no_growth":
        while True:
            bnd = _boundary_edges(ins, ext)
            closed = not any(b.any() for b in bnd)
            if closed or rounds >= max_rounds:
                break
            cells = np.argwhere(_cells_around(bnd, ext))
            for c in range(8):
                b = (cells + np.asarray([c & 1, (c >> 1) & 1, (c >> 2) & 1])) // B
                active[tuple(b.T)] = True
            ext = extracted(active)
            rounds += 1
    n_samples += int(active.sum()) * B ** 3
    return Rule(B, tuple(nb), seed, active, ext0, ext, rounds, closed, n_samples, P, corner)


def rule_occupancy(val, iso, r):
    """the occupancy the band gives: value < iso in active bricks, the first lattice corner's elsewhere"""
    val = np.asarray(val, np.float32)
    ix = [(np.arange(d) + 1) // r.B for d in val.shape]                          # sample s is padded vertex s + 1
    act, cor = r.active[np.ix_(*ix)], r.corner[np.ix_(*ix)]
    return np.where(act, val < np.float32(iso), cor)


# ------------------------------------------------------------------ the checkers
def same_mesh(got, want, what=""):
    """bit for bit: verts, tris, attrs and their order"""
    gv, gt, ga = got
    wv, wt, wa = want
    assert gv.shape == wv.shape and gt.shape == wt.shape, f"{what}: {gv.shape} / {gt.shape} against {wv.shape} / {wt.shape}"
    assert np.array_equal(np.asarray(gt, np.int64), np.asarray(wt, np.int64)), f"{what}: triangles differ"
    assert np.array_equal(np.asarray(gv, np.float32).view(np.uint32), np.asarray(wv, np.float32).view(np.uint32)), f"{what}: vertices differ"
    assert (ga is None) == (wa is None), what
    if ga is not None:
        assert np.array_equal(np.asarray(ga, np.float32).view(np.uint32), np.asarray(wa, np.float32).view(np.uint32)), f"{what}: attributes differ"


def check_all_active(dense, got):
    """(a): with every brick active the result IS the dense mesh"""
    same_mesh(got, (dense.verts, dense.tris, dense.attrs), "all bricks active")


def check_closed_result(dense, r, got):
    """(b): when the growth closed, the result is the dense mesh restricted to the extracted cells, that is a union of whole
    connected components of the dense mesh, and it holds every component that has a triangle in a cell of the seed bricks"""
    assert r.closed
    same_mesh(got, select_cells(dense, r.ext), "extracted cells")
    if len(dense.tris):
        face_label = dense.labels[dense.tris[:, 0]]
        kept = r.ext[tuple(dense.tri_cell.T)]
        assert not np.isin(face_label[~kept], np.unique(face_label[kept])).any(), "a component is only partly in the result"
        assert np.isin(np.unique(face_label[r.ext0[tuple(dense.tri_cell.T)]]), np.unique(face_label[kept])).all()


def check_seed_components(dense, r, got):
    """(b) as the cases are built: no grown brick meets a component the seeds do not, so the result is exactly the union of the
    components with a triangle in a cell of the seed bricks"""
    same_mesh(got, component_union(dense, r.ext0), "components of the seed bricks")


def largest_component_np(verts, tris, labels=None, components=None):
    """isosurface.largest_component in NumPy (most faces, ties to the smallest root)"""
    if not len(tris):
        return verts, tris
    lab = components(np.asarray(tris, np.int32), len(verts)) if labels is None else labels
    fl = lab[tris[:, 0]]
    roots, counts = np.unique(fl, return_counts=True)
    best = roots[np.argmax(counts)]
    keep_v = lab == best
    remap = np.cumsum(keep_v) - 1
    return verts[keep_v], remap[tris[fl == best]].astype(np.int32)
