"""Regions of the volume as known regions on a triplane: the `y0` / `mask` pair of GaussianDiffusion's `known=` (outpainting and
local editing).  Host-side plumbing; our own design, the reference has no such code.

A latent triplane stores the volume's cells as three axis-aligned projections, xy [H, W], xz [H, D] and yz [W, D] (x runs along H,
y along W, z along D).  A 3-D box (x0, x1, y0, y1, z0, z1) in latent cells therefore marks its projection on each plane,

    xy[x0:x1, y0:y1]    xz[x0:x1, z0:z1]    yz[y0:y1, z0:z1]

and that is the limit of what a box can say: a plane pixel stands for a whole column of the volume, so keeping the xy projection of
a box also pins, on that plane, everything in front of and behind the box.  `planes=` restricts an operation to a subset.
"""
from __future__ import annotations

import math

import torch

PLANES = ("xy", "xz", "yz")
_AXES = {"xy": (0, 1), "xz": (0, 2), "yz": (1, 2)}          # the volume axes (x, y, z = 0, 1, 2) a plane's rows and columns run along


def _planes(planes):
    if planes is None:
        return PLANES
    if isinstance(planes, str):
        planes = [p for p in planes.replace(",", " ").split() if p]
    planes = tuple(planes)
    for p in planes:
        if p not in PLANES:
            raise ValueError(f"plane {p!r}: expected a subset of {PLANES}")
    return tuple(p for p in PLANES if p in planes)


def cells_from_fractions(box, hwd):
    """A box given in fractions of the volume (x0, x1, y0, y1, z0, z1 in [0, 1]) in cells: floor(lo * n), ceil(hi * n)."""
    box = tuple(float(v) for v in box)
    assert len(box) == 6
    out = []
    for a, n in enumerate(hwd):
        out += [int(math.floor(box[2 * a] * n)), int(math.ceil(box[2 * a + 1] * n))]
    return tuple(out)


def _clip(box, hwd):
    box = tuple(int(v) for v in box)
    assert len(box) == 6
    out = []
    for a, n in enumerate(hwd):
        out += [max(box[2 * a], 0), min(box[2 * a + 1], int(n))]
    if any(out[2 * a + 1] <= out[2 * a] for a in range(3)):
        raise ValueError(f"box {box} is empty on a canvas of {tuple(hwd)} cells")
    return tuple(out)


def _ramp(lo, hi, n, feather):
    """Weights of cells lo..hi-1 along one axis of n cells: 1, or with feather = f a linear ramp over the f cells inside each end
    of the box that has free cells beyond it (an end on the canvas border has nothing to blend into)."""
    w = torch.ones(hi - lo)
    f = int(feather)
    if f > 0:
        j = torch.arange(hi - lo, dtype=torch.float32)
        if lo > 0:
            w = torch.minimum(w, (j + 1) / (f + 1))
        if hi < n:
            w = torch.minimum(w, (hi - lo - j) / (f + 1))
    return w


def box_mask(hwd, box, planes=None, feather=0):
    """{plane: [rows, cols] float mask} of a 3-D box (cells, clipped to the canvas) on a canvas of (H, W, D) cells: 1 inside the
    projection (with `feather` = n a linear ramp over n cells inside the box, the smaller of the two axes' weights), 0 outside; an
    all-zero mask for a plane that `planes` leaves out."""
    box = _clip(box, hwd)
    use = _planes(planes)
    out = {}
    for p in PLANES:
        r, c = _AXES[p]
        m = torch.zeros(int(hwd[r]), int(hwd[c]))
        if p in use:
            wr = _ramp(box[2 * r], box[2 * r + 1], int(hwd[r]), feather)
            wc = _ramp(box[2 * c], box[2 * c + 1], int(hwd[c]), feather)
            m[box[2 * r]:box[2 * r + 1], box[2 * c]:box[2 * c + 1]] = torch.minimum(wr[:, None], wc[None, :])
        out[p] = m
    return out


# ---------------------------------------------------------------------------------------------------- operations
def keep(box, planes=None, feather=0):
    """The source cells of `box` stay where they are."""
    return dict(op="keep", box=tuple(int(v) for v in box), planes=planes, feather=int(feather))


def paste(src_box, dst_corner, planes=None, feather=0):
    """The source cells of `src_box` appear with their low corner at `dst_corner` (x, y, z) of the canvas."""
    return dict(op="paste", box=tuple(int(v) for v in src_box), dst=tuple(int(v) for v in dst_corner), planes=planes,
                feather=int(feather))


def outpaint(grow, planes=None, feather=0):
    """The canvas is the source grown by grow = ((x_lo, x_hi), (y_lo, y_hi), (z_lo, z_hi)) cells per side, and the whole source is
    kept at that offset.  planes=None keeps only the planes that contain a grown axis: a plane without one has the size it had, and
    each of its pixels is a column through old AND new material — it stays free, and the sampler re-draws it in agreement with
    the kept planes."""
    grow = tuple((int(a), int(b)) for a, b in grow)
    assert len(grow) == 3 and all(a >= 0 and b >= 0 for a, b in grow)
    return dict(op="outpaint", grow=grow, planes=planes, feather=int(feather))


def outpaint_canvas(src_hwd, grow):
    """The canvas (H, W, D) of outpaint(grow) on a source of src_hwd cells."""
    return tuple(int(n) + int(a) + int(b) for n, (a, b) in zip(src_hwd, grow))


def outpaint_planes(grow):
    """The planes outpaint(grow) keeps by default: those that contain a grown axis."""
    grown = [a for a, (lo, hi) in enumerate(grow) if lo or hi]
    return tuple(p for p in PLANES if any(a in _AXES[p] for a in grown))


def build_known(src_planes, canvas_hwd, ops):
    """(y0 [C, H+D, W+D], mask [C, H+D, W+D]) for a canvas of (H, W, D) cells: the composed source latent placed by `ops` (keep /
    paste / outpaint, later ones overwrite earlier ones where they overlap) and the mask that goes with it; zero where nothing is
    known and in the D x D corner.  src_planes: (xy [C, H0, W0], xz [C, H0, D0], yz [C, W0, D0]), e.g.
    load_triplane_data(path, compose=False).  Boxes are clipped to source and canvas; an empty one is a ValueError."""
    from .triplane_util import compose_featmaps
    src = dict(zip(PLANES, src_planes))
    C = src["xy"].shape[0]
    src_hwd = (src["xy"].shape[1], src["xy"].shape[2], src["xz"].shape[2])
    assert src["xz"].shape[1] == src_hwd[0] and tuple(src["yz"].shape[1:]) == (src_hwd[1], src_hwd[2])
    hwd = tuple(int(v) for v in canvas_hwd)
    dev, dt = src["xy"].device, src["xy"].dtype
    y0 = {p: torch.zeros((C, hwd[_AXES[p][0]], hwd[_AXES[p][1]]), device=dev, dtype=dt) for p in PLANES}
    mask = {p: torch.zeros((hwd[_AXES[p][0]], hwd[_AXES[p][1]]), device=dev, dtype=dt) for p in PLANES}
    for o in ops:
        if o["op"] == "outpaint":
            if outpaint_canvas(src_hwd, o["grow"]) != hwd:
                raise ValueError(f"outpaint{o['grow']} of a {src_hwd} source is a {outpaint_canvas(src_hwd, o['grow'])} canvas, not {hwd}")
            sbox = (0, src_hwd[0], 0, src_hwd[1], 0, src_hwd[2])
            shift = tuple(g[0] for g in o["grow"])
            planes = o["planes"] if o["planes"] is not None else outpaint_planes(o["grow"])
        else:
            sbox = o["box"]
            shift = (0, 0, 0) if o["op"] == "keep" else tuple(o["dst"][a] - o["box"][2 * a] for a in range(3))
            planes = o["planes"]
        sbox = _clip(sbox, src_hwd)
        dbox = _clip(tuple(sbox[2 * a + k] + shift[a] for a in range(3) for k in range(2)), hwd)
        sbox = tuple(dbox[2 * a + k] - shift[a] for a in range(3) for k in range(2))
        m = box_mask(hwd, dbox, planes, o["feather"])
        for p in _planes(planes):
            r, c = _AXES[p]
            ds = (slice(dbox[2 * r], dbox[2 * r + 1]), slice(dbox[2 * c], dbox[2 * c + 1]))
            ss = (slice(sbox[2 * r], sbox[2 * r + 1]), slice(sbox[2 * c], sbox[2 * c + 1]))
            y0[p][(slice(None),) + ds] = src[p][(slice(None),) + ss]
            mask[p][ds] = m[p][ds].to(device=dev, dtype=dt)
    y0c, _ = compose_featmaps(y0["xy"], y0["xz"], y0["yz"])
    mc, _ = compose_featmaps(mask["xy"], mask["xz"], mask["yz"])
    return y0c, mc[None].expand(C, -1, -1)
