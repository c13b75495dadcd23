"""Multi-view renders of a triangle mesh on the device (s3d_render.hip): project, bin, raster, shade.
Scan, sort and segment starts between the kernels are torch calls here, as in data/mesh_sampler.py.
Smooth normals, normal maps, the GGX light model and the material passes (s3d_render_pbr.hip) are the keyword
arguments shading / passes / lights / ambient of render_views; without them a call is what it was.
Shadows (s3d_ray.hip) are opt-in: render_views(shadows=True) sends one shadow ray per sample and light through a
uniform cell grid over the mesh; ray_occluded is the any-hit ray query under them, public on its own."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from .. import _lib
from . import camera

TILE = _lib.RENDER_TILE


def _f16(m):
    return (C.c_float * 16)(*[float(x) for x in np.asarray(m, dtype=np.float64).reshape(16)])


def _f3(v):
    return (C.c_float * 3)(*[float(x) for x in np.asarray(v, dtype=np.float64).reshape(3)])


def project(verts, matrix, Ws, Hs, near=camera.NEAR):
    """(xy_fixed int32 [V, 2], inv_w float32 [V]) of float32 device vertices: sample coordinates snapped to 1 / 256; a vertex
    with w <= near has inv_w = 0."""
    _lib.require_gpu(verts)
    v = verts.contiguous().float()
    V = v.shape[0]
    with torch.cuda.device(v.device):
        xy = torch.empty((V, 2), device=v.device, dtype=torch.int32)
        iw = torch.empty(V, device=v.device, dtype=torch.float32)
        _lib.check(_lib.load().s3d_render_project(_lib.ptr(v), V, _f16(matrix), int(Ws), int(Hs), float(near), _lib.ptr(xy), _lib.ptr(iw),
                                                  _lib.stream_ptr()))
    return xy, iw


def rasterize(xy_fixed, inv_w, faces, Ws, Hs, timer=None):
    """The raster stage on given snapped coordinates: dict with face_id int32 [Hs, Ws] (-1: none), depth float32 [Hs, Ws] (1 / w),
    count uint8 [Hs, Ws] (covering triangles, clamped at 255), status uint8 [F] (0 drawn, 1 a flagged corner, 2 out of range,
    3 zero area) and info: dropped / degenerate / near counts, the number of (tile, triangle) pairs and the longest tile list.
    timer(stage): called on the stream after every stage (tools/bench_render.py records a device event there)."""
    timer = timer or (lambda stage: None)
    _lib.require_gpu(xy_fixed)
    lib = _lib.load()
    Ws, Hs = int(Ws), int(Hs)
    xy = xy_fixed.contiguous().to(torch.int32)
    iw = inv_w.contiguous().float()
    t = faces.contiguous().to(torch.int32).reshape(-1, 3)
    V, F, dev = xy.shape[0], t.shape[0], xy.device
    n_tiles = -(-Ws // TILE) * -(-Hs // TILE)
    with torch.cuda.device(dev):
        st = _lib.stream_ptr()
        counts = torch.zeros(F, device=dev, dtype=torch.int64)
        status = torch.zeros(F, device=dev, dtype=torch.uint8)
        _lib.check(lib.s3d_render_bin_count(_lib.ptr(xy), _lib.ptr(iw), V, _lib.ptr(t), F, Ws, Hs, _lib.ptr(counts), _lib.ptr(status), st))
        timer("bin count")
        ends = torch.cumsum(counts, 0)
        n_pairs = int(ends[-1]) if F else 0
        if n_pairs > _lib.RENDER_MAX_PAIRS:
            raise NotImplementedError(f"rasterize: {n_pairs} (tile, triangle) pairs on a {Ws} x {Hs} sample grid: {n_pairs * 8 / 2 ** 30:.2f} GiB "
                                      f"of workspace, over the cap of {_lib.RENDER_MAX_PAIRS} pairs = 1 GiB")
        offsets = (ends - counts).contiguous()
        pair_tile = torch.empty(max(n_pairs, 1), device=dev, dtype=torch.int32)
        pair_tri = torch.empty(max(n_pairs, 1), device=dev, dtype=torch.int32)
        timer("scan")
        _lib.check(lib.s3d_render_bin_fill(_lib.ptr(xy), _lib.ptr(iw), V, _lib.ptr(t), F, Ws, Hs, _lib.ptr(offsets), n_pairs, _lib.ptr(pair_tile),
                                           _lib.ptr(pair_tri), st))
        timer("bin fill")
        keys, order = torch.sort(pair_tile[:n_pairs], stable=True)
        seg_tri = pair_tri[:n_pairs][order].contiguous()
        seg = torch.searchsorted(keys, torch.arange(n_tiles + 1, device=dev, dtype=torch.int32)).to(torch.int64).contiguous()
        timer("sort and segments")
        face_id = torch.empty((Hs, Ws), device=dev, dtype=torch.int32)
        depth = torch.empty((Hs, Ws), device=dev, dtype=torch.float32)
        count = torch.empty((Hs, Ws), device=dev, dtype=torch.uint8)
        _lib.check(lib.s3d_render_raster(_lib.ptr(xy), _lib.ptr(iw), V, _lib.ptr(t), F, Ws, Hs, _lib.ptr(seg), _lib.ptr(seg_tri), n_pairs,
                                         _lib.ptr(face_id), _lib.ptr(depth), _lib.ptr(count), st))
        timer("raster")
        hist = torch.bincount(status.long(), minlength=4).tolist() if F else [0, 0, 0, 0]
        longest = int((seg[1:] - seg[:-1]).max())
        torch.cuda.current_stream().synchronize()          # the temporaries above are done with
    info = {"dropped": hist[1] + hist[2] + hist[3], "near": hist[1], "out_of_range": hist[2], "degenerate": hist[3], "n_pairs": n_pairs,
            "longest_tile_list": longest}
    return {"face_id": face_id, "depth": depth, "count": count, "status": status, "info": info}


def pack_materials(materials, device):
    """(mat_table int64 [M, 3] = {byte offset, W, H}, kd float32 [M, 3], images uint8, image_bytes): the layout of
    s3d_meshsdf_texture.  materials: dicts with Kd and image (uint8 [H, W, 3+], array or tensor, top row first, or None)."""
    table, blobs, kds, off = [], [], [], 0
    for m in materials:
        kds.append([float(x) for x in m.get("Kd", (1.0, 1.0, 1.0))])
        img = m.get("image")
        if img is None:
            table.append([0, 0, 0])
            continue
        img = img if torch.is_tensor(img) else torch.from_numpy(np.array(img, dtype=np.uint8, order="C"))        # (a copy: PIL's is read-only)
        img = img.to(device)[..., :3].contiguous()
        table.append([off, img.shape[1], img.shape[0]])
        blobs.append(img.reshape(-1))
        off += img.numel()
    images = torch.cat(blobs) if blobs else torch.zeros(1, device=device, dtype=torch.uint8)
    return (torch.tensor(table, dtype=torch.int64, device=device).reshape(-1, 3).contiguous(),
            torch.tensor(kds, dtype=torch.float32, device=device).reshape(-1, 3).contiguous(), images.contiguous(), off)


def vertex_normals(verts, faces):
    """float32 [V, 3]: the area-weighted normal of every vertex (the normalised sum of cross(b - a, c - a) over its faces, in
    ascending corner order, float64 on the device); (0, 0, 0) for a vertex no face references or whose sum vanishes."""
    _lib.require_gpu(verts)
    v = verts.contiguous().float().reshape(-1, 3)
    t = faces.contiguous().to(torch.int32).reshape(-1, 3)
    V, F, dev = v.shape[0], t.shape[0], v.device
    with torch.cuda.device(dev):
        keys, order = torch.sort(t.reshape(-1).to(torch.int64), stable=True)
        start = torch.searchsorted(keys, torch.arange(V + 1, device=dev, dtype=torch.int64)).to(torch.int64).contiguous()
        order = order.contiguous()
        out = torch.empty((V, 3), device=dev, dtype=torch.float32)
        _lib.check(_lib.load().s3d_pbr_vertex_normals(_lib.ptr(v), V, _lib.ptr(t), F, _lib.ptr(order), _lib.ptr(start), _lib.ptr(out),
                                                         _lib.stream_ptr()))
        torch.cuda.current_stream().synchronize()          # the temporaries above are done with
    return out


def face_tangents(verts, faces, uvs):
    """float32 [F, 2, 3]: (T, B) = (d position / d u, d position / d v) of every face's uv map, uvs [F, 3, 2]; zeros where the
    uv triangle has no area."""
    _lib.require_gpu(verts)
    v = verts.contiguous().float().reshape(-1, 3)
    t = faces.contiguous().to(torch.int32).reshape(-1, 3)
    V, F, dev = v.shape[0], t.shape[0], v.device
    uv = uvs.to(dev).contiguous().float().reshape(F, 3, 2)
    with torch.cuda.device(dev):
        out = torch.empty((F, 2, 3), device=dev, dtype=torch.float32)
        _lib.check(_lib.load().s3d_pbr_face_tangents(_lib.ptr(v), V, _lib.ptr(t), F, _lib.ptr(uv), _lib.ptr(out), _lib.stream_ptr()))
        torch.cuda.current_stream().synchronize()
    return out


def eye_of(matrix):
    """float64 [3]: the centre of projection of an object-to-clip matrix, the point its x, y and w rows all send to 0."""
    m = np.asarray(matrix, dtype=np.float64).reshape(4, 4)[[0, 1, 3]]
    return -np.linalg.solve(m[:, :3], m[:, 3])


RAY_SLACK_REL = 2.0 ** -18           # the binning slack over the largest coordinate magnitude: twice the 2^-19 DESIGN.md §29 asks for
RAY_MAX_CELLS_PER_AXIS = 256
RAY_REACH_CAP = 1024.0               # ray origins count into the slack up to this many mesh magnitudes
SHADOW_T_MIN_REL = 1e-4              # default start of a shadow ray, in bounding-box diagonals


def ray_grid_dims(extent, n_faces):
    """The default resolution of the ray grid: ceil(sqrt(n_faces / 2)) cells along the longest side of the (padded) box, cubic
    cells, every dimension clamped to 1 .. RAY_MAX_CELLS_PER_AXIS — a surface of F faces then puts a few triangles into a cell
    it crosses."""
    ext = [float(x) for x in extent]
    n_long = min(RAY_MAX_CELLS_PER_AXIS, max(1, math.ceil(math.sqrt(max(int(n_faces), 0) / 2.0))))
    cell = max(ext) / n_long
    return tuple(min(RAY_MAX_CELLS_PER_AXIS, max(1, math.ceil(e / cell))) for e in ext)


def ray_grid_box(vmin, vmax, n_faces, grid=None, reach=0.0):
    """(origin float32 [3], cell, dims, slack) of the ray grid over the box vmin .. vmax: slack = RAY_SLACK_REL times the largest
    coordinate magnitude (of the box, and of the ray origins up to RAY_REACH_CAP box magnitudes: `reach`), the box padded by four
    slacks, dims = grid or ray_grid_dims, cell = the largest padded side / dims ratio (so the grid covers the box).  Pure host
    arithmetic (tests/test_render_shadow_host.py)."""
    lo, hi = np.asarray(vmin, dtype=np.float64).reshape(3), np.asarray(vmax, dtype=np.float64).reshape(3)
    mag = float(max(np.abs(lo).max(), np.abs(hi).max()))
    mag = mag if mag > 0 else 1.0
    mag = max(mag, min(float(reach), RAY_REACH_CAP * mag))
    slack = RAY_SLACK_REL * mag
    lo, hi = lo - 4 * slack, hi + 4 * slack
    if grid is None:
        dims = ray_grid_dims(hi - lo, n_faces)
    else:
        dims = tuple(int(x) for x in grid)
        if len(dims) != 3 or min(dims) < 1:
            raise ValueError(f"ray grid {grid!r}: three dimensions of at least 1")
    cell = float(max((hi[k] - lo[k]) / dims[k] for k in range(3))) * (1.0 + 1e-6)
    return lo.astype(np.float32), float(np.float32(cell)), dims, float(np.float32(slack))


def build_ray_grid(verts, faces, grid=None, reach=0.0):
    """The mesh as s3d_mesh_ray_occluded takes it: dict with tri9 [F, 9], the grid (o3, cell, d3 as ctypes; dims, slack), seg,
    seg_tri and n_pairs — s3d_meshsdf_bin_count / _bin_fill with the slack as their band, scan, stable sort and segment starts in
    torch, as MeshSampler._binned."""
    _lib.require_gpu(verts)
    lib = _lib.load()
    v = verts.contiguous().float().reshape(-1, 3)
    t = faces.contiguous().to(torch.int64).reshape(-1, 3)
    F, dev = t.shape[0], v.device
    with torch.cuda.device(dev):
        if F:
            if int(t.min()) < 0 or int(t.max()) >= v.shape[0]:
                raise ValueError(f"ray grid: face indices outside the {v.shape[0]} vertices")
            tri9 = v[t.reshape(-1)].reshape(F, 9).contiguous()
            c = tri9.reshape(-1, 3)
            c = c[torch.isfinite(c).all(1)]
            lo, hi = (c.min(0).values.double().cpu().numpy(), c.max(0).values.double().cpu().numpy()) if c.shape[0] else (np.zeros(3), np.ones(3))
        else:
            tri9 = torch.zeros((1, 9), device=dev, dtype=torch.float32)
            lo, hi = np.zeros(3), np.ones(3)
        origin, cell, dims, slack = ray_grid_box(lo, hi, F, grid, reach)
        o3, d3 = (C.c_float * 3)(*[float(x) for x in origin]), (C.c_int * 3)(*dims)
        n_cells = dims[0] * dims[1] * dims[2]
        st = _lib.stream_ptr()
        counts = torch.zeros(max(F, 1), device=dev, dtype=torch.int64)
        _lib.check(lib.s3d_meshsdf_bin_count(_lib.ptr(tri9), F, slack, o3, cell, d3, _lib.ptr(counts), st))
        ends = torch.cumsum(counts[:F], 0)
        n_pairs = int(ends[-1]) if F else 0
        if n_pairs > _lib.MESHSDF_MAX_PAIRS:
            raise NotImplementedError(f"ray grid: {n_pairs} (cell, triangle) pairs on a {dims[0]} x {dims[1]} x {dims[2]} grid, over the cap of "
                                      f"{_lib.MESHSDF_MAX_PAIRS}: pass a coarser grid")
        offsets = (ends - counts[:F]).contiguous() if F else counts
        pair_cell = torch.empty(max(n_pairs, 1), device=dev, dtype=torch.int64)
        pair_tri = torch.empty(max(n_pairs, 1), device=dev, dtype=torch.int32)
        _lib.check(lib.s3d_meshsdf_bin_fill(_lib.ptr(tri9), F, slack, o3, cell, d3, _lib.ptr(offsets), n_pairs, _lib.ptr(pair_cell),
                                            _lib.ptr(pair_tri), st))
        keys, order = torch.sort(pair_cell[:n_pairs], stable=True)
        seg_tri = pair_tri[:n_pairs][order].contiguous() if n_pairs else pair_tri
        seg = torch.searchsorted(keys, torch.arange(n_cells + 1, device=dev, dtype=torch.int64)).to(torch.int64).contiguous()
        torch.cuda.current_stream().synchronize()          # the temporaries above are done with
    return {"tri9": tri9, "F": F, "o3": o3, "cell": cell, "d3": d3, "dims": dims, "slack": slack, "seg": seg, "seg_tri": seg_tri, "n_pairs": n_pairs,
            "diagonal": float(np.linalg.norm(hi - lo))}


def ray_occluded(verts, faces, origins, dirs, skip_face=None, t_min=0.0, t_max=math.inf, grid=None):
    """(hit uint8 [n], status uint8 [n]) on the device: hit = 1 when the ray origins[i] + t dirs[i] crosses some triangle of the mesh
    other than skip_face[i] (int32, -1: none; None: none) at a parameter t in [t_min, t_max] — any hit, edges inclusive, fp32 in the
    order include/sin3dm_hip.h spells out, independent of the grid; not watertight across shared edges.  status: 0 walked, 1 the
    ray does not meet the grid box, 2 an origin or direction that is not finite or a zero direction (hit 0 for both).
    grid=(nx, ny, nz): the cell grid's resolution (None: ray_grid_dims).  Pass a grid built earlier (build_ray_grid) to reuse it."""
    _lib.require_gpu(verts)
    o = origins.contiguous().float().reshape(-1, 3)
    d = dirs.to(o.device).contiguous().float().reshape(-1, 3)
    n, dev = o.shape[0], o.device
    if d.shape[0] != n:
        raise ValueError(f"ray_occluded: {n} origins, {d.shape[0]} directions")
    sk = None
    if skip_face is not None:
        sk = skip_face.to(dev).contiguous().to(torch.int32).reshape(-1)
        if sk.shape[0] != n:
            raise ValueError(f"ray_occluded: {n} rays, {sk.shape[0]} faces to skip")
    if n == 0:
        return torch.zeros(0, device=dev, dtype=torch.uint8), torch.zeros(0, device=dev, dtype=torch.uint8)
    with torch.cuda.device(dev):
        if isinstance(grid, dict):
            g = grid
        else:
            fin = o[torch.isfinite(o)]
            g = build_ray_grid(verts, faces, grid, float(fin.abs().max()) if fin.numel() else 0.0)
        hit = torch.zeros(n, device=dev, dtype=torch.uint8)
        status = torch.zeros(n, device=dev, dtype=torch.uint8)
        _lib.check(_lib.load().s3d_mesh_ray_occluded(_lib.ptr(o), _lib.ptr(d), _lib.ptr(sk), n, float(t_min), float(t_max), _lib.ptr(g["tri9"]), g["F"],
                                                    g["o3"], g["cell"], g["d3"], _lib.ptr(g["seg"]), _lib.ptr(g["seg_tri"]), g["n_pairs"],
                                                    _lib.ptr(hit), _lib.ptr(status), _lib.stream_ptr()))
        torch.cuda.current_stream().synchronize()
    return hit, status


def shadow_mask(verts, faces, buffers, matrix, lights, t_min, grid):
    """lit uint8 [Hs, Ws] of one view: bit k set where light k reaches the sample (s3d_pbr_shadow_mask).  buffers: face_id,
    xy_fixed and inv_w of the view's raster stage; lights [n, 4]; grid: build_ray_grid's dict.  Enqueued, not synchronised."""
    v = verts.contiguous().float().reshape(-1, 3)
    t = faces.contiguous().to(torch.int32).reshape(-1, 3)
    face_id = buffers["face_id"]
    Hs, Ws = face_id.shape
    lights = np.asarray(lights, dtype=np.float64).reshape(-1, 4)
    light_arr = (C.c_float * max(4 * len(lights), 1))(*[float(x) for x in lights.reshape(-1)])
    with torch.cuda.device(v.device):
        lit = torch.empty((Hs, Ws), device=v.device, dtype=torch.uint8)
        _lib.check(_lib.load().s3d_pbr_shadow_mask(_lib.ptr(v), _lib.ptr(buffers["xy_fixed"]), _lib.ptr(buffers["inv_w"]), v.shape[0], _lib.ptr(t),
                                                     t.shape[0], _lib.ptr(face_id), Ws, Hs, _f16(matrix), light_arr, len(lights), float(t_min),
                                                     _lib.ptr(grid["tri9"]), grid["o3"], grid["cell"], grid["d3"], _lib.ptr(grid["seg"]),
                                                     _lib.ptr(grid["seg_tri"]), grid["n_pairs"], _lib.ptr(lit), _lib.stream_ptr()))
    return lit


SHADINGS = ("flat", "smooth", "pbr", "pbr_flat")


def _render_views_pbr(v, t, uvs, face_mat, materials, vertex_colors, views, W, H, ss, return_buffers, timer, shading, passes, lights, ambient,
                      normals=None, shadows=False, shadow_t_min=None, shadow_grid=None):
    """render_views with the light model of s3d_render_pbr.hip: one raster stage per view, one shade launch per pass.  shadows: the
    ray grid once per call, one shadow mask per view, and the shade launches read it (s3d_ray.hip)."""
    from . import pbr
    lib = _lib.load()
    dev, V, F = v.device, v.shape[0], t.shape[0]
    Ws, Hs = W * ss, H * ss
    single = isinstance(passes, str)
    names = (passes,) if single else tuple(passes)
    if not names or any(n not in _lib.RENDER_PASSES for n in names):
        raise ValueError(f"render_views: passes {passes!r} (of {_lib.RENDER_PASSES})")
    lights = pbr.three_light_rig() if lights is None else np.asarray(lights, dtype=np.float64).reshape(-1, 4)
    if len(lights) > _lib.RENDER_MAX_LIGHTS:
        raise ValueError(f"render_views: {len(lights)} lights (at most {_lib.RENDER_MAX_LIGHTS})")
    ambient = _lib.RENDER_PBR_AMBIENT if ambient is None else float(ambient)
    light_arr = (C.c_float * max(4 * len(lights), 1))(*[float(x) for x in lights.reshape(-1)])
    vcol = uv = fm = tang = nrm = None
    table = kd = images = None
    ptab = pfac = None
    n_mats = img_bytes = 0
    if uvs is not None:
        uv = uvs.to(dev).contiguous().float().reshape(F, 3, 2)
    is_pbr = shading in ("pbr", "pbr_flat")
    if vertex_colors is not None and not (is_pbr and materials):      # (pbr without materials: the colours are the albedo, as for smooth)
        vcol = vertex_colors.to(dev).contiguous().float().reshape(V, 3)
    elif materials:
        if face_mat is not None:
            fm = face_mat.to(dev).contiguous().to(torch.int32).reshape(F)
        if is_pbr:
            tab, fac, images, img_bytes = pbr.pack_pbr_materials(materials, dev)
            n_mats = tab.shape[0]
            if n_mats > _lib.RENDER_PBR_MAX_MATERIALS:
                raise NotImplementedError(f"render_views: {n_mats} PBR materials (at most {_lib.RENDER_PBR_MAX_MATERIALS} in one call)")
            ptab = (C.c_int64 * tab.size)(*[int(x) for x in tab.reshape(-1)])
            pfac = (C.c_float * fac.size)(*[float(x) for x in fac.reshape(-1)])
            if uv is not None and (tab[:, 3, 1] > 0).any():
                tang = face_tangents(v, t, uv)
        else:
            table, kd, images, img_bytes = pack_materials(materials, dev)
            n_mats = table.shape[0]
    if shading in ("smooth", "pbr"):
        if normals is not None:
            nrm = normals.to(dev).contiguous().float().reshape(-1, 3)
            if nrm.shape[0] != V:
                raise ValueError(f"render_views: {nrm.shape[0]} normals for {V} vertices")
        else:
            nrm = vertex_normals(v, t)
    out = {n: torch.empty((len(views), H, W, 4), device=dev, dtype=torch.uint8) for n in names}
    buffers = []
    grid = lit = None
    if shadows:
        timer("start")
        grid = shadow_grid if isinstance(shadow_grid, dict) else build_ray_grid(v, t, shadow_grid)
        t_min = SHADOW_T_MIN_REL * grid["diagonal"] if shadow_t_min is None else float(shadow_t_min)
        if not (t_min >= 0 and math.isfinite(t_min)):
            raise ValueError(f"render_views: shadow_t_min {shadow_t_min!r} (finite, not negative)")
        timer("grid")
    for k, view in enumerate(views):
        timer("start")
        xy, iw = project(v, view.matrix, Ws, Hs, view.near)
        timer("project")
        r = rasterize(xy, iw, t, Ws, Hs, timer)
        eye = _f3(eye_of(view.matrix))
        if shadows:
            lit = shadow_mask(v, t, dict(r, xy_fixed=xy, inv_w=iw), view.matrix, lights, t_min, grid)
            timer("shadow")
        with torch.cuda.device(dev):
            for n in names:
                if shadows:
                    _lib.check(lib.s3d_pbr_shade_lit(_lib.ptr(v), _lib.ptr(xy), _lib.ptr(iw), V, _lib.ptr(t), F, _lib.ptr(r["face_id"]), Ws, Hs, ss,
                                                     _f16(view.matrix), _lib.ptr(vcol), _lib.ptr(uv), _lib.ptr(fm), _lib.ptr(table), _lib.ptr(kd),
                                                     n_mats, _lib.ptr(images) if img_bytes else C.c_void_p(0), img_bytes, _lib.ptr(nrm),
                                                     _lib.ptr(tang), ptab, pfac, eye, light_arr, len(lights), ambient,
                                                     _lib.RENDER_PASSES.index(n), _lib.ptr(lit), _lib.ptr(out[n][k]), _lib.stream_ptr()))
                    continue
                _lib.check(lib.s3d_pbr_shade(_lib.ptr(v), _lib.ptr(xy), _lib.ptr(iw), V, _lib.ptr(t), F, _lib.ptr(r["face_id"]), Ws, Hs, ss,
                                                    _f16(view.matrix), _lib.ptr(vcol), _lib.ptr(uv), _lib.ptr(fm), _lib.ptr(table), _lib.ptr(kd),
                                                    n_mats, _lib.ptr(images) if img_bytes else C.c_void_p(0), img_bytes, _lib.ptr(nrm),
                                                    _lib.ptr(tang), ptab, pfac, eye, light_arr, len(lights), ambient,
                                                    _lib.RENDER_PASSES.index(n), _lib.ptr(out[n][k]), _lib.stream_ptr()))
        timer("shade")
        if return_buffers:
            buffers.append(dict(r, xy_fixed=xy, inv_w=iw, **({"lit": lit} if shadows else {})))
    with torch.cuda.device(dev):
        torch.cuda.current_stream().synchronize()
    res = out[names[0]] if single or len(names) == 1 else out
    return (res, buffers) if return_buffers else res


def render_views(verts, faces, *, uvs=None, face_mat=None, materials=None, vertex_colors=None, views=None, resolution=(512, 512),
                 supersample=2, return_buffers=False, timer=None, shading="flat", passes=("shaded",), lights=None, ambient=None, normals=None,
                 shadows=False, shadow_t_min=None, shadow_grid=None):
    """uint8 [n_views, H, W, 4] renders of a mesh given as device tensors: verts [V, 3], faces [F, 3].
    shading / passes / lights / ambient (a call without them is the flat shader of §22, bit for bit):
    shading "smooth": the same base colours under area-weighted vertex normals and the GGX light model (metallic 0, roughness
    0.5); "pbr": the materials' further entries are used (rendering/pbr.py: metallic_image, roughness_image, normal_image, Pm,
    Pr) on smooth normals, "pbr_flat" on flat ones — materials come before vertex colours there, and without materials the
    vertex colours are the albedo, as for "smooth"; "flat" with any of the other three given: the light model on flat normals.
    passes: names of _lib.RENDER_PASSES; one pass returns the array, several a dict of arrays by name (the raster stage runs once per view either way).  lights:
    [n <= 4, 4] unit directions towards the light in the space of verts and intensities (None: pbr.three_light_rig());
    ambient: scalar (None: _lib.RENDER_PBR_AMBIENT).  normals [V, 3]: vertex normals that replace the area-weighted ones under
    "smooth" and "pbr" (the field normals of decode_mesh(normals="field"), say); the flat shadings do not read them.
    shadows=True (like any of the options above it takes the light-model path, on flat normals under "flat"): a light
    adds nothing at a sample it does not reach — one shadow ray per sample and light the sample's face is turned to, through a
    uniform cell grid built once per call.  Hard shadows of the mesh on itself: no penumbra, no ground plane, no ambient occlusion;
    the terminator follows the faces under smooth normals too.  shadow_t_min: where the shadow rays start (None: SHADOW_T_MIN_REL =
    1e-4 of the bounding-box diagonal; contact shadows shorter than it are lost).  shadow_grid=(nx, ny, nz): the grid's resolution
    (None: ray_grid_dims, from the face count and the box, 1 to 256 a side).  The albedo, metallic, roughness and normal passes
    do not change; the geo pass is shadowed.
    Base colour: vertex_colors [V, 3] in [0, 1]; or materials (dicts with Kd and image, see pack_materials) with face_mat [F]
    (None: material 0) and per-corner uvs [F, 3, 2]; or white.  views: camera.View objects (None: the reference's eight views of
    the mesh normalised by its bounding box, camera.standard_views).  resolution: (W, H).  Alpha is the covered share of a pixel.
    return_buffers: also a list with, per view, face_id / depth / count [H ss, W ss], xy_fixed, inv_w, status and info, and with
    shadows lit uint8 [H ss, W ss] (bit k: light k reaches the sample).
    timer: see rasterize; with shadows also "grid" (once) and "shadow" (per view)."""
    timer = timer or (lambda stage: None)
    _lib.require_gpu(verts)
    lib = _lib.load()
    W, H, ss = int(resolution[0]), int(resolution[1]), int(supersample)
    if W < 1 or H < 1 or not 1 <= ss <= 8:
        raise ValueError(f"render_views: resolution {W} x {H}, supersample {ss} (1 to 8)")
    Ws, Hs = W * ss, H * ss
    dev = verts.device
    v = verts.contiguous().float().reshape(-1, 3)
    t = faces.contiguous().to(torch.int32).reshape(-1, 3)
    V, F = v.shape[0], t.shape[0]
    if views is None:
        if V:
            lo, hi = v.min(0).values.double().cpu().numpy(), v.max(0).values.double().cpu().numpy()
        else:
            lo, hi = np.zeros(3), np.ones(3)
        views = camera.standard_views(lo, hi, (W, H))
    if shading not in SHADINGS:
        raise ValueError(f"render_views: shading {shading!r} (of {SHADINGS})")
    if shading != "flat" or tuple(passes) != ("shaded",) or isinstance(passes, str) or lights is not None or ambient is not None or shadows:
        return _render_views_pbr(v, t, uvs, face_mat, materials, vertex_colors, views, W, H, ss, return_buffers, timer, shading, passes, lights,
                                 ambient, normals, shadows, shadow_t_min, shadow_grid)
    vcol = uv = fm = None
    table = kd = images = None
    n_mats = img_bytes = 0
    if vertex_colors is not None:
        vcol = vertex_colors.to(dev).contiguous().float().reshape(V, 3)
    elif materials:
        table, kd, images, img_bytes = pack_materials(materials, dev)
        n_mats = table.shape[0]
        if uvs is not None:
            uv = uvs.to(dev).contiguous().float().reshape(F, 3, 2)
        if face_mat is not None:
            fm = face_mat.to(dev).contiguous().to(torch.int32).reshape(F)
    out = torch.empty((len(views), H, W, 4), device=dev, dtype=torch.uint8)
    buffers = []
    for k, view in enumerate(views):
        timer("start")
        xy, iw = project(v, view.matrix, Ws, Hs, view.near)
        timer("project")
        r = rasterize(xy, iw, t, Ws, Hs, timer)
        with torch.cuda.device(dev):
            _lib.check(lib.s3d_render_shade(_lib.ptr(v), _lib.ptr(xy), _lib.ptr(iw), V, _lib.ptr(t), F, _lib.ptr(r["face_id"]), Ws, Hs, ss,
                                            _f16(view.matrix), _f3(view.light), _lib.ptr(vcol), _lib.ptr(uv), _lib.ptr(fm), _lib.ptr(table),
                                            _lib.ptr(kd), n_mats, _lib.ptr(images) if img_bytes else C.c_void_p(0), img_bytes,
                                            _lib.ptr(out[k]), _lib.stream_ptr()))
        timer("shade")
        if return_buffers:
            buffers.append(dict(r, xy_fixed=xy, inv_w=iw))
    with torch.cuda.device(dev):
        torch.cuda.current_stream().synchronize()
    return (out, buffers) if return_buffers else out
