"""ShapeAutoEncoder (reference: src/encoding/model.py): checkpoints, decode, and the auto-encoder training loop
(:51-139, 178-258, 309-317) on the MI355X, and the mesh export: decode_mesh (vertex-coloured OBJ, the default) and
decode_texmesh (:362-473: decimated, UV-mapped, textured OBJ/MTL/PNG or GLB by an own design).  The
tensorboard figures are out of scope."""
from __future__ import annotations

import ctypes as C
import json
import os

import numpy as np
import torch
import torch.nn.functional as F

from .. import _lib
from .networks import get_networks


def _fma_f32(q, b, c):
    """float32 [n]: q * b + c with a single rounding to nearest even (q float32 [n], b and c float32 values), exact through rationals
    — a host fused multiply-add for the few thousand axis coordinates of index_sampler."""
    from fractions import Fraction
    out = np.empty(len(q), np.float32)
    fb, fc = Fraction(float(np.float32(b))), Fraction(float(np.float32(c)))
    for n, x in enumerate(np.asarray(q, np.float32)):
        exact = Fraction(float(x)) * fb + fc
        mid = np.float32(float(exact))
        near = (np.nextafter(mid, np.float32(-np.inf)), mid, np.nextafter(mid, np.float32(np.inf)))
        out[n] = min(near, key=lambda v: (abs(Fraction(float(v)) - exact), int(np.float32(v).view(np.uint32)) & 1))
    return out

_SDF_LOSS = {"l1": 0, "weightedl1": 1}
_TEX_LOSS = {"l1": 0, "l2": 1, "huber": 2}


def ae_loss_cfg(sdf_loss, tex_loss, sdf_threshold, tex_threshold_ratio=0.999, tex_weight=1.0, sdf_renorm=False):
    """The s3d_ae_loss_cfg of _forward_batch (reference :186-225) from the CLI's loss names.  The reference's texture band is
    `gt_sdf.abs() < sdf_threshold * tex_threshold_ratio`: a float32 tensor against a Python float, so the bound is the
    double product rounded once to float32.  The library multiplies its two float fields, which would round each factor
    first (one ulp lower or higher for about a quarter of thresholds), so the product is formed here in double and passed
    as the threshold with a ratio of exactly 1.0."""
    band = (1.0 if sdf_renorm else float(sdf_threshold)) * float(tex_threshold_ratio)
    return _lib.AeLossCfg(_SDF_LOSS[sdf_loss], _TEX_LOSS[tex_loss], band, 1.0, tex_weight)


class FlatGroupAdamW:
    """torch.optim.AdamW over the auto-encoder's two parameter groups (geo: lr*split, tex: lr; betas 0.9/0.999, eps 1e-8,
    weight_decay 0.01 = torch's default, which the reference inherits at model.py:131-137) followed by ExponentialLR,
    on the flat parameter vector: two launches of the fused Adam kernel per step.  The geometry-only net (data_type sdf) has no
    tex group: one group at the geometry group's rate, lr*split when split > 0 (the reference crashes there in
    tex_parameters())."""

    def __init__(self, net, lr, lr_split=-1.0, lr_decay=1.0, weight_decay=0.01):
        self.net = net
        flat = net.flat_parameters
        tb = net.tex_group_begin
        self.ranges = tuple(r for r in ((0, tb), (tb, flat.numel())) if r[1] > r[0])
        self.lrs = [lr * lr_split if lr_split > 0 else lr, lr][:len(self.ranges)]
        self.lr_decay, self.weight_decay = float(lr_decay), float(weight_decay)
        self.exp_avg, self.exp_avg_sq = torch.zeros_like(flat), torch.zeros_like(flat)
        self.steps = 0

    def step(self, flat_grad):
        flat = self.net.flat_parameters
        self.steps += 1
        lib = _lib.load()
        none = (C.c_void_p * 1)(None)
        rates = (C.c_float * 1)(0.0)
        with torch.cuda.device(flat.device):
            for (b, e), lr in zip(self.ranges, self.lrs):
                _lib.check(lib.s3d_train_adamw_ema(_lib.ptr(flat[b:e]), _lib.ptr(flat_grad[b:e]), _lib.ptr(self.exp_avg[b:e]),
                                                   _lib.ptr(self.exp_avg_sq[b:e]), none, rates, 0, e - b, lr, 0.9, 0.999, 1e-8,
                                                   self.weight_decay, self.steps, _lib.stream_ptr()))
        self.net.mark_parameters_changed()
        self.lrs = [lr * self.lr_decay for lr in self.lrs]            # ExponentialLR.step()

    def state_dict(self):
        return {"steps": self.steps, "lrs": list(self.lrs), "exp_avg": self.exp_avg.cpu(), "exp_avg_sq": self.exp_avg_sq.cpu()}

    def load_state_dict(self, sd):
        self.steps, self.lrs = int(sd["steps"]), list(sd["lrs"])
        self.exp_avg.copy_(sd["exp_avg"]); self.exp_avg_sq.copy_(sd["exp_avg_sq"])


class ShapeAutoEncoder:
    """Reads and writes `<log_dir>/ckpt_{name}.pth` exactly where the reference does (src/encoding/model.py:143, 161), so an
    experiment directory trained by either side loads on the other; trains, encodes and decodes on the MI355X."""

    def __init__(self, log_dir, cfg, device=None):
        if getattr(cfg, "data_type", "sdftex") == "sdfpbr" and getattr(cfg, "tex_loss", "l1") != "l1":
            # the reference defines only l1 for sdfpbr (:226-233) and silently trains without any material loss otherwise
            raise ValueError(f"--tex_loss {cfg.tex_loss} with --data_type sdfpbr: the material losses (rgb, mr, normal) are "
                             "defined for l1 only")
        self.log_dir = log_dir
        self.device = device or torch.device(f"cuda:{getattr(cfg, 'gpu_id', 0)}")
        self.net = get_networks(cfg).to(self.device)
        self.aabb = self.net.aabb.clone()
        self.featmap_size = None
        # training hyper-parameters (reference :18-37)
        g = lambda k, d: getattr(cfg, k, d)
        self.batch_size, self.n_iters, self.vol_ratio = g("enc_batch_size", 65536), g("enc_n_iters", 25000), g("vol_ratio", 0.1)
        self.fm_reso, self.data_type = g("fm_reso", 128), g("data_type", "sdftex")
        self.sdf_loss_type, self.tex_loss_type = g("sdf_loss", "weightedl1"), g("tex_loss", "l1")
        self.tex_weight, self.tex_threshold_ratio = g("tex_weight", 1.0), g("tex_threshold_ratio", 0.999)
        self.sdf_renorm = g("sdf_renorm", 0)
        self.init_lr, self.lr_split, self.min_lr_ratio = g("enc_lr", 5e-3), g("enc_lr_split", -1), g("enc_lr_decay", 0.01)
        self.material = {"Ka": None, "Kd": None, "Ks": None, "Ns": None}
        self.sdf_threshold = None
        self.input_grid = None

    def load_ckpt(self, name=None):
        """Reference :158-176 — `<log_dir>/ckpt_{name}.pth`, dict {net, optimizer, scheduler, Ka, Kd, Ks, Ns, aabb,
        featmap_size}.  (Directories written by round 1 of this build kept it under `model/`: read as a fallback.)"""
        path = name if name and os.path.isabs(str(name)) else os.path.join(self.log_dir, f"ckpt_{name}.pth")
        if not os.path.exists(path) and os.path.exists(os.path.join(self.log_dir, "model", f"ckpt_{name}.pth")):
            path = os.path.join(self.log_dir, "model", f"ckpt_{name}.pth")
        ckpt = torch.load(path, map_location="cpu", weights_only=False)
        self.net.load_state_dict(ckpt["net"])
        self.aabb = torch.as_tensor(ckpt["aabb"], dtype=torch.float32).to(self.device)
        self.net.reset_aabb(self.aabb)
        self.featmap_size = tuple(ckpt["featmap_size"])
        self.material = {k: ckpt.get(k) for k in ("Ka", "Kd", "Ks", "Ns")}

    def _resize_aabb(self, featmap_size):
        """aabb scaled by the feature-map ratio for retargeted triplanes (reference :351-360)."""
        if self.featmap_size is None or tuple(featmap_size) == tuple(self.featmap_size):
            return self.aabb
        scale = torch.tensor([featmap_size[i] / self.featmap_size[i] for i in range(3)], device=self.aabb.device)
        new = self.aabb.clone()
        new[:3] = self.aabb[:3] * scale
        new[3:] = self.aabb[3:] * scale
        return new

    @torch.no_grad()
    def decode_batch(self, triplane_feat, points, batch_size=2 ** 14, aabb=None):
        """Reference :319-333.  Any chunking gives identical per-point results, so all points go in one launch."""
        self.net.eval()
        return self.net.decode(points, triplane_feat, aabb=self.aabb if aabb is None else aabb, clamp_color=True)

    @torch.no_grad()
    def decode_grid(self, triplane_feat, reso, batch_size=2 ** 14, aabb=None):
        """Reference :335-349 -> [Nx, Ny, Nz, 1 | 4 | 9] (sdf | sdftex | sdfpbr), colour / material columns clamped to [0,1]."""
        self.net.eval()
        return self.net.decode_grid(triplane_feat, reso, aabb=self.aabb if aabb is None else aabb)

    @torch.no_grad()
    def decode_voxel(self, save_dir, triplane_feat, reso):
        """Reference :475-488: occupancy = sdf < 0, saved as r{reso}_voxel.npz."""
        H, W = triplane_feat[0].shape[-2:]
        D = triplane_feat[1].shape[-1]
        grid = self.decode_grid(triplane_feat, reso, aabb=self._resize_aabb((H, W, D)))
        vox = (grid[..., 0] < 0).cpu().numpy()
        os.makedirs(save_dir, exist_ok=True)
        np.savez_compressed(os.path.join(save_dir, f"r{reso}_voxel.npz"), voxel=vox)
        return vox

    def index_sampler(self, triplane_feat, aabb, reso):
        """(sample_fn, dims) for isosurface.marching_cubes_sparse: sample_fn maps float32 index coordinates [M,3] of the decode grid
        (integers: its samples; x.5: the brick-corner lattice) to net.decode(points, ..., clamp_color=True).  The points are
        k_decode's own grid expression AS COMPILED: q = (0.5 + i) / gdim rounded to float32 (IEEE division), then q * gsize + amin
        with ONE rounding — hipcc contracts that product and sum into a fused multiply-add, the __fmul_rn / __fadd_rn spelling
        notwithstanding (tools/compare_isa.py s3d_decoder.hip --kernels k_decodeI holds the kernel's instructions in place).  They
        are taken per axis on the host, exactly, and gathered on the device, so a band sample carries the bits of decode_grid's; the device test of
        decode_mesh(sparse=...) against the dense files is what notices if either side changes."""
        self.net.eval()
        a = aabb.detach().to("cpu", torch.float32).reshape(6)
        dims = (C.c_int * 3)()
        _lib.check(_lib.load().s3d_decoder_grid_dims((C.c_float * 6)(*[float(v) for v in a]), int(reso), dims))
        dims = (dims[0], dims[1], dims[2])
        dev = triplane_feat[0].device
        tabs = []
        for k in range(3):                          # entry j: the coordinate i = j / 2 - 0.5, j = 0 .. 2 dims (every sample and half step)
            i = torch.arange(2 * dims[k] + 1, dtype=torch.float32) / 2.0 - 0.5
            q = ((0.5 + i) / float(dims[k])).numpy()
            tabs.append(torch.from_numpy(_fma_f32(q, (a[3 + k] - a[k]).item(), a[k].item())).to(dev))

        def sample_fn(idx):
            j = (idx * 2.0 + 1.0).round().long()
            pts = torch.stack([tabs[k][j[:, k].clamp(0, 2 * dims[k])] for k in range(3)], 1)
            return self.net.decode(pts, triplane_feat, aabb=aabb, clamp_color=True)
        return sample_fn, dims

    def _sparse_isosurface(self, triplane_feat, aabb, reso, block, dilate, n_attr, occupancy):
        """the iso-surface at level 0 of the padded decode grid from its narrow band -> (verts, tris, attrs, occupancy or None)"""
        from .isosurface import marching_cubes_sparse
        if block not in (4, 8, 16):
            raise ValueError(f"sparse={block!r}: expected None or a brick size of 4, 8 or 16")
        sample_fn, dims = self.index_sampler(triplane_feat, aabb, reso)
        verts, tris, attrs, info = marching_cubes_sparse(sample_fn, dims, 0.0, 1.0, n_attr=n_attr, block=block, dilate=dilate,
                                                         return_info=True, occupancy=occupancy, device=triplane_feat[0].device)
        if not info["closed"]:
            import warnings
            warnings.warn(f"sparse iso-surface: the growth did not close in {info['rounds']} rounds; the mesh may have open borders")
        self.last_sparse_info = {k: v for k, v in info.items() if k != "occupancy"}
        return verts, tris, attrs, info.get("occupancy")

    def _refine_and_normals(self, triplane_feat, aabb, verts, tris, reso, box_size, refine, refine_max_move, normals):
        """The field's part of the mesh exports: `refine` Newton steps of the vertices onto the decoded zero level
        set, each step and the total move clamped to refine_max_move cells of the decode grid (box_size / reso, world units) per
        component, and with normals="field" the unit gradient at the final vertices (sdf < 0 is inside: +g points outward), the
        area-weighted normal where the gradient vanishes.  -> (verts, normals or None); faces are never changed."""
        if normals not in (None, "field"):
            raise ValueError(f"normals {normals!r}: expected 'field' (or None)")
        refine = int(refine)
        if refine < 0 or not refine_max_move > 0:
            raise ValueError(f"refine={refine}, refine_max_move={refine_max_move}: expected refine >= 0 and a positive move")
        if (refine == 0 and normals is None) or verts.shape[0] == 0:
            return verts, (verts.new_zeros((0, 3)) if normals is not None else None)
        self.net.eval()
        limit = float(refine_max_move) * float(box_size) / float(reso)
        verts, _, grad = self.net.project_to_surface(verts, triplane_feat, aabb=aabb, iters=refine, max_step=limit, max_move=limit)
        if normals is None:
            return verts, None
        from ..rendering.rasterizer import vertex_normals
        g2 = (grad * grad).sum(1, keepdim=True)
        flat = g2[:, 0] < 1e-20
        n = grad / g2.clamp_min(1e-20).sqrt()
        if bool(flat.any()):
            n = torch.where(flat[:, None], vertex_normals(verts, tris), n)
        return verts, n

    @torch.no_grad()
    def decode_mesh(self, save_dir, triplane_feat, reso, name="object.obj", only_largest_cc=True, save_voxel=True, refine=0,
                    refine_max_move=0.5, normals=None, return_normals=False, sparse=None, sparse_dilate=0):
        """The geometry half of decode_texmesh (reference :362-390): decode_grid -> voxel.npz -> iso-surface of the
        padded SDF grid at level 0 -> largest connected component -> `v / reso * box_size + box_min`, all on the device
        (sdfgrid_to_mesh, utils3d.py:196-208, used PyMCubes + point_cloud_utils on the CPU).  The decoded colour is
        interpolated onto the vertices and written as a vertex-coloured OBJ (sdfpbr: the albedo; sdf: an OBJ without
        colours); decimation, UV atlas and the baked texture that follow in the reference are decode_texmesh.
        refine=K > 0 projects the vertices onto the decoded zero level set after the re-normalisation (K Newton steps, at most
        refine_max_move cells per axis; the colours stay the interpolated ones); normals="field" writes the unit gradient there as
        `vn` lines (_refine_and_normals).  return_normals: a fourth entry, the normals [V,3] (None without them).  With the
        defaults the file and the returned tuple are what they always were.
        sparse=4 | 8 | 16 (+ sparse_dilate): the narrow-band front end (_sparse_isosurface) in place of the dense grid
        — decode_grid is never called, voxel.npz comes from the band; everything after the iso-surface is the same code."""
        from .isosurface import export_obj, largest_component, marching_cubes
        H, W = triplane_feat[0].shape[-2:]
        D = triplane_feat[1].shape[-1]
        aabb = self._resize_aabb((H, W, D))
        os.makedirs(save_dir, exist_ok=True)
        # vertex colour: the decoded rgb (sdftex), the albedo = columns 1..3 (sdfpbr), none (sdf)
        if sparse is not None:
            verts, tris, cols, occ = self._sparse_isosurface(triplane_feat, aabb, reso, sparse, sparse_dilate,
                                                             min(self.net.out_channels - 1, 3), save_voxel)
            if save_voxel:
                np.savez_compressed(os.path.join(save_dir, "voxel.npz"), vox_grid=occ.bool().cpu().numpy())
        else:
            grid = self.decode_grid(triplane_feat, reso, aabb=aabb)              # [Nx, Ny, Nz, 1+3], colours clamped
            if save_voxel:
                np.savez_compressed(os.path.join(save_dir, "voxel.npz"), vox_grid=(grid[..., 0] < 0).cpu().numpy())
            verts, tris, cols = marching_cubes(grid, 0.0, 1.0, n_attr=min(grid.shape[-1] - 1, 3))
        if only_largest_cc:
            verts, tris, cols = largest_component(verts, tris, cols)
        box_min = aabb[:3]
        box_size = aabb[3:].max() - aabb[:3].min()                               # the reference's re-normalisation (:385-387)
        verts = verts / float(reso) * box_size + box_min
        verts, vn = self._refine_and_normals(triplane_feat, aabb, verts, tris, reso, box_size, refine, refine_max_move, normals)
        export_obj(os.path.join(save_dir, name), verts, tris, cols, **({"normals": vn} if vn is not None else {}))
        return (verts, tris, cols, vn) if return_normals else (verts, tris, cols)

    @torch.no_grad()
    def decode_texmesh(self, save_dir, triplane_feat, reso, n_faces=10000, texture_reso=2048, only_largest_cc=True, save_voxel=True,
                       mtl_path=None, file_format="obj", decimation="cluster", refine=0, refine_max_move=0.5, normals=None,
                       normal_map=None, normal_map_project=0, normal_map_max_move=1.0, sparse=None, sparse_dilate=0):
        """Reference :362-473 for data_type sdftex: decode_grid -> voxel.npz -> iso-surface -> largest component -> the re-normalisation
        of decode_mesh -> decimation to n_faces (isosurface.simplify_mesh) -> UV atlas at texture_reso and ONE decode_batch call over
        its covered texels, quantised and dilated on the device (isosurface.bake_texture) -> object.obj + object.mtl + object.png, or
        object.glb.  Decimation and atlas are an own design; n_surf_pc and save_highres_mesh are not built.
        decimation: "cluster" (vertex clustering, isosurface.simplify_mesh) or "quadric" (quadric-error edge collapse,
        isosurface.simplify_mesh_quadric, the kind of decimation the reference asks open3d for).
        data_type sdf (:392-397): sdfgrid_r{reso}.npz (`sdf_grid`) and the decimated mesh_r{reso}_simple.obj, no atlas, no texture.
        data_type sdfpbr (:459-471): ONE bake of all 8 channels, split into albedo [..., :3], metallic [..., 3], roughness [..., 4]
        and normal [..., 5:] -> object.obj + object.mtl + textures/{albedo,metallic,roughness,normal}.png (export_pbr_obj), or
        object.glb with one metallic-roughness material (export_pbr_glb).
        refine=K > 0 projects the DECIMATED vertices onto the decoded zero level set (_refine_and_normals) before the atlas, so the
        texel positions are taken on the refined mesh; normals="field" writes the field's unit normals (`vn`, or NORMAL in the GLB)
        and returns them as "normals".
        normal_map="field" (not for data_type sdf) bakes the decoded field's normals on the final mesh into a
        tangent-space map on the same atlas (isosurface.bake_normal_map): the detail the decimation removed, kept for shading.  The
        gradient is net.sdf_and_grad at the texel positions; normal_map_project=K > 0 first projects those positions onto the zero
        level set in K Newton steps (step and total move at most normal_map_max_move cells of the decode grid per axis) and takes
        the gradient there — the colour bake keeps its on-face positions.  Base normals: those of normals="field" when asked for,
        else the area-weighted vertex normals; they are always written then (a tangent-space map means nothing without them).
        sdftex: object_normal.png + a `map_Bump` line, or normalTexture and TANGENT in the GLB; sdfpbr: the baked map takes the
        place of the normal head's image.  Returned as "normal_map" [T,T,3] and "normal_status" [T,T].
        sparse=4 | 8 | 16 (+ sparse_dilate): the narrow-band front end of decode_mesh; not for data_type sdf, whose
        sdfgrid_r{reso}.npz is the dense grid itself.
        With the defaults every file is what it always was.
        Returns a dict of what was written (verts, tris, info, and with a texture uvs, image, mask, gb_pos, corner0), or None for
        an empty iso-surface (no mesh file is written then)."""
        import warnings
        from . import isosurface as iso
        if file_format not in ("obj", "glb"):
            raise NotImplementedError(f"file_format {file_format!r}: 'obj' or 'glb'")
        if decimation not in ("cluster", "quadric"):
            raise ValueError(f"decimation {decimation!r}: expected 'cluster' or 'quadric'")
        if normal_map not in (None, "field"):
            raise ValueError(f"normal_map {normal_map!r}: expected 'field' (or None)")
        if normal_map is not None:
            if self.data_type == "sdf":
                raise ValueError("normal_map='field' needs a texture atlas: data_type sdf writes none")
            normal_map_project = int(normal_map_project)
            if normal_map_project < 0 or not normal_map_max_move > 0:
                raise ValueError(f"normal_map_project={normal_map_project}, normal_map_max_move={normal_map_max_move}: expected a number "
                                 f"of steps >= 0 and a positive move")
        H, W = triplane_feat[0].shape[-2:]
        D = triplane_feat[1].shape[-1]
        aabb = self._resize_aabb((H, W, D))
        os.makedirs(save_dir, exist_ok=True)
        if sparse is not None:
            if self.data_type == "sdf":
                raise NotImplementedError("decode_texmesh(sparse=...): data_type sdf writes the dense sdfgrid_r{reso}.npz; use decode_mesh")
            verts, tris, _, occ = self._sparse_isosurface(triplane_feat, aabb, reso, sparse, sparse_dilate, 0, save_voxel)
            if save_voxel:
                np.savez_compressed(os.path.join(save_dir, "voxel.npz"), vox_grid=occ.bool().cpu().numpy())
        else:
            grid = self.decode_grid(triplane_feat, reso, aabb=aabb)
            if save_voxel:
                np.savez_compressed(os.path.join(save_dir, "voxel.npz"), vox_grid=(grid[..., 0] < 0).cpu().numpy())
            if self.data_type == "sdf":
                np.savez_compressed(os.path.join(save_dir, f"sdfgrid_r{reso}.npz"), sdf_grid=grid[..., 0].cpu().numpy())
            verts, tris, _ = iso.marching_cubes(grid, 0.0, 1.0)
        if only_largest_cc:
            verts, tris, _ = iso.largest_component(verts, tris)
        if tris.shape[0] == 0:
            warnings.warn(f"decode_texmesh: the decoded SDF has no zero level set at reso {reso}; no mesh written to {save_dir}")
            return None
        box_min = aabb[:3]
        box_size = aabb[3:].max() - aabb[:3].min()
        verts = verts / float(reso) * box_size + box_min
        verts, tris, info = (iso.simplify_mesh_quadric if decimation == "quadric" else iso.simplify_mesh)(verts, tris, n_faces)
        verts, vn = self._refine_and_normals(triplane_feat, aabb, verts, tris, reso, box_size, refine, refine_max_move, normals)
        nk = {"normals": vn} if vn is not None else {}
        if self.data_type == "sdf":
            iso.export_obj(os.path.join(save_dir, f"mesh_r{reso}_simple.obj"), verts, tris, **nk)
            return {"verts": verts, "tris": tris, "info": info, **nk}
        image, mask, gb_pos, uvs, corner0 = iso.bake_texture(
            verts, tris, texture_reso, lambda p: self.decode_batch(triplane_feat, p, aabb=aabb)[..., 1:])
        nm, glb_nm, obj_nm = {}, {}, {}
        if normal_map is not None:
            nk, nmap, nstat, tang = self._bake_field_normal_map(triplane_feat, aabb, verts, tris, texture_reso, reso, box_size, vn,
                                                                normal_map_project, normal_map_max_move)
            nm = {"normal_map": nmap, "normal_status": nstat}
            glb_nm, obj_nm = {"tangents": tang}, {"normal_map": nmap}
        if self.data_type == "sdfpbr":
            maps = iso.split_pbr_image(image)
            if normal_map is not None:
                maps = maps[:3] + (nmap,)
            if file_format == "obj":
                iso.export_pbr_obj(os.path.join(save_dir, "object.obj"), verts, tris, uvs, *maps, **nk)
            else:
                iso.export_pbr_glb(os.path.join(save_dir, "object.glb"), verts, tris, uvs, *maps, **nk, **glb_nm)
        elif file_format == "obj":
            mtl_str = iso.read_material_params_from_mtl(mtl_path) if mtl_path is not None else None
            iso.export_textured_obj(os.path.join(save_dir, "object.obj"), verts, tris, uvs, image, material=self.material, mtl_str=mtl_str,
                                    **nk, **obj_nm)
        else:
            iso.export_glb(os.path.join(save_dir, "object.glb"), verts, tris, uvs, image, **nk, **obj_nm, **glb_nm)
        return {"verts": verts, "tris": tris, "uvs": uvs, "image": image, "mask": mask, "gb_pos": gb_pos, "corner0": corner0, "info": info,
                **nk, **nm}

    def _bake_field_normal_map(self, triplane_feat, aabb, verts, tris, texture_reso, reso, box_size, vn, project, max_move):
        """decode_texmesh(normal_map="field"): ({"normals": base normals [V,3]}, map uint8 [T,T,3], status uint8 [T,T], face
        tangents [F,2,3]).  The base normals are `vn` (normals="field") when given, else the area-weighted vertex normals."""
        from . import isosurface as iso
        from ..rendering.rasterizer import vertex_normals
        self.net.eval()
        base = vn if vn is not None else vertex_normals(verts, tris)
        limit = float(max_move) * float(box_size) / float(reso)
        if project > 0:
            def grad_fn(p):
                return self.net.project_to_surface(p, triplane_feat, aabb=aabb, iters=project, max_step=limit, max_move=limit)[2]
        else:
            def grad_fn(p):
                return self.net.sdf_and_grad(p, triplane_feat, aabb=aabb)[1]
        nmap, nstat, tang = iso.bake_normal_map(verts, tris, texture_reso, grad_fn, base_normals=base)
        return {"normals": base}, nmap, nstat, tang

    # ------------------------------------------------------------------ training (reference :51-139, 178-258)
    def _load_data(self, path, sdf_renorm=False):
        """The preprocessed .npz of one shape: grid + near-surface samples (reference :51-112).  data_type sdf has no tex_*
        arrays and a 1-channel volume; sdfpbr has 8 material channels."""
        self._build_tier()
        data = np.load(path)
        has_tex = self.data_type != "sdf"
        dev = self.device
        self.aabb = torch.from_numpy(data["aabb"]).float().to(dev)
        self.sdf_threshold = float(data["threshold"])
        self.material = {"Ka": data["Ka"].tolist() if "Ka" in data else [0, 0, 0], "Kd": data["Kd"].tolist() if "Kd" in data else [1, 1, 1],
                         "Ks": data["Ks"].tolist() if "Ks" in data else [0.4, 0.4, 0.4], "Ns": data["Ns"].tolist() if "Ns" in data else 10}
        pts_grid, sdf_grid = data["pts_grid"], data["sdf_grid"]
        tex_grid = data["tex_grid"] if has_tex else None
        fs = (torch.tensor(pts_grid.shape[:3]).float() * (self.fm_reso / max(pts_grid.shape[:3]))).long().tolist()
        self.featmap_size = [int(x // 2 * 2) for x in fs]
        grid = np.concatenate([sdf_grid[np.newaxis], tex_grid.transpose(3, 0, 1, 2)], axis=0) if has_tex else sdf_grid[np.newaxis]
        grid = torch.from_numpy(grid).float().to(dev)
        want = [x * 2 for x in self.featmap_size]
        if list(grid.shape[1:]) != want:
            grid = F.interpolate(grid.unsqueeze(0), size=want, mode="trilinear", align_corners=False).squeeze(0)
        self.input_grid = grid.unsqueeze(0).contiguous()                                     # [1, C, 2H, 2W, 2D]
        thr = self.sdf_threshold
        self.pts_grid = torch.from_numpy(pts_grid).float().to(dev).view(-1, 3)
        self.sdf_grid = torch.from_numpy(sdf_grid).float().to(dev).view(-1, 1).clamp_(-thr, thr)
        self.pts_near_surf = torch.from_numpy(data["pts_near_surf"]).float().to(dev).view(-1, 3)
        self.sdf_near_surf = torch.from_numpy(data["sdf_near_surf"]).float().to(dev).view(-1, 1).clamp_(-thr, thr)
        if has_tex:
            tc = tex_grid.shape[-1]
            if tc != self.net.cfg[5]:
                raise ValueError(f"{path}: tex_grid has {tc} channels, --data_type {self.data_type} takes {self.net.cfg[5]}")
            self.tex_grid = torch.from_numpy(tex_grid).float().to(dev).view(-1, tc)
            self.tex_near_surf = torch.from_numpy(data["tex_near_surf"]).float().to(dev).view(-1, tc)
        if has_tex and "pts_on_surf" in data:
            self.pts_on_surf = torch.from_numpy(data["pts_on_surf"]).float().to(dev).view(-1, 3)
            self.tex_on_surf = torch.from_numpy(data["tex_on_surf"]).float().to(dev).view(-1, tc)
        if sdf_renorm:
            self.sdf_grid = self.sdf_grid / thr
            self.sdf_near_surf = self.sdf_near_surf / thr

    def _build_tier(self):
        """the network's s3d_ae_* tier; the PBR network with texture (three material heads) is named explicitly"""
        if self.net.variant == 2:
            self.net.build_training_tier(material_heads=True)
        else:
            self.net.build_training_tier()

    def _sample_batch(self, batch_size):
        """vol_ratio of the batch from the regular grid, the rest near the surface (reference :114-127)."""
        n_grid = int(batch_size * self.vol_ratio)
        gi = torch.randint(0, self.pts_grid.shape[0], (n_grid,), device=self.device)
        si = torch.randint(0, self.pts_near_surf.shape[0], (batch_size - n_grid,), device=self.device)
        batch = {"pts": torch.cat([self.pts_grid[gi], self.pts_near_surf[si]], dim=0),
                 "sdf": torch.cat([self.sdf_grid[gi], self.sdf_near_surf[si]], dim=0)}
        if self.data_type != "sdf":
            batch["tex"] = torch.cat([self.tex_grid[gi], self.tex_near_surf[si]], dim=0)
        return batch

    def _loss_cfg(self):
        return ae_loss_cfg(self.sdf_loss_type, self.tex_loss_type, self.sdf_threshold, self.tex_threshold_ratio, self.tex_weight,
                           bool(self.sdf_renorm))

    def _set_optimizer(self, lr, min_lr_ratio=0.01):
        """AdamW with the geo group at lr*lr_split + ExponentialLR reaching min_lr_ratio after n_iters (reference :129-139)."""
        self.optimizer = FlatGroupAdamW(self.net, lr, self.lr_split, lr_decay=min_lr_ratio ** (1 / self.n_iters))

    def train_step(self, data):
        """_forward_batch + update_network (reference :178-237) -> device scalars {"sdf_loss"} (sdf), {"sdf_loss", "tex_loss"}
        (sdftex) or {"sdf_loss", "rgb_loss", "mr_loss", "normal_loss"} (sdfpbr)."""
        losses, _, grads = self.net.loss_and_grads(self.input_grid, data["pts"], data["sdf"], data.get("tex"), self._loss_cfg(),
                                                   aabb=self.aabb, grad_out=getattr(self, "_grad", None))
        self._grad = grads
        self.optimizer.step(grads)
        return {k: losses[i] for i, k in enumerate(self.net.loss_names)}

    def train(self, data_path, log_every=100):
        self._load_data(data_path, sdf_renorm=bool(self.sdf_renorm))
        self.net.reset_aabb(self.aabb)
        self._set_optimizer(self.init_lr, self.min_lr_ratio)
        os.makedirs(self.log_dir, exist_ok=True)
        for i in range(self.n_iters):
            self.step = i
            losses = self.train_step(self._sample_batch(self.batch_size))
            if log_every and (i % log_every == 0 or i == self.n_iters - 1):
                vals = {k: float(v) for k, v in losses.items()}
                print(f"[ae {i}/{self.n_iters}] " + " ".join(f"{k} {v:.5f}" for k, v in vals.items()), flush=True)
                with open(os.path.join(self.log_dir, "progress.jsonl"), "a") as f:
                    f.write(json.dumps({"step": i, **vals}) + "\n")
        stat = self.evaluate()
        with open(os.path.join(self.log_dir, "eval_stat.json"), "w") as f:
            json.dump(stat, f, indent=2)
        self.save_ckpt("final")

    @torch.no_grad()
    def evaluate(self):
        """tsdf statistics over the regular grid (reference :273-296, 491-515)."""
        fm = self.encode()
        pred = self.decode_batch(fm, self.pts_grid)[..., :1]
        gt = self.sdf_grid
        if self.sdf_renorm:
            pred, gt = pred * self.sdf_threshold, gt * self.sdf_threshold
        l1 = (pred - gt).abs()
        stat = {"mean_tsdf_l1_error": l1.mean().item(), "mean_tsdf_rel_error": (l1 / gt.abs()).mean().item(),
                "mean_tsdf_acc": (pred * gt >= 0).float().mean().item()}
        if hasattr(self, "pts_on_surf"):
            tex = self.decode_batch(fm, self.pts_on_surf)[..., 1:]
            stat["surf_tex_l1_error"] = (tex - self.tex_on_surf).abs().mean().item()
        return stat

    @torch.no_grad()
    def encode(self, vol=None):
        """reference :309-317"""
        self._build_tier()
        return self.net.encode(self.input_grid if vol is None else vol)

    def save_ckpt(self, name):
        """reference :141-156 (the optimizer entry holds this implementation's flat Adam state)."""
        os.makedirs(self.log_dir, exist_ok=True)
        sd = {k: v.detach().cpu().clone() for k, v in self.net.state_dict().items()}
        torch.save({"net": sd, "optimizer": self.optimizer.state_dict() if hasattr(self, "optimizer") else None, "scheduler": None,
                    **self.material, "aabb": self.aabb.tolist(), "featmap_size": self.featmap_size},
                   os.path.join(self.log_dir, f"ckpt_{name}.pth"))
