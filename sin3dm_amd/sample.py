"""Sampling CLI with the reference's flags and on-disk layout (src/sample.py):

    python -m sin3dm_amd.sample --tag EXP --n_samples N [--use_ddim True --timestep_respacing 100] [--resize a b c] [--vox]
    python -m torch.distributed.run --nproc-per-node 8 -m sin3dm_amd.sample --tag EXP --n_samples 64 ...
    S3D_SAMPLER=dpmpp2m python -m sin3dm_amd.sample --tag EXP --n_samples N --timestep_respacing logsnr20

S3D_SAMPLER=dpmpp1 | dpmpp2m | dpmpp2m_sde samples with the DPM-Solver++ multistep update instead of DDPM / DDIM: the
same number of model evaluations as --timestep_respacing keeps steps, second order with dpmpp2m; logsnrN spaces the steps evenly in
logSNR (it may keep fewer than N: the count is printed).  edit.py reads it as well (not with --resample > 1).

Reads EXP/encoding/{args.json,feat.npz}, EXP/diffusion/{args.json,ema_<rate>_<iters>.pt} and the AE checkpoint
EXP/encoding/ckpt_final.pth written by the reference's train.py; writes EXP/<output>/NNN/feat.npz (and
r<reso>_voxel.npz with --vox).  Multi-GPU: sample indices are striped over the ranks (sin3dm_amd/parallel.py).
Without --vox the decode stage extracts the iso-surface on the device (marching cubes) and writes a vertex-coloured
object.obj.  The reference's default output, a decimated and textured mesh, is opt-in:

    S3D_MESH=textured python -m sin3dm_amd.sample --tag EXP --n_samples N [--n_faces 10000 --texreso 2048 --file_format obj|glb --copy_mtl]

writes object.obj + object.mtl + object.png (or object.glb) by this project's own decimation and atlas.
S3D_DECIMATE=quadric beside it decimates by quadric-error edge collapse instead of vertex clustering (the default, `cluster`).
An experiment of --data_type sdfpbr writes object.obj + object.mtl + textures/{albedo,metallic,roughness,normal}.png (or a
metallic-roughness object.glb) there, one of --data_type sdf writes sdfgrid_r<reso>.npz + mesh_r<reso>_simple.obj; in the default mode
they write object.obj coloured by the albedo / without colours.  The data type comes from EXP/encoding/args.json.
S3D_MESH_REFINE=K (default 0) projects the exported vertices onto the decoded zero level set in K Newton steps, and
S3D_MESH_NORMALS=field writes the field's unit normals into the mesh files; edit.py reads both as well.
S3D_MESH_NORMAL_MAP=field beside S3D_MESH=textured bakes the field's normals on the decimated mesh into a tangent-space normal map
(object_normal.png, textures/normal.png for sdfpbr, normalTexture in a GLB), S3D_MESH_NORMAL_MAP_PROJECT=K takes them
at the texel positions projected onto the zero level set in K Newton steps; edit.py reads both as well.
S3D_MESH_SPARSE=B (4, 8 or 16) extracts the iso-surface from the bricks of B^3 grid vertices the surface crosses instead of the dense
decode grid: the same mesh files wherever the largest component is seen by the brick lattice, a fraction of the decoder
evaluations, and no 893^3 ceiling (--reso 1024 works); edit.py reads it as well.
S3D_RENDER=views beside any of these also writes renderings/000.png ... 007.png into every sample folder that gets a mesh: the
reference's eight views, drawn on the device from the arrays the export holds (sin3dm_amd/rendering).
S3D_RENDER_SHADING=smooth or pbr beside it draws them with smooth normals and the three-light GGX model of DESIGN.md §24 (pbr: the
metallic, roughness and normal channels of an sdfpbr sample's bake included, and the map of S3D_MESH_NORMAL_MAP=field for either
data type); unset: the flat shader, as before.
S3D_RENDER_SHADOWS=1 beside S3D_RENDER=views draws them with the hard shadows of DESIGN.md §29 (render_views(shadows=True): the light
model of §24, on flat normals unless S3D_RENDER_SHADING says otherwise); edit.py reads it as well.
"""
from __future__ import annotations

import os

import torch

from . import parallel
from .utils import dist_util
from .utils.parser_util import (diffusion_model_path, encoding_feat_path, encoding_log_dir, sample_args)


def noise_source(noise=None):
    """"device" (the device's Philox generators, the default) or "torch_cpu" (torch's CPU stream generated on the device,
    diffusion/cpu_stream.py: sample i is what the reference writes for --n_samples 1 after torch.manual_seed of its seed).
    noise=None reads the environment variable S3D_NOISE."""
    name = noise if noise is not None else (os.environ.get("S3D_NOISE") or "device")
    if name not in ("device", "torch_cpu"):
        raise ValueError(f"noise source {name!r}: expected 'device' or 'torch_cpu'")
    return name


def sampler_choice(name=None):
    """"" (the default: DDPM, or DDIM with --use_ddim, as ever) or a few-step sampler of diffusion.gaussian_diffusion.MULTISTEP_SAMPLERS:
    "dpmpp1", "dpmpp2m" or "dpmpp2m_sde" (DPM-Solver++ multistep; --use_ddim is then not looked at, and
    --timestep_respacing logsnrN is the spacing they are meant for).  name=None reads the environment variable S3D_SAMPLER."""
    from .diffusion.gaussian_diffusion import MULTISTEP_SAMPLERS
    name = name if name is not None else (os.environ.get("S3D_SAMPLER") or "")
    if name != "" and name not in MULTISTEP_SAMPLERS:
        raise ValueError(f"sampler {name!r}: expected one of {', '.join(sorted(MULTISTEP_SAMPLERS))} (or unset)")
    return name


def mesh_mode(mode=None):
    """"vertex" (the vertex-coloured object.obj of decode_mesh, the default) or "textured" (decode_texmesh: --n_faces, --texreso,
    --file_format and --copy_mtl apply).  mode=None reads the environment variable S3D_MESH."""
    name = mode if mode is not None else (os.environ.get("S3D_MESH") or "vertex")
    if name not in ("vertex", "textured"):
        raise ValueError(f"mesh mode {name!r}: expected 'vertex' or 'textured'")
    return name


def decimation_mode(mode=None):
    """"cluster" (vertex clustering, isosurface.simplify_mesh, the default) or "quadric" (quadric-error edge collapse,
    isosurface.simplify_mesh_quadric): how the textured export cuts the iso-surface to --n_faces.  mode=None reads the
    environment variable S3D_DECIMATE."""
    name = mode if mode is not None else (os.environ.get("S3D_DECIMATE") or "cluster")
    if name not in ("cluster", "quadric"):
        raise ValueError(f"decimation {name!r}: expected 'cluster' or 'quadric'")
    return name


def render_mode(mode=None):
    """"" (off, the default) or "views": every sample folder that gets a mesh also gets renderings/000.png ... 007.png, the
    reference's eight views drawn by the device rasteriser (sin3dm_amd/rendering) from the arrays the export
    already holds on the device.  mode=None reads the environment variable S3D_RENDER."""
    name = mode if mode is not None else (os.environ.get("S3D_RENDER") or "")
    if name not in ("", "views"):
        raise ValueError(f"render mode {name!r}: expected 'views' (or unset)")
    return name


def mesh_refine(value=None):
    """K >= 0 (default 0): Newton steps of the exported mesh's vertices onto the decoded zero level set (decode_mesh /
    decode_texmesh refine=K).  value=None reads the environment variable S3D_MESH_REFINE."""
    raw = value if value is not None else (os.environ.get("S3D_MESH_REFINE") or "0")
    try:
        k = int(raw)
    except (TypeError, ValueError):
        k = -1
    if k < 0:
        raise ValueError(f"mesh refine {raw!r}: expected a number of steps >= 0")
    return k


def mesh_normals(mode=None):
    """"" (the default: no normals in the mesh files) or "field": the decoded field's unit gradient at every vertex, written as
    `vn` lines or the GLB's NORMAL (normals="field").  mode=None reads the environment variable S3D_MESH_NORMALS."""
    name = mode if mode is not None else (os.environ.get("S3D_MESH_NORMALS") or "")
    if name not in ("", "field"):
        raise ValueError(f"mesh normals {name!r}: expected 'field' (or unset)")
    return name


def mesh_normal_map(mode=None):
    """"" (the default: no baked normal map) or "field": decode_texmesh(normal_map="field"), DESIGN.md §27.  mode=None reads the
    environment variable S3D_MESH_NORMAL_MAP."""
    name = mode if mode is not None else (os.environ.get("S3D_MESH_NORMAL_MAP") or "")
    if name not in ("", "field"):
        raise ValueError(f"mesh normal map {name!r}: expected 'field' (or unset)")
    return name


def mesh_normal_map_project(value=None):
    """K >= 0 (default 0): Newton steps of the texel positions onto the zero level set before the gradient of the baked normal
    map is taken (decode_texmesh normal_map_project=K).  value=None reads the environment variable S3D_MESH_NORMAL_MAP_PROJECT."""
    raw = value if value is not None else (os.environ.get("S3D_MESH_NORMAL_MAP_PROJECT") or "0")
    try:
        k = int(raw)
    except (TypeError, ValueError):
        k = -1
    if k < 0:
        raise ValueError(f"mesh normal map project {raw!r}: expected a number of steps >= 0")
    return k


def mesh_sparse(value=None):
    """0 (the default: the dense decode grid) or a brick size of 4, 8 or 16: the narrow-band iso-surface of decode_mesh /
    decode_texmesh sparse=B, which decodes only the bricks the surface crosses and has no 893^3 ceiling.
    value=None reads the environment variable S3D_MESH_SPARSE."""
    raw = value if value is not None else (os.environ.get("S3D_MESH_SPARSE") or "0")
    try:
        b = int(raw)
    except (TypeError, ValueError):
        b = -1
    if b not in (0, 4, 8, 16):
        raise ValueError(f"mesh sparse {raw!r}: expected a brick size of 4, 8 or 16 (or unset)")
    return b


def render_shading(mode=None):
    """"" (the default: the flat shader the views always had), "flat", "smooth" or "pbr": the shading of the S3D_RENDER=views
    renders (rendering/rasterizer.render_views).  mode=None reads the environment variable S3D_RENDER_SHADING."""
    name = mode if mode is not None else (os.environ.get("S3D_RENDER_SHADING") or "")
    if name not in ("", "flat", "smooth", "pbr"):
        raise ValueError(f"render shading {name!r}: expected 'flat', 'smooth' or 'pbr' (or unset)")
    return name


def render_shadows(value=None):
    """False (the default) or True: the S3D_RENDER=views renders with shadows (render_views(shadows=True)).
    value=None reads the environment variable S3D_RENDER_SHADOWS ("1" or "0" / unset)."""
    raw = value if value is not None else (os.environ.get("S3D_RENDER_SHADOWS") or "0")
    if raw in (True, False):
        return bool(raw)
    if str(raw) not in ("0", "1"):
        raise ValueError(f"render shadows {raw!r}: expected '1' (or '0' / unset)")
    return str(raw) == "1"


def render_sample(save_dir, mesh, shading=None, shadows=None):
    """renderings/ beside a decoded mesh.  mesh: what decode_mesh (verts, tris, colours) or decode_texmesh (a dict, or None for an
    empty iso-surface) returned.  shading: see render_shading; with "pbr" the 8-channel bake of an sdfpbr sample is used as it
    lies on the device (albedo [..., :3], metallic [..., 3], roughness [..., 4], normal [..., 5:]); a baked "normal_map" in the dict
    (decode_texmesh normal_map="field") is the material's normal_image under "pbr", for an sdftex sample too.  Field normals in the mesh (a
    dict's "normals", a fourth tuple entry) are passed on to render_views, which uses them under "smooth" and "pbr".  shadows: see
    render_shadows.  Returns the paths written."""
    from .rendering.rasterizer import render_views
    from .rendering.render_multiview import write_views
    shading = render_shading(shading)
    shadows = render_shadows(shadows)
    if mesh is None:
        return []
    if isinstance(mesh, dict):
        verts, tris, kw = mesh["verts"], mesh["tris"], {}
        vn = mesh.get("normals")
        if mesh.get("image") is not None and shading == "pbr" and mesh["image"].shape[-1] == 8:
            img = mesh["image"].flip(0)                         # (texel row 0 first: see below)
            kw = dict(uvs=mesh["uvs"].reshape(-1, 3, 2), materials=[{"Kd": (1.0, 1.0, 1.0), "image": img[..., :3], "metallic_image": img[..., 3],
                                                                     "roughness_image": img[..., 4], "normal_image": img[..., 5:8]}])
        elif mesh.get("image") is not None:
            # the baked image has texel row 0 first, which the PNG shows as its bottom row: the rasteriser reads top row first
            kw = dict(uvs=mesh["uvs"].reshape(-1, 3, 2), materials=[{"Kd": (1.0, 1.0, 1.0), "image": mesh["image"][..., :3].flip(0)}])
        if kw and shading == "pbr" and mesh.get("normal_map") is not None:
            kw["materials"][0]["normal_image"] = mesh["normal_map"].flip(0)
    else:
        verts, tris, cols = mesh[:3]
        vn = mesh[3] if len(mesh) > 3 else None
        coloured = cols is not None and cols.dim() == 2 and cols.shape[1] >= 3           # (an sdf experiment decodes no colour)
        kw = dict(vertex_colors=cols[:, :3].clamp(0, 1)) if coloured else {}
    if tris.shape[0] == 0:
        return []
    if shading not in ("", "flat"):                             # (unset: the call stays the one it always was)
        kw["shading"] = shading
        if vn is not None:
            kw["normals"] = vn
    if shadows:                                                 # (unset: no such argument in the call)
        kw["shadows"] = True
    images = render_views(verts, tris, **kw)
    return write_views(images.cpu().numpy(), os.path.join(save_dir, "renderings"))


def find_copy_mtl(args):
    """--copy_mtl: the first mesh/*.mtl beside args.data_path (reference: src/sample.py:70-76), or None."""
    import glob
    if not getattr(args, "copy_mtl", False) or not getattr(args, "data_path", None):
        return None
    found = sorted(glob.glob(os.path.join(os.path.dirname(args.data_path), "mesh", "*.mtl")))
    return found[0] if found else None


def sample_generators(groups, device, base_seed=1000, noise=None):
    """One generator per sample of every batch in `groups` (lists of sample indices), seeded parallel.sample_seed(base_seed, i)."""
    if noise_source(noise) == "torch_cpu":
        from .diffusion.cpu_stream import TorchCpuStream
        return [[TorchCpuStream(parallel.sample_seed(base_seed, i), device=device) for i in idx] for idx in groups]
    return [[torch.Generator(device=device).manual_seed(parallel.sample_seed(base_seed, i)) for i in idx] for idx in groups]


def sample_diffusion(args, rank=0, world=1, base_seed=1000, noise=None, hwd=None, loop_kw=None):
    """Reference: src/sample.py:6-48, with per-sample seeds and rank striping.  noise: see noise_source.
    hwd / loop_kw (sin3dm_amd.edit): the canvas when it is not the --resize one, and further keywords of the sampling loops
    (known=, resample=)."""
    from .diffusion.script_util import create_model_and_diffusion_from_args
    from .utils.triplane_util import decompose_featmaps, load_triplane_data, save_triplane_data

    dev = dist_util.dev()
    src_data, sizes = load_triplane_data(encoding_feat_path(args.tag), device=dev)
    model, diffusion = create_model_and_diffusion_from_args(args)
    model.load_state_dict(dist_util.load_state_dict(diffusion_model_path(args.tag, args.ema_rate, args.diff_n_iters),
                                                    map_location="cpu"))
    model.to(dev).eval()
    sample_fn = diffusion.ddim_sample_loop if args.use_ddim else diffusion.p_sample_loop
    sampler = sampler_choice()
    chain_kw = {}
    if sampler:                                                # (unset: the calls below are the ones they always were)
        import functools
        from .diffusion.gaussian_diffusion import multistep_sampler
        order, sde = multistep_sampler(sampler)
        sample_fn = functools.partial(diffusion.multistep_sample_loop, order=order, sde=sde)
        chain_kw = {"sampler": sampler}
        if rank == 0:
            print(f"sampler {sampler}: {diffusion.num_timesteps} model evaluations per sample")

    result_dir = os.path.join(args.tag, args.output)
    os.makedirs(result_dir, exist_ok=True)
    C = src_data.shape[0]
    H, W, D = hwd if hwd is not None else (int(s * r) for s, r in zip(sizes, args.resize))
    loop_kw = dict(loop_kw or {})
    if rank == 0:
        print("H, W, D:", H, W, D)

    paths = []
    mine = parallel.shard_indices(args.n_samples, rank, world)
    groups = list(parallel.batches(mine, args.diff_batch_size))
    # x_T and every step's eps of sample i come from ITS generator (seed = base + i): a sample does not depend on the batch it
    # is in, the chain it runs on or the number of GPUs
    gens = sample_generators(groups, dev, base_seed, noise)
    kw = {"H": H, "W": W, "D": D}
    nch = sample_chains(len(groups), args.diff_batch_size)
    full = [g for g in range(len(groups)) if len(groups[g]) == args.diff_batch_size]
    outs = {}
    if nch > 1 and len(full) > 1:
        # several batches of equal shape on this GPU: up to `nch` of them in flight as independent chains (one stream + one
        # workspace lane each) instead of one after the other (src/sample.py:33-47)
        res = diffusion.sample_loop_chains(model, [args.diff_batch_size, C, H + D, W + D], len(full), chains=nch,
                                           ddim=bool(args.use_ddim), generators=[gens[g] for g in full], device=dev, model_kwargs=kw,
                                           **chain_kw, **loop_kw)
        outs = dict(zip(full, res))
    for g, idx in enumerate(groups):
        samples = outs[g] if g in outs else sample_fn(model, [len(idx), C, H + D, W + D], progress=rank == 0, model_kwargs=kw,
                                                      generator=gens[g], **loop_kw)
        xy, xz, yz = (t.detach().cpu().numpy() for t in decompose_featmaps(samples, (H, W, D)))
        for j, i in enumerate(idx):
            path = os.path.join(result_dir, f"{i:03d}", "feat.npz")
            save_triplane_data(path, xy[j], xz[j], yz[j])
            paths.append(path)
    return paths


def sample_chains(n_batches, batch):
    """How many of a rank's batches run at once as independent chains (GaussianDiffusion.sample_loop_chains).  S3D_SAMPLE_CHAINS
    sets it (1 = off).  Default: chains pay where a step's launches are a round or two of blocks each — measured on one MI355X
    at 128^3 (profiles/r05_two_chains.txt) — so three at batch 1, two at batch 2, none from batch 4 on."""
    env = os.environ.get("S3D_SAMPLE_CHAINS")
    if env:
        return max(1, min(int(env), n_batches))
    return max(1, min(3 if batch == 1 else 2 if batch == 2 else 1, n_batches))


def decode(args, paths):
    """Reference: src/sample.py:51-78.  mesh_mode() picks between the vertex-coloured OBJ and the textured export."""
    from .encoding.model import ShapeAutoEncoder
    from .utils.triplane_util import load_triplane_data

    textured = mesh_mode() == "textured"
    # only a choice other than the default is passed on: the default call is the one it always was
    decimate = {"decimation": "quadric"} if decimation_mode() == "quadric" else {}
    field = {}
    if mesh_refine():
        field["refine"] = mesh_refine()
    if mesh_normals():
        field["normals"] = mesh_normals()
    if mesh_sparse():
        field["sparse"] = mesh_sparse()
    baked = {}
    if mesh_normal_map():
        if not textured:
            raise ValueError("S3D_MESH_NORMAL_MAP=field needs S3D_MESH=textured: the vertex-coloured mesh has no atlas")
        baked["normal_map"] = mesh_normal_map()
        if mesh_normal_map_project():
            baked["normal_map_project"] = mesh_normal_map_project()
    ae = ShapeAutoEncoder(encoding_log_dir(args.tag), args, device=dist_util.dev())
    ae.load_ckpt("final")
    views = render_mode() == "views"
    shading = render_shading() if views else None              # (a mistyped value fails here, before the decoding)
    for path in paths:
        fm = [f.unsqueeze(0) for f in load_triplane_data(path, device=dist_util.dev(), compose=False)]
        if args.vox:
            ae.decode_voxel(os.path.dirname(path), fm, args.reso)
            continue
        if textured:
            mesh = ae.decode_texmesh(os.path.dirname(path), fm, args.reso, n_faces=args.n_faces, texture_reso=args.texreso,
                                     mtl_path=find_copy_mtl(args), file_format=args.file_format, **decimate, **field, **baked)
        else:
            # iso-surface on the device, vertex-coloured object.obj
            mesh = ae.decode_mesh(os.path.dirname(path), fm, args.reso, **field, **({"return_normals": True} if "normals" in field else {}))
        if views:
            render_sample(os.path.dirname(path), mesh, shading)


def main(argv=None):
    args = sample_args(argv)
    rank, local, world = parallel.env_rank_world()
    dist_util.setup_dist(local if world > 1 else args.gpu_id)
    parallel.init(device=dist_util.dev())
    paths = sample_diffusion(args, rank, world)
    decode(args, paths)
    all_paths = sorted(p for ps in parallel.gather_objects(paths) for p in ps)
    if rank == 0:
        print(f"wrote {len(all_paths)} samples under {os.path.join(args.tag, args.output)}")
    parallel.shutdown()                              # barrier + destroy_process_group
    return all_paths


if __name__ == "__main__":
    from .launcher import maybe_spawn_module
    rc = maybe_spawn_module("sin3dm_amd.sample")      # S3D_GPUS=N: N fresh ranks, one per GPU (this process touches none)
    if rc is not None:
        raise SystemExit(rc)
    main()
