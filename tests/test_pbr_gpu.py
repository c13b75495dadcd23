"""GPU: PBR and geometry-only assets — the decoder variants against the reference's outputs
(tests/golden/pbr_decoder.npz) and against the float64 restatement pbr_cases.py (itself pinned to that golden by
test_pbr_host.py), the PBR material export, and the sampling CLI on sdf and sdfpbr experiment directories."""
import json
import os
import struct

import numpy as np
import pytest
import torch

import pbr_cases as P
from conftest import golden, relerr
from sin3dm_amd import testing as T

pytestmark = pytest.mark.gpu

TOL_FWD = 1e-4          # the project's bound and measure for this kind of kernel (test_hip_parity.py: test_decoder_golden)


def cu(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32).to("cuda:0")


def make_net(kind, up, hid):
    from sin3dm_amd.encoding.networks import AutoEncoderGroupPBR, AutoEncoderGroupSkip
    if kind == "pbr":
        net = AutoEncoderGroupPBR(4, 8, up, hid, 4, use_tex=True, tex_channels=8)
    elif kind == "geo":
        net = AutoEncoderGroupSkip(4, 8, up, hid, 4, use_tex=False)
    else:
        net = AutoEncoderGroupSkip(4, 8, up, hid, 4, use_tex=True, tex_channels=8 if kind == "skip8" else 3)
    missing, unexpected = net.load_state_dict(T.synthetic_state_dict(P.shapes_of(kind, up, hid), 5), strict=False)
    assert not unexpected and all(k.startswith(("geo_encoder", "tex_encoder", "aabb")) for k in missing)
    return net.to("cuda:0").eval()


def check_clamp_and_empty(net, pts, fm, aabb, width):
    """clamp_color clamps columns >= 1 of the SAME call's values and never the sdf; decoding no points gives an empty tensor"""
    raw = net.decode(pts, fm, aabb=aabb)
    clamped = net.decode(pts, fm, aabb=aabb, clamp_color=True)
    assert torch.equal(clamped[:, 0], raw[:, 0])
    assert torch.equal(clamped[:, 1:], raw[:, 1:].clamp(0, 1))
    empty = net.decode(pts[:0], fm, aabb=aabb)
    assert tuple(empty.shape) == (0, width)
    return raw


@pytest.mark.parametrize("tag", ["small", "wide"])
def test_pbr_decoder_golden(tag):
    g = golden("pbr_decoder")
    up, hid, H, W, D = (int(v) for v in g[f"pbr.{tag}.cfg"])
    fm = [cu(g[f"pbr.{tag}.{p}"]) for p in T.PLANES]
    pts, aabb = cu(g[f"pbr.{tag}.pts"]), torch.from_numpy(g[f"pbr.{tag}.aabb"])
    errs = {}
    # ---- AutoEncoderGroupPBR (variant 2)
    net = make_net("pbr", up, hid)
    out = check_clamp_and_empty(net, pts, fm, aabb, 9)
    assert tuple(out.shape) == (257, 9)
    errs["pbr.out"] = relerr(out.cpu().numpy(), g[f"pbr.{tag}.out"])
    errs["pbr.out_default_aabb"] = relerr(net.decode(pts[:33], fm).cpu().numpy(), g[f"pbr.{tag}.out_default_aabb"])
    mat = out[:, 1:]
    assert 0.3 < float(((mat < 0) | (mat > 1)).float().mean()) < 0.7          # the clamp above had something to do
    for grp in ("geo", "tex0", "tex"):
        for p, f in zip(T.PLANES, net.plane_features(fm, grp)):
            errs[f"pbr.{grp}_{p}"] = relerr(f.cpu().numpy(), g[f"pbr.{tag}.{grp}_{p}"])
    # the geo parameters have the names of variant 0's: the identical network
    skip = make_net("skip", up, hid)
    sdf0 = skip.decode(pts, fm, aabb=aabb)[:, 0]
    assert torch.equal(out[:, 0], sdf0), "sdf_vs_variant0: one point kernel, one geo network, the same bits"
    # ---- geometry only (variant 1), planes of fdim_geo channels
    gfm = [f[:, :4].contiguous() for f in fm]
    gnet = make_net("geo", up, hid)
    gout = check_clamp_and_empty(gnet, pts, gfm, aabb, 1)
    errs["geo.out"] = relerr(gout.cpu().numpy(), g[f"geo.{tag}.out"])
    errs["geo.out_default_aabb"] = relerr(gnet.decode(pts[:33], gfm).cpu().numpy(), g[f"geo.{tag}.out_default_aabb"])
    assert torch.equal(gout[:, 0], sdf0), "geo.sdf_vs_variant0"
    for p, f in zip(T.PLANES, gnet.plane_features(gfm, "geo")):
        errs[f"geo.geo_{p}"] = relerr(f.cpu().numpy(), g[f"pbr.{tag}.geo_{p}"])
    with pytest.raises(AssertionError):
        gnet.plane_features(gfm, "tex")
    with pytest.raises(AssertionError):
        gnet.decode(pts, fm, aabb=aabb)                                        # 12-channel planes are not this net's input
    # ---- the skip net with the 8 sigmoid channels of sdfpbr
    if tag == "small":
        snet = make_net("skip8", up, hid)
        sout = check_clamp_and_empty(snet, pts, fm, aabb, 9)
        errs["skip8.out"] = relerr(sout.cpu().numpy(), g[f"skip8.{tag}.out"])
        errs["skip8.out_default_aabb"] = relerr(snet.decode(pts[:33], fm).cpu().numpy(), g[f"skip8.{tag}.out_default_aabb"])
        assert float(sout[:, 1:].min()) > 0 and float(sout[:, 1:].max()) < 1
    print(tag, {k: f"{v:.2e}" for k, v in errs.items()})
    assert max(errs.values()) < TOL_FWD, errs


GRID = dict(up=64, hid=256, hwd=(20, 12, 16), reso=24, aabb=[-1.0, -0.6, -0.8, 1.0, 0.6, 0.8])


@pytest.fixture(scope="module")
def grid_reference():
    """float64 restatement on the restated cell centres, computed once: {"pbr": [N,9], "geo": [N,1]} and the points"""
    H, W, D = GRID["hwd"]
    fm = P.synthetic_planes(H, W, D)
    pts, res = P.grid_points(GRID["aabb"], GRID["reso"])
    assert res == (24, 14, 19)
    want = {"pbr": P.decode("pbr", P.weights("pbr", GRID["up"], GRID["hid"]), pts, fm, GRID["aabb"]).numpy(),
            "geo": P.decode("geo", P.weights("geo", GRID["up"], GRID["hid"]), pts, [f[:, :4] for f in fm], GRID["aabb"]).numpy()}
    return fm, pts, want


@pytest.mark.parametrize("kind", ["pbr", "geo"])
def test_pbr_grid(grid_reference, kind):
    fm, pts, want = grid_reference
    width = 9 if kind == "pbr" else 1
    net = make_net(kind, GRID["up"], GRID["hid"])
    planes = [cu(f if kind == "pbr" else f[:, :4]) for f in fm]
    aabb = torch.tensor(GRID["aabb"])
    grid = net.decode_grid(planes, GRID["reso"], aabb=aabb)
    assert tuple(grid.shape) == (24, 14, 19, width)
    ref = want[kind].copy()
    ref[:, 1:] = np.clip(ref[:, 1:], 0, 1)                                   # decode_grid clamps the material columns
    e_ref = relerr(grid.reshape(-1, width).cpu().numpy(), ref)
    pts_out = net.decode(cu(pts.numpy()), planes, aabb=aabb, clamp_color=True)
    e_pts = relerr(pts_out.cpu().numpy(), grid.reshape(-1, width).cpu().numpy())
    print(kind, f"grid vs restatement {e_ref:.2e}, grid mode vs point mode {e_pts:.2e}")
    assert e_ref < TOL_FWD
    assert e_pts < 1e-5, "grid mode and point mode must agree"            # (in-kernel coordinates: one ulp from torch's linspace/div)


def head_table_nets(up, hid):
    """Four nets on one set of weights: A the skip net with 3 texture channels, B the same with 8 (every tensor of equal shape and
    rows 0..2 of the last texture layer are A's, rows 3..7 arbitrary), C geometry only and D the PBR net with A's geo parameters."""
    from sin3dm_amd.encoding.networks import AutoEncoderGroupPBR, AutoEncoderGroupSkip
    sd_a = T.synthetic_state_dict(P.shapes_of("skip", up, hid), 5)
    sd_b = T.synthetic_state_dict(P.shapes_of("skip8", up, hid), 9)
    for k, v in sd_a.items():
        if sd_b[k].shape == v.shape:
            sd_b[k] = v.clone()
    last = "tex_decoder.second_layers.4."
    assert sd_b[last + "weight"].shape == (8, hid) and sd_a[last + "weight"].shape == (3, hid)
    for leaf in ("weight", "bias"):
        sd_b[last + leaf][:3] = sd_a[last + leaf]
    geo = {k: v for k, v in sd_a.items() if k.startswith("geo_")}
    sd_c = {k: geo[k].clone() for k in P.shapes_of("geo", up, hid)}
    sd_d = T.synthetic_state_dict(P.shapes_of("pbr", up, hid), 9)
    sd_d.update({k: v.clone() for k, v in geo.items()})
    nets = {"A": AutoEncoderGroupSkip(4, 8, up, hid, 4, use_tex=True, tex_channels=3),
            "B": AutoEncoderGroupSkip(4, 8, up, hid, 4, use_tex=True, tex_channels=8),
            "C": AutoEncoderGroupSkip(4, 8, up, hid, 4, use_tex=False),
            "D": AutoEncoderGroupPBR(4, 8, up, hid, 4, use_tex=True, tex_channels=8)}
    for tag, sd in (("A", sd_a), ("B", sd_b), ("C", sd_c), ("D", sd_d)):
        missing, unexpected = nets[tag].load_state_dict(sd, strict=False)
        assert not unexpected and all(k.startswith(("geo_encoder", "tex_encoder", "aabb")) for k in missing)
        nets[tag].to("cuda:0").eval()
    return nets


# the five compiled (up, hidden) tile pairs and one unpadded width
@pytest.mark.parametrize("up,hid", [(64, 256), (32, 32), (32, 256), (32, 64), (96, 128), (48, 256)])
def test_head_columns_do_not_depend_on_the_other_heads(up, hid):
    """A head's output columns are the same bits whichever other heads or groups its network has: the sdf of the skip net, of the
    geometry-only net and of the PBR net, and the first three texture channels of the skip net with 3 and with 8 of them."""
    nets = head_table_nets(up, hid)
    fm = [cu(f) for f in P.synthetic_planes(6, 5, 4)]
    planes = {"A": fm, "B": fm, "C": [f[:, :4].contiguous() for f in fm], "D": fm}
    aabb = torch.tensor(GRID["aabb"])
    # 130 points: a second block with two live lanes; both lane halves store (B's columns 5..8 come from half 1); some outside
    g = np.random.Generator(np.random.PCG64(17))
    half = np.asarray(GRID["aabb"][3:])
    pts = g.uniform(-1.0, 1.0, size=(130, 3)) * half
    axis = np.asarray([0, 1, 2, 0, 1, 2])
    pts[[0, 31, 64, 127, 128, 129], axis] = np.asarray([1.3, -1.2, 1.5, -1.1, 1.25, -1.4]) * half[axis]      # the border clamp acts
    assert int((np.abs(pts) > half).any(axis=1).sum()) == 6
    pts = cu(pts)
    modes = {"decode": lambda n, f: n.decode(pts, f, aabb=aabb),
             "decode, clamp_color": lambda n, f: n.decode(pts, f, aabb=aabb, clamp_color=True),
             "decode_grid": lambda n, f: n.decode_grid(f, 9, aabb=aabb)}            # dims (9, 5, 7): three blocks, the last partial
    for mode, run in modes.items():
        out = {tag: run(net, planes[tag]) for tag, net in nets.items()}
        if mode == "decode_grid":
            assert tuple(out["A"].shape) == (9, 5, 7, 4)
            out = {tag: o.reshape(315, -1) for tag, o in out.items()}
        assert [o.shape[1] for o in out.values()] == [4, 9, 1, 9] and bool(torch.isfinite(out["A"]).all())
        assert float(out["A"][:, 0].std()) > 0 and float(out["A"][:, 1:].std()) > 0
        assert torch.equal(out["B"][:, :4], out["A"]), mode
        assert torch.equal(out["C"][:, 0], out["A"][:, 0]), mode
        assert torch.equal(out["D"][:, 0], out["A"][:, 0]), mode


def test_prepare_cache_and_retarget(monkeypatch):
    from sin3dm_amd import _lib
    up, hid = 16, 32
    net = make_net("pbr", up, hid)
    sd = P.weights("pbr", up, hid)
    lib = _lib.load()
    calls = []
    real = lib.s3d_decoder_prepare_triplane
    monkeypatch.setattr(lib, "s3d_decoder_prepare_triplane", lambda *a: (calls.append(a[4:7]), real(*a))[1], raising=False)
    g = np.random.Generator(np.random.PCG64(11))
    for n, (H, W, D) in enumerate(((10, 14, 6), (7, 9, 13))):                # the second: another size -> re-prepare
        fm = P.synthetic_planes(H, W, D, seed=60 + n)
        planes = [cu(f) for f in fm]
        pts = (g.uniform(-1.1, 1.1, size=(300, 3)) * np.asarray(P.AABB[3:])).astype(np.float32)
        a = net.decode(cu(pts), planes, aabb=torch.tensor(P.AABB))
        assert len(calls) == n + 1 and tuple(calls[-1]) == (H, W, D)
        b = net.decode(cu(pts[:77]), planes, aabb=torch.tensor(P.AABB))
        net.decode_grid(planes, 8, aabb=torch.tensor(P.AABB))
        assert len(calls) == n + 1, "a second decode on the same triplane re-ran the plane stage"
        assert torch.equal(a[:77], b)
        want = P.decode("pbr", sd, pts, fm, P.AABB).numpy()
        assert relerr(a.cpu().numpy(), want) < TOL_FWD
    planes[0].mul_(0.5)                                                      # same storage, new contents
    c = net.decode(cu(pts), planes, aabb=torch.tensor(P.AABB))
    assert len(calls) == 3
    fm[0] = fm[0] * 0.5
    assert relerr(c.cpu().numpy(), P.decode("pbr", sd, pts, fm, P.AABB).numpy()) < TOL_FWD


# ------------------------------------------------------------------ experiment directories of the other two data types
EXP_AABB = [-0.72, -1.0, -0.72, 0.72, 1.0, 0.72]


def make_experiment(root, data_type, enc_net_type, hwd=(24, 32, 24), mc=64):
    """test_cli_gpu.make_experiment for --data_type sdf / sdfpbr: feat.npz and the UNet have fdim_geo (+ fdim_tex) channels,
    ckpt_final.pth holds the reference's state_dict of that network (encoders and aabb included)."""
    from sin3dm_amd.utils import parser_util as pu
    tag = os.path.join(root, "exp")
    pu.train_args(["--tag", tag, "--data_path", "shape.npz", "--model_channels", str(mc), "--fm_reso", "32",
                   "--data_type", data_type, "--enc_net_type", enc_net_type])
    C = 4 if data_type == "sdf" else 12
    H, W, D = hwd
    np.savez_compressed(pu.encoding_feat_path(tag), feat_xy=np.tanh(T.synthetic_noise((C, H, W), 1)),
                        feat_xz=np.tanh(T.synthetic_noise((C, H, D), 2)), feat_yz=np.tanh(T.synthetic_noise((C, W, D), 3)))
    torch.save(T.synthetic_state_dict(T.unet_param_shapes(in_channels=C, model_channels=mc, out_channels=C), 0),
               pu.diffusion_model_path(tag, 0.9999, 25000))
    if data_type == "sdf":
        shapes = T.geo_only_param_shapes(with_encoder=True)
    elif enc_net_type == "pbr":
        shapes = T.pbr_param_shapes(with_encoder=True)
    else:
        shapes = T.ae_param_shapes(tex_channels=8, with_encoder=True)
    net = T.synthetic_state_dict(shapes, 5)
    net["aabb"] = torch.tensor(EXP_AABB)
    torch.save({"net": net, "aabb": net["aabb"].numpy(), "featmap_size": hwd, "Ka": None, "Kd": None, "Ks": None, "Ns": None},
               os.path.join(pu.encoding_log_dir(tag), "ckpt_final.pth"))
    return tag


def autoencoder(tag):
    from sin3dm_amd.encoding.model import ShapeAutoEncoder
    from sin3dm_amd.utils import parser_util as pu
    args = pu.sample_args(["--tag", tag])
    ae = ShapeAutoEncoder(pu.encoding_log_dir(tag), args, device=torch.device("cuda:0"))
    ae.load_ckpt("final")                                                    # strict load_state_dict(ckpt["net"])
    return ae


def files_under(folder):
    return sorted(os.path.relpath(os.path.join(r, f), folder) for r, _, fs in os.walk(folder) for f in fs)


PBR_OBJ_FILES = ["object.mtl", "object.obj", "textures/albedo.png", "textures/metallic.png", "textures/normal.png", "textures/roughness.png"]


def test_decode_texmesh_pbr(tmp_path):
    from test_texmesh_gpu import decode_png, parse_obj
    from sin3dm_amd.utils import parser_util as pu
    from sin3dm_amd.utils.triplane_util import load_triplane_data
    tag = make_experiment(str(tmp_path), "sdfpbr", "pbr")
    ae = autoencoder(tag)
    assert ae.data_type == "sdfpbr" and type(ae.net).__name__ == "AutoEncoderGroupPBR"
    fm = [f.unsqueeze(0) for f in load_triplane_data(pu.encoding_feat_path(tag), device="cuda:0", compose=False)]
    out_dir = str(tmp_path / "obj")
    out = ae.decode_texmesh(out_dir, fm, 48, n_faces=2000, texture_reso=512)
    assert out is not None and files_under(out_dir) == PBR_OBJ_FILES + ["voxel.npz"]
    aabb = ae._resize_aabb((fm[0].shape[-2], fm[0].shape[-1], fm[1].shape[-1]))
    mask, image = out["mask"], out["image"]
    assert tuple(image.shape) == (512, 512, 8) and 0 < len(out["tris"]) <= 2000 and int(mask.sum()) > 0
    cols = ae.decode_batch(fm, out["gb_pos"][mask], aabb=aabb)[..., 1:]
    assert tuple(cols.shape) == (int(mask.sum()), 8)
    assert torch.equal(image[mask], (cols * 255.0).clamp(0, 255).to(torch.uint8))          # same kernel, same inputs, all 8 channels
    img = image.cpu().numpy()
    for name, want in (("albedo", img[..., :3]), ("metallic", img[..., 3:4]), ("roughness", img[..., 4:5]), ("normal", img[..., 5:])):
        png = decode_png(open(os.path.join(out_dir, "textures", name + ".png"), "rb").read())
        assert np.array_equal(png.reshape(want.shape), want[::-1]), name
    pv, pvt, pf, other = parse_obj(os.path.join(out_dir, "object.obj"))
    assert other == ["mtllib object.mtl", "usemtl material_0"] and len(pvt) == 3 * len(pf)
    lo, hi = aabb[:3].cpu().numpy().astype(np.float64), aabb[3:].cpu().numpy().astype(np.float64)
    cell = (hi - lo).max() / 48
    assert (pv >= lo - cell).all() and (pv <= hi + cell).all()
    mtl = [l.strip() for l in open(os.path.join(out_dir, "object.mtl"))]
    assert mtl[0] == "newmtl material_0" and mtl[-4:] == ["map_Kd textures/albedo.png", "map_Pm textures/metallic.png",
                                                           "map_Pr textures/roughness.png", "map_Bump -bm 1.000000 textures/normal.png"]
    glb_dir = str(tmp_path / "glb")
    out2 = ae.decode_texmesh(glb_dir, fm, 48, n_faces=2000, texture_reso=512, save_voxel=False, file_format="glb")
    assert files_under(glb_dir) == ["object.glb"] and torch.equal(out2["image"], image)
    data = open(os.path.join(glb_dir, "object.glb"), "rb").read()
    jlen = struct.unpack("<I", data[12:16])[0]
    gl = json.loads(data[20:20 + jlen])
    assert struct.unpack("<III", data[:12]) == (0x46546C67, 2, len(data)) and len(gl["images"]) == 3
    assert gl["materials"][0]["pbrMetallicRoughness"]["metallicFactor"] == 1.0
    bv = gl["bufferViews"][gl["images"][0]["bufferView"]]
    blob = data[28 + jlen:]
    assert blob[bv["byteOffset"]:bv["byteOffset"] + bv["byteLength"]] == open(os.path.join(out_dir, "textures", "albedo.png"), "rb").read()
    # the vertex-coloured default: albedo = columns 1..3
    verts, tris, cols = ae.decode_mesh(str(tmp_path / "vertex"), fm, 48)
    assert cols.shape[1] == 3 and len(tris) > 0


def test_sample_cli_geometry_only(tmp_path, monkeypatch, oracle):
    import torch_port as tp
    from sin3dm_amd import sample
    from sin3dm_amd.diffusion.unet_triplane import TriplaneUNetModelSmall
    # one UNet forward at 4 channels against the CPU port of the reference's algorithm
    mc, (H, W, D), B = 64, (10, 14, 6), 2
    sd = T.synthetic_state_dict(T.unet_param_shapes(in_channels=4, model_channels=mc, out_channels=4), 0)
    model = TriplaneUNetModelSmall(4, mc, 4, use_scale_shift_norm=True)
    model.load_state_dict(sd)
    model.to("cuda:0").eval()
    x = torch.from_numpy(T.synthetic_noise((B, 4, H + D, W + D), 1))
    t = torch.tensor([7.0, 431.0])
    with torch.no_grad():
        y = model(x.to("cuda:0"), t.to("cuda:0"), H=H, W=W, D=D)
        want = tp.unet_forward(sd, x, t, H, W, D, mc)
    e = relerr(y.cpu().numpy(), want.numpy())
    print(f"UNet forward at 4 channels vs the CPU port: {e:.2e}")
    assert tuple(y.shape) == (B, 4, H + D, W + D) and e < 1e-4
    # ... and one ancestral and one DDIM step (the fused step of the sampling loops) against the oracle's update of that output
    from sin3dm_amd.diffusion.script_util import create_gaussian_diffusion
    diff = create_gaussian_diffusion(steps=1000, predict_xstart=True, timestep_respacing="10")
    eps = T.synthetic_noise((B, 4, H + D, W + D), 2)
    diff.noise_fn = lambda z: torch.from_numpy(eps).to(z.device)
    ti = 7
    tab, tmap = oracle.schedule_tables(sorted(diff.use_timesteps))
    with torch.no_grad():
        tt = torch.full((B,), ti, device="cuda:0", dtype=torch.int64)
        o1 = diff.p_sample(model, x.to("cuda:0"), tt, model_kwargs=dict(H=H, W=W, D=D))
        o2 = diff.ddim_sample(model, x.to("cuda:0"), tt, model_kwargs=dict(H=H, W=W, D=D))
        mo = tp.unet_forward(sd, x, torch.full((B,), float(tmap[ti])), H, W, D, mc).numpy()
    s1, p1 = oracle.p_sample_update(mo, x.numpy(), eps, tab, ti)
    s2, _ = oracle.ddim_update(mo, x.numpy(), eps, tab, ti)
    errs = (relerr(o1["sample"].cpu().numpy(), s1), relerr(o1["pred_xstart"].cpu().numpy(), p1), relerr(o2["sample"].cpu().numpy(), s2))
    print("sampler step at 4 channels vs the oracle (p_sample, pred_xstart, ddim):", ["%.2e" % v for v in errs])
    assert max(errs) < 1e-4
    # the CLI on a --data_type sdf experiment: voxels, then the textured-mode output of an untextured asset
    tag = make_experiment(str(tmp_path), "sdf", "skip")
    common = ["--tag", tag, "--n_samples", "1", "--use_ddim", "True", "--timestep_respacing", "5", "--reso", "32"]
    paths = sample.main(common + ["--vox", "--output", "vox"])
    d = np.load(paths[0])
    assert d["feat_xy"].shape == (4, 24, 32) and d["feat_xz"].shape == (4, 24, 24) and d["feat_yz"].shape == (4, 32, 24)
    assert all(np.isfinite(d[k]).all() for k in d.files)
    vox = np.load(os.path.join(os.path.dirname(paths[0]), "r32_voxel.npz"))["voxel"]
    assert vox.shape == (23, 32, 23) and vox.dtype == bool
    monkeypatch.setenv("S3D_MESH", "textured")
    paths = sample.main(common + ["--n_faces", "2000", "--output", "mesh"])
    folder = os.path.dirname(paths[0])
    assert sorted(os.listdir(folder)) == ["feat.npz", "mesh_r32_simple.obj", "sdfgrid_r32.npz", "voxel.npz"]
    sdf = np.load(os.path.join(folder, "sdfgrid_r32.npz"))["sdf_grid"]
    assert sdf.shape == (23, 32, 23) and np.isfinite(sdf).all() and sdf.min() < 0 < sdf.max()
    rows = [l.split() for l in open(os.path.join(folder, "mesh_r32_simple.obj"))]
    assert {r[0] for r in rows} == {"v", "f"} and all(len(r) == 4 for r in rows)          # no colours, no texture coordinates
    v = np.asarray([[float(c) for c in r[1:]] for r in rows if r[0] == "v"])
    assert 0 < sum(r[0] == "f" for r in rows) <= 2000 and np.isfinite(v).all()
    # and the vertex mode writes an OBJ without colours
    monkeypatch.delenv("S3D_MESH")
    paths = sample.main(common + ["--output", "vertex"])
    rows = [l.split() for l in open(os.path.join(os.path.dirname(paths[0]), "object.obj"))]
    assert rows and all(len(r) == 4 for r in rows)


def test_sample_cli_pbr(tmp_path, monkeypatch):
    from sin3dm_amd import sample
    tag = make_experiment(str(tmp_path), "sdfpbr", "pbr")
    monkeypatch.setenv("S3D_MESH", "textured")
    paths = sample.main(["--tag", tag, "--n_samples", "1", "--use_ddim", "True", "--timestep_respacing", "5", "--reso", "32",
                         "--n_faces", "2000", "--texreso", "512"])
    d = np.load(paths[0])
    assert d["feat_xy"].shape == (12, 24, 32) and all(np.isfinite(d[k]).all() for k in d.files)
    folder = os.path.dirname(paths[0])
    assert files_under(folder) == ["feat.npz"] + PBR_OBJ_FILES + ["voxel.npz"]
    from test_texmesh_gpu import decode_png
    for name, ch in (("albedo", 3), ("metallic", 1), ("roughness", 1), ("normal", 3)):
        png = decode_png(open(os.path.join(folder, "textures", name + ".png"), "rb").read())
        assert png.reshape(512, 512, -1).shape[2] == ch and png.max() > 0
