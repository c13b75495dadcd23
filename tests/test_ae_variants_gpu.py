"""The auto-encoder training tier's network variants on the MI355X against vectors captured from the reference under autograd
(tests/golden/ae_variants.npz; cases, inputs and bounds in tests/ae_variants_cases.py): the geometry-only net (data_type sdf)
and the skip net with 8 material channels (sdfpbr with --enc_net_type skip).  The bounds are those of tests/test_hip_ae.py."""
import ctypes as C
import json
from types import SimpleNamespace

import numpy as np
import pytest

import ae_variants_cases as V
from conftest import digest_errors, golden, relerr, zero_grad_params
from sin3dm_amd import testing as T

pytestmark = pytest.mark.gpu
CASES = list(V.CASES)


def _net(case):
    import torch
    from sin3dm_amd.encoding.networks import AutoEncoderGroupSkip
    c = V.CASES[case]
    net = AutoEncoderGroupSkip(*c["args"], use_tex=c["kind"] != "geo", tex_channels=max(c["tex_channels"], 1))
    missing, unexpected = net.load_state_dict(T.synthetic_state_dict(V.shapes(case), V.SEED_WEIGHTS), strict=False)
    assert not unexpected and missing == ["aabb"]
    net = net.to(torch.device("cuda:0")).build_training_tier()
    net.reset_aabb(torch.tensor(V.AABB).cuda())
    return net


def _volume(case):
    import torch
    return torch.from_numpy(V.volume(case)).cuda()


def _batch(case, seed, n=V.N_POINTS):
    import torch
    return [None if a is None else torch.from_numpy(a).cuda() for a in V.batch(case, seed, n)]


def _loss_cfg():
    from sin3dm_amd.encoding.model import ae_loss_cfg
    return ae_loss_cfg("weightedl1", "l1", V.THR, V.RATIO, 1.0)


def _check(what, value, bound):
    print(f"{what}: {value:.3e} (bound {bound:.0e})")
    assert value < bound, (what, value, bound)


@pytest.mark.parametrize("case", CASES)
def test_encode_forward_losses_and_grads(case):
    import torch
    g = golden("ae_variants")
    net, vol = _net(case), _volume(case)
    fm = net.encode(vol)
    assert all(f.shape[1] == net.in_feat_channels for f in fm)
    _check(f"{case} encode", max(relerr(f.cpu().numpy(), g[f"{case}.{k}"]) for f, k in zip(fm, V.PLANES)), V.BOUNDS["encode"])
    pts, sdf, tex = _batch(case, int(g[f"{case}.seed"]))
    pred = net(vol, pts)
    assert tuple(pred.shape) == (V.N_POINTS, net.out_channels)
    _check(f"{case} pred", relerr(pred.cpu().numpy(), g[f"{case}.pred"]), V.BOUNDS["pred"])
    # the training-tier forward and the inference decoder (fused gather+MLP kernel) agree
    _check(f"{case} decode", relerr(net.decode(pts, fm).cpu().numpy(), g[f"{case}.pred"]), V.BOUNDS["pred"])
    losses, pred2, grads = net.loss_and_grads(vol, pts, sdf, tex, _loss_cfg(), want_pred=True)
    assert torch.equal(pred2, pred)
    names = V.loss_names(case)
    assert net.loss_names == names
    got = losses.cpu().numpy()[:len(names)]
    _check(f"{case} losses", float(np.max(np.abs(got - g[f"{case}.losses"]))), V.BOUNDS["loss"])
    if case == "geo":
        assert float(losses[1]) == 0.0                               # no texture term
    grads = grads.clone()
    _, _, again = net.loss_and_grads(vol, pts, sdf, tex, _loss_cfg())
    assert torch.equal(grads, again)                               # every reduction has a fixed order (no float atomics)
    named = {k: v.cpu().numpy() for k, v in net.split_flat(grads).items()}
    assert all(np.isfinite(v).all() for v in named.values())
    w = digest_errors(named, g, f"{case}.grad")
    for k in ("norm", "proj", "full"):
        _check(f"{case} grad.{k}", w[k], V.BOUNDS[f"grad.{k}"])


@pytest.mark.parametrize("case", CASES)
def test_optimizer_steps(case):
    """three ShapeAutoEncoder iterations on the fixture's batches: AdamW per parameter group + ExponentialLR on the flat vector"""
    from sin3dm_amd.encoding.model import FlatGroupAdamW
    g = golden("ae_variants")
    lr, split, decay = (float(v) for v in g[f"{case}.steps.hyper"])
    net, vol = _net(case), _volume(case)
    init = {k: v.detach().clone() for k, v in net.named_parameters()}
    opt = FlatGroupAdamW(net, lr, split, lr_decay=decay)
    assert len(opt.ranges) == (1 if case == "geo" else 2)
    for step in range(3):
        p, s, c = _batch(case, int(g[f"{case}.steps.seeds"][step]))
        losses, _, grads = net.loss_and_grads(vol, p, s, c, _loss_cfg())
        want = g[f"{case}.steps.losses"][step]
        got = losses.cpu().numpy()[:len(want)]
        assert np.all(np.abs(got - want) < 5e-4 * np.maximum(1.0, want)), (step, got, want)
        opt.step(grads)
    skip = zero_grad_params(case, "ae_variants")
    d = {k: (p.detach() - init[k]).cpu().numpy() for k, p in net.named_parameters()}
    w = digest_errors(d, g, f"{case}.steps.dparam", skip)
    _check(f"{case} steps.norm", w["norm"], V.BOUNDS["steps.norm"])
    _check(f"{case} steps.proj", w["proj"], V.BOUNDS["steps.proj"])
    # the decode path sees the trained weights
    fm = net.encode(vol)
    p, _, _ = _batch(case, 7, 64)
    _check(f"{case} decode after steps", relerr(net.decode(p, fm).cpu().numpy(), net(vol, p).cpu().numpy()), V.BOUNDS["pred"])


@pytest.mark.parametrize("case", CASES)
def test_weight_gradients_on_the_side_stream_change_no_bit(case):
    """BWD_SIDE on (the default) and off in ONE process: identical losses and gradients, iteration after iteration; 8192 points
    on 24 x 32 x 20 maps, so that every launch has more than one block"""
    import torch
    from sin3dm_amd import _lib
    H, W, D, N = 24, 32, 20, 8192
    C_ = 1 + V.CASES[case]["tex_channels"]
    vol = torch.tanh(torch.from_numpy(T.synthetic_noise((1, C_, 2 * H, 2 * W, 2 * D), 1200))).cuda()

    def run():
        net = _net(case)
        out = []
        for it in range(3):
            p, s, c = _batch(case, 50 + it, N)
            losses, _, grads = net.loss_and_grads(vol, p, s, c, _loss_cfg())
            torch.cuda.synchronize()
            out.append((losses.clone(), grads.clone()))
        return out

    try:
        _lib.set_option("BWD_SIDE", 0)
        inline = run()
        _lib.set_option("BWD_SIDE", None)
        side = run()
    finally:
        _lib.set_option("BWD_SIDE", None)
    for (la, ga), (lb, gb) in zip(inline, side):
        assert torch.equal(la, lb) and torch.equal(ga, gb)
        assert torch.isfinite(ga).all() and float(ga.abs().max()) > 0


def test_sdftex_through_the_variant_constructor_is_the_same_bits():
    """s3d_ae_create_variant(cfg, 0) (what the Python network calls) against s3d_ae_create on the same parameters, volume and batch"""
    import torch
    from sin3dm_amd import _lib
    from sin3dm_amd.encoding.networks import AutoEncoderGroupSkip
    lib = _lib.load()
    net = AutoEncoderGroupSkip(4, 8, 64, 256, 4)
    net.load_state_dict(T.synthetic_state_dict(T.ae_param_shapes(with_encoder=True), 5), strict=False)
    net = net.to(torch.device("cuda:0"))
    net.reset_aabb(torch.tensor(V.AABB).cuda())
    H, W, D = V.HWD
    vol = torch.tanh(torch.from_numpy(T.synthetic_noise((1, 4, 2 * H, 2 * W, 2 * D), 1200))).cuda()
    rng = np.random.Generator(np.random.PCG64(11))
    pts = torch.from_numpy(rng.uniform(-1.1, 1.1, size=(1000, 3)).astype(np.float32) * np.asarray(V.AABB[3:], np.float32)).cuda()
    sdf = torch.from_numpy(np.clip(rng.normal(0, 0.04, size=(1000, 1)), -V.THR, V.THR).astype(np.float32)).cuda()
    tex = torch.from_numpy(rng.uniform(0, 1, size=(1000, 3)).astype(np.float32)).cuda()
    cfg = _loss_cfg()
    losses, pred, grads = net.loss_and_grads(vol, pts, sdf, tex, cfg, want_pred=True)
    h = C.c_void_p()
    _lib.check(lib.s3d_ae_create(C.byref(_lib.DecoderCfg(4, 8, 64, 256, 4, 3)), C.byref(h)))
    try:
        flat = net.flat_parameters.clone()
        st = _lib.stream_ptr()
        _lib.check(lib.s3d_ae_attach(h, _lib.ptr(flat), flat.numel()))
        _lib.check(lib.s3d_ae_repack(h, st))
        _lib.check(lib.s3d_ae_set_volume(h, _lib.ptr(vol), 4, 2 * H, 2 * W, 2 * D, st))
        l2, p2, g2 = torch.empty(2, device="cuda"), torch.empty_like(pred), torch.empty_like(grads)
        _lib.check(lib.s3d_ae_loss_grads(h, _lib.ptr(pts), _lib.ptr(sdf), _lib.ptr(tex), 1000, net._aabb6(None), C.byref(cfg),
                                         _lib.ptr(l2), _lib.ptr(p2), _lib.ptr(g2), st))
        torch.cuda.synchronize()
        assert torch.equal(l2, losses) and torch.equal(p2, pred) and torch.equal(g2, grads)
        # three texture channels are ONE group: the grouped entry point gives the two-loss call's numbers
        l4, g4 = torch.empty(4, device="cuda"), torch.empty_like(grads)
        _lib.check(lib.s3d_ae_loss_grads_groups(h, _lib.ptr(pts), _lib.ptr(sdf), _lib.ptr(tex), 1000, net._aabb6(None), C.byref(cfg),
                                                _lib.ptr(l4), None, _lib.ptr(g4), st))
        torch.cuda.synchronize()
        assert torch.equal(l4[:2], losses) and float(l4[2]) == 0.0 and float(l4[3]) == 0.0 and torch.equal(g4, grads)
    finally:
        lib.s3d_ae_destroy(h)


def _synthetic_npz(path, data_type):
    """the shape of tests/test_hip_ae.py:test_train_loop_reduces_the_loss in the reference's data format for sdf / sdfpbr"""
    rng = np.random.Generator(np.random.PCG64(3))
    R, ext = (24, 32, 20), np.asarray([0.7, 1.0, 0.45])
    ax = [np.linspace(-1, 1, r) * s for r, s in zip(R, ext)]
    pts_grid = np.stack(np.meshgrid(*ax, indexing="ij"), -1).astype(np.float32)
    sdf = (np.linalg.norm(pts_grid / ext, axis=-1) - 0.6).astype(np.float32) * 0.3
    near = (rng.uniform(-1, 1, size=(4000, 3)) * ext).astype(np.float32)
    sdf_near = ((np.linalg.norm(near / ext, axis=-1) - 0.6) * 0.3).astype(np.float32)
    arrs = dict(aabb=np.asarray([-0.7, -1.0, -0.45, 0.7, 1.0, 0.45], np.float32), threshold=0.05, pts_grid=pts_grid, sdf_grid=sdf,
                pts_near_surf=near, sdf_near_surf=sdf_near)
    if data_type == "sdfpbr":
        def mat(p):                                              # eight smooth material channels in [0, 1]
            return np.concatenate([0.5 + 0.5 * np.sin(3 * p), 0.5 + 0.5 * np.cos(2 * p[..., :2]), 0.5 + 0.5 * np.sin(4 * p + 1)],
                                  -1).astype(np.float32)
        arrs.update(tex_grid=mat(pts_grid), tex_near_surf=mat(near), pts_on_surf=near[:500], tex_on_surf=mat(near[:500]))
    np.savez(path, **arrs)


@pytest.mark.parametrize("data_type, enc_net_type", [("sdf", "skip"), ("sdf", "pbr"), ("sdfpbr", "skip")])
def test_train_loop_reduces_the_loss(tmp_path, data_type, enc_net_type):
    """ShapeAutoEncoder.train on a synthetic .npz of the data type; the checkpoint loads back in a fresh object for decoding"""
    import torch
    from sin3dm_amd.encoding.model import ShapeAutoEncoder
    path = str(tmp_path / "shape.npz")
    _synthetic_npz(path, data_type)
    cfg = SimpleNamespace(enc_net_type=enc_net_type, fdim_geo=4, fdim_tex=8, fdim_up=64, hidden_dim=256, n_hidden_layers=4,
                          data_type=data_type, enc_batch_size=2048, enc_n_iters=60, vol_ratio=0.1, fm_reso=32, sdf_loss="weightedl1",
                          tex_loss="l1", tex_weight=1.0, tex_threshold_ratio=0.999, sdf_renorm=0, enc_lr=5e-3, enc_lr_split=0.2,
                          enc_lr_decay=0.1, gpu_id=0)
    ae = ShapeAutoEncoder(str(tmp_path / "encoding"), cfg)
    ae.train(path, log_every=20)
    assert ae.featmap_size == [24, 32, 20]
    assert tuple(ae.input_grid.shape) == (1, 1 if data_type == "sdf" else 9, 48, 64, 40)
    assert ("tex" in ae._sample_batch(8)) == (data_type != "sdf")
    logs = [json.loads(l) for l in open(tmp_path / "encoding" / "progress.jsonl")]
    keys = {"sdf": {"sdf_loss"}, "sdfpbr": {"sdf_loss", "rgb_loss", "mr_loss", "normal_loss"}}[data_type]
    assert set(logs[0]) == keys | {"step"}
    assert logs[-1]["sdf_loss"] < 0.6 * logs[0]["sdf_loss"], logs
    assert all(np.isfinite(v) for l in logs for v in l.values())
    stat = json.load(open(tmp_path / "encoding" / "eval_stat.json"))
    assert np.isfinite(stat["mean_tsdf_l1_error"]) and ("surf_tex_l1_error" in stat) == (data_type != "sdf")
    ae2 = ShapeAutoEncoder(str(tmp_path / "encoding"), cfg)
    ae2.load_ckpt("final")
    fm = ae.encode()
    p = ae.pts_grid[:777]
    a, b = ae.net.decode(p, fm, aabb=ae.aabb), ae2.net.decode(p, fm, aabb=ae2.aabb)
    assert torch.equal(a, b) and a.shape[1] == (1 if data_type == "sdf" else 9)
    _check(f"{data_type}/{enc_net_type} decode vs net(vol, p)", relerr(b.cpu().numpy(), ae.net(ae.input_grid, p, aabb=ae.aabb).cpu().numpy()), 2e-5)
