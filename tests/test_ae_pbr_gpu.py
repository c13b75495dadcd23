"""The auto-encoder training tier of the PBR network with its material heads (s3d_ae_create_pbr; data_type sdfpbr with
--enc_net_type pbr) on the MI355X against vectors captured from the reference under autograd (tests/golden/ae_pbr.npz; cases,
inputs and bounds in tests/ae_pbr_cases.py, each bound beside the reference's own float32 gap it comes from)."""
import json
from types import SimpleNamespace

import numpy as np
import pytest

import ae_pbr_cases as P
from conftest import digest_errors, golden, relerr, zero_grad_params
from sin3dm_amd import testing as T

pytestmark = pytest.mark.gpu
CASES = list(P.CASES)


def _net(case):
    import torch
    from sin3dm_amd.encoding.networks import AutoEncoderGroupPBR
    net = AutoEncoderGroupPBR(*P.CASES[case]["args"], tex_channels=P.TEX_CHANNELS)
    missing, unexpected = net.load_state_dict(P.state_dict(case), strict=False)
    assert not unexpected and missing == ["aabb"]
    net = net.to(torch.device("cuda:0")).build_training_tier(material_heads=True)
    net.reset_aabb(torch.tensor(P.AABB).cuda())
    return net


def _volume(case):
    import torch
    return torch.from_numpy(P.volume(case)).cuda()


def _batch(case, seed, n=P.N_POINTS):
    import torch
    return [torch.from_numpy(a).cuda() for a in P.batch(case, seed, n)]


def _loss_cfg():
    from sin3dm_amd.encoding.model import ae_loss_cfg
    return ae_loss_cfg("weightedl1", "l1", P.THR, P.RATIO, 1.0)


def _check(what, value, bound):
    print(f"{what}: {value:.3e} (bound {bound:.1e})")
    assert value < bound, (what, value, bound)


@pytest.mark.parametrize("case", CASES)
def test_encode_forward_losses_and_grads(case):
    import torch
    g, B = golden("ae_pbr"), P.BOUNDS[case]
    net, vol = _net(case), _volume(case)
    fm = net.encode(vol)
    assert all(f.shape[1] == net.in_feat_channels for f in fm)
    _check(f"{case} encode", max(relerr(f.cpu().numpy(), g[f"{case}.{k}"]) for f, k in zip(fm, P.PLANES)), B["encode"])
    pts, sdf, tex = _batch(case, int(g[f"{case}.seed"]))
    pred = net(vol, pts)
    assert tuple(pred.shape) == (P.N_POINTS, 9)
    _check(f"{case} pred", relerr(pred.cpu().numpy(), g[f"{case}.pred"]), B["pred"])
    # the training-tier forward and the inference decoder (fused gather+MLP kernel) agree
    _check(f"{case} decode", relerr(net.decode(pts, fm).cpu().numpy(), g[f"{case}.pred"]), B["pred"])
    _check(f"{case} decode vs pred", relerr(net.decode(pts, fm).cpu().numpy(), pred.cpu().numpy()), B["pred"])
    losses, pred2, grads = net.loss_and_grads(vol, pts, sdf, tex, _loss_cfg(), want_pred=True)
    assert torch.equal(pred2, pred)
    assert net.loss_names == P.LOSS_NAMES and tuple(losses.shape) == (4,)
    _check(f"{case} losses", float(np.max(np.abs(losses.cpu().numpy() - g[f"{case}.losses"]))), B["loss"])
    grads = grads.clone()
    _, _, again = net.loss_and_grads(vol, pts, sdf, tex, _loss_cfg())
    assert torch.equal(grads, again)                               # every reduction has a fixed order (no float atomics)
    named = {k: v.cpu().numpy() for k, v in net.split_flat(grads).items()}
    assert all(np.isfinite(v).all() for v in named.values())
    w = digest_errors(named, g, f"{case}.grad")
    for k in ("norm", "proj", "full"):
        _check(f"{case} grad.{k}", w[k], B[f"grad.{k}"])
    # the twice-used norm: its gradient, stored whole in the fixture, on its own
    for pl in P.PLANES:
        for leaf in ("weight", "bias"):
            k = f"tex_convs.1.norm_{pl}.{leaf}"
            _check(f"{case} {k}", relerr(named[k], g[f"{case}.grad/full/{k}"]), B["grad.full"])


@pytest.mark.parametrize("case", CASES)
def test_optimizer_steps(case):
    """three ShapeAutoEncoder iterations on the fixture's batches: AdamW per parameter group + ExponentialLR on the flat vector"""
    from sin3dm_amd.encoding.model import FlatGroupAdamW
    g, B = golden("ae_pbr"), P.BOUNDS[case]
    lr, split, decay = (float(v) for v in g[f"{case}.steps.hyper"])
    net, vol = _net(case), _volume(case)
    init = {k: v.detach().clone() for k, v in net.named_parameters()}
    opt = FlatGroupAdamW(net, lr, split, lr_decay=decay)
    assert len(opt.ranges) == 2 and opt.ranges[1][0] == net.tex_group_begin and opt.lrs == pytest.approx([lr * split, lr])
    tex_names = {n for n, off, _, _ in net._ae_layout if off >= net.tex_group_begin}
    assert tex_names == {n for n, _ in net.named_parameters() if not n.startswith("geo_")}
    for step in range(3):
        p, s, c = _batch(case, int(g[f"{case}.steps.seeds"][step]))
        losses, _, grads = net.loss_and_grads(vol, p, s, c, _loss_cfg())
        want = g[f"{case}.steps.losses"][step]
        got = losses.cpu().numpy()
        print(f"{case} step {step} losses: max |got - want| {np.max(np.abs(got - want)):.3e}")
        assert np.all(np.abs(got - want) < P.STEPS_LOSS * np.maximum(1.0, want)), (step, got, want)
        opt.step(grads)
    skip = zero_grad_params(case, "ae_pbr")
    d = {k: (p.detach() - init[k]).cpu().numpy() for k, p in net.named_parameters()}
    w = digest_errors(d, g, f"{case}.steps.dparam", skip)
    _check(f"{case} steps.norm", w["norm"], B["steps.norm"])
    _check(f"{case} steps.proj", w["proj"], B["steps.proj"])
    # the decode path sees the trained weights
    fm = net.encode(vol)
    p, _, _ = _batch(case, 7, 64)
    _check(f"{case} decode after steps", relerr(net.decode(p, fm).cpu().numpy(), net(vol, p).cpu().numpy()), B["pred"])


def test_weight_gradients_on_the_side_stream_change_no_bit():
    """BWD_SIDE on (the default) and off in ONE process: identical losses and gradients, iteration after iteration; 8192 points
    on 24 x 32 x 20 maps, so that every launch has more than one block"""
    import torch
    from sin3dm_amd import _lib
    H, W, D, N = 24, 32, 20, 8192
    vol = torch.tanh(torch.from_numpy(T.synthetic_noise((1, 9, 2 * H, 2 * W, 2 * D), 1200))).cuda()

    def run():
        net = _net("pbr")
        out = []
        for it in range(3):
            p, s, c = _batch("pbr", 50 + it, N)
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


def test_a_pbr_handle_shares_no_state_with_a_skip_net():
    """one skip-net (skip8) iteration before and after a PBR handle was created and used in the same process: the same bits"""
    import torch
    import ae_variants_cases as V
    from sin3dm_amd.encoding.networks import AutoEncoderGroupSkip

    def skip8():
        c = V.CASES["skip8"]
        net = AutoEncoderGroupSkip(*c["args"], tex_channels=8)
        net.load_state_dict(T.synthetic_state_dict(V.shapes("skip8"), V.SEED_WEIGHTS), strict=False)
        net = net.to(torch.device("cuda:0")).build_training_tier()
        net.reset_aabb(torch.tensor(V.AABB).cuda())
        p, s, c_ = _batch("pbr", 61)
        losses, pred, grads = net.loss_and_grads(_volume("pbr"), p, s, c_, _loss_cfg(), want_pred=True)
        torch.cuda.synchronize()
        return losses.clone(), pred.clone(), grads.clone()

    before = skip8()
    pbr = _net("pbr")
    p, s, c_ = _batch("pbr", 62)
    _, _, gp = pbr.loss_and_grads(_volume("pbr"), p, s, c_, _loss_cfg())
    torch.cuda.synchronize()
    assert torch.isfinite(gp).all()
    after = skip8()
    assert all(torch.equal(a, b) for a, b in zip(before, after))


def test_train_loop_reduces_the_loss(tmp_path):
    """ShapeAutoEncoder.train for --data_type sdfpbr --enc_net_type pbr on a synthetic .npz; the checkpoint loads back in a fresh
    object and decodes to the same bits"""
    import torch
    from sin3dm_amd.encoding.model import ShapeAutoEncoder
    from test_ae_variants_gpu import _synthetic_npz
    path = str(tmp_path / "shape.npz")
    _synthetic_npz(path, "sdfpbr")
    cfg = SimpleNamespace(enc_net_type="pbr", fdim_geo=4, fdim_tex=8, fdim_up=64, hidden_dim=256, n_hidden_layers=4,
                          data_type="sdfpbr", enc_batch_size=2048, enc_n_iters=60, vol_ratio=0.1, fm_reso=32, sdf_loss="weightedl1",
                          tex_loss="l1", tex_weight=1.0, tex_threshold_ratio=0.999, sdf_renorm=0, enc_lr=5e-3, enc_lr_split=0.2,
                          enc_lr_decay=0.1, gpu_id=0)
    ae = ShapeAutoEncoder(str(tmp_path / "encoding"), cfg)
    ae.train(path, log_every=20)
    assert ae.net.variant == 2 and ae.net.training_tier_built
    assert ae.featmap_size == [24, 32, 20] and tuple(ae.input_grid.shape) == (1, 9, 48, 64, 40)
    logs = [json.loads(l) for l in open(tmp_path / "encoding" / "progress.jsonl")]
    assert set(logs[0]) == {"sdf_loss", "rgb_loss", "mr_loss", "normal_loss", "step"}
    print("sdf_loss", logs[0]["sdf_loss"], "->", logs[-1]["sdf_loss"])
    assert logs[-1]["sdf_loss"] < 0.6 * logs[0]["sdf_loss"], logs
    assert all(np.isfinite(v) for l in logs for v in l.values())
    ae2 = ShapeAutoEncoder(str(tmp_path / "encoding"), cfg)
    ae2.load_ckpt("final")
    assert set(ae2.net.state_dict()) == set(T.pbr_param_shapes(4, 8, 64, 256, 4, 8, with_encoder=True)) | {"aabb"}
    fm = ae.encode()
    p = ae.pts_grid[:777]
    a, b = ae.net.decode(p, fm, aabb=ae.aabb), ae2.net.decode(p, fm, aabb=ae2.aabb)
    assert torch.equal(a, b) and a.shape[1] == 9
    _check("sdfpbr/pbr decode vs net(vol, p)", relerr(b.cpu().numpy(), ae.net(ae.input_grid, p, aabb=ae.aabb).cpu().numpy()), 2e-5)
