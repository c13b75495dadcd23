"""Auto-encoder training tier (s3d_ae.hip, s3d_ae_kernels.hip) against the CPU port (oracle/torch_port.py) under float64
autograd, over shapes, configs, point counts and placements, and every loss mode the CLI offers.

Same parameters (T.synthetic_state_dict) and the same float32 inputs on both sides; the port promotes them to float64.
Each case checks encode, the training forward and the inference decoder, both losses, every gradient, and that a second
call gives the same bits.  Batches are drawn so that no hidden ReLU pre-activation, sdf residual or texture residual
lies within KINK of zero (in float64): at such a point relu', sign(g - p) and sign(d) are round-off decisions and the
gradient is implementation-defined.  A row that comes too close is redrawn; N stays fixed."""
import numpy as np
import pytest

from conftest import relerr
from sin3dm_amd import testing as T

pytestmark = pytest.mark.gpu

KINK = 1e-5
# conv biases that feed an InstanceNorm: their gradient is analytically zero (round-off on the device)
ZERO_GRAD = {"geo_encoder.bias", "tex_encoder.bias", "geo_convs.in_layers.0.bias", "tex_convs.in_layers.0.bias"}
# (geo, tex, up, hidden, hidden layers, tex_channels)
CFG_A = (4, 8, 64, 256, 4, 3)                 # the default
CFG_B = (8, 4, 32, 64, 4, 3)
CFG_C = (4, 4, 96, 128, 4, 1)
CFG_D = (4, 8, 32, 32, 4, 2)
AABB = (-0.7, -1.0, -0.45, 0.7, 1.0, 0.45)
AABB_OFF = (0.1, -0.3, 0.2, 0.9, 0.5, 0.65)   # not centred on the origin
AABB_UNIT = (-1.0, -1.0, -1.0, 1.0, 1.0, 1.0)
LOSS = dict(sdf_loss="weightedl1", tex_loss="l1", thr=0.05, ratio=0.999, tw=1.0, renorm=False)


@pytest.fixture(scope="module", autouse=True)
def _port_threads(oracle):                       # (the oracle fixture puts oracle/ with torch_port on sys.path)
    import torch
    n = torch.get_num_threads()
    torch.set_num_threads(min(16, n))
    yield
    torch.set_num_threads(n)


def _volume(hwd, tc, seed):
    import torch
    H, W, D = hwd
    vol = torch.tanh(torch.from_numpy(T.synthetic_noise((1, 1 + tc, 2 * H, 2 * W, 2 * D), seed)))
    vol[:, 1:] = 0.5 * vol[:, 1:] + 0.5
    return vol


def _placer(place, hwd, aabb, rng):
    """n -> float32 points [n, 3].  Normalised coordinates u (aabb -> [-1, 1]) per placement:
    uniform  u in [-1.15, 1.15]: outside the aabb on every axis (border clamp);
    faces    one coordinate exactly on a face of the aabb, the others inside;
    lattice  every coordinate on a texel centre or a texel edge of its planes (align_corners=False);
    cell     every point in the one bilinear cell chosen here (all points in one sorted bin of every plane)."""
    lo, hi = np.asarray(aabb[:3], np.float32), np.asarray(aabb[3:], np.float32)
    R = np.asarray(hwd)
    cell = rng.integers(0, np.maximum(R - 1, 1))

    def to_pts(u):
        return (lo + (u + 1) / 2 * (hi - lo)).astype(np.float32)

    def draw(n):
        if place == "uniform":
            return to_pts(rng.uniform(-1.15, 1.15, size=(n, 3)))
        if place == "faces":
            p = to_pts(rng.uniform(-1, 1, size=(n, 3)))
            ax, side = rng.integers(0, 3, size=n), rng.integers(0, 2, size=n)
            p[np.arange(n), ax] = np.where(side == 1, hi[ax], lo[ax])
            return p
        if place == "lattice":
            return to_pts(rng.integers(0, 2 * R + 1, size=(n, 3)) / R - 1)
        if place == "cell":
            f = cell + rng.uniform(0.1, 0.9, size=(n, 3))
            return to_pts((2 * f + 1) / R - 1)
        raise ValueError(place)
    return draw


def _batch(sd32, vol, hwd, cfg, N, place, aabb, seed, loss, tex_near=False, band_rows=None):
    """Deterministic (pts, sdf, tex) float32 with every kink at least KINK away (see the module docstring).
    tex_near: texture targets pred +- U(0.01, 0.2) (huber residuals on both sides of its 0.1 cut-off);
    band_rows: sdf values pinned into the first rows (kept through redraws: only their points and textures move)."""
    import torch
    import torch_port as tp
    rng = np.random.Generator(np.random.PCG64(seed))
    thr, tc = loss["thr"], cfg[5]
    draw_pts = _placer(place, hwd, aabb, rng)
    lim = 0.5 * thr if loss.get("all_band") else thr
    scale = 1.0 / thr if loss["renorm"] else 1.0

    def draw_sdf(n):
        return (np.clip(rng.normal(0, 0.6 * thr, size=(n, 1)), -lim, lim) * scale).astype(np.float32)

    def draw_d(n):
        return rng.uniform(0.01, 0.2, size=(n, tc)) * rng.choice([-1.0, 1.0], size=(n, tc))

    pts, sdf = draw_pts(N), draw_sdf(N)
    tex = rng.uniform(0, 1, size=(N, tc)).astype(np.float32)
    d = draw_d(N)
    pinned = np.zeros(N, bool)
    if band_rows is not None:
        sdf[:len(band_rows), 0] = band_rows
        pinned[:len(band_rows)] = True
    sd64 = {k: v.double() for k, v in sd32.items()}
    a64 = torch.tensor(aabb, dtype=torch.float64)
    with torch.no_grad():
        fm64 = tp.ae_encode(sd64, vol.double())
    todo = np.arange(N)
    for _ in range(40):
        taps = []
        with torch.no_grad():
            pred = tp.ae_decode(sd64, torch.from_numpy(pts[todo]).double(), fm64, a64, cfg[0], taps=taps).numpy()
        if tex_near:
            tex[todo] = (pred[:, 1:] + d[todo]).astype(np.float32)
        m = np.min([t.abs().min(1).values.numpy() for t in taps], axis=0)
        m = np.minimum(m, np.abs(pred[:, 0] - sdf[todo, 0]))
        m = np.minimum(m, np.abs(pred[:, 1:] - tex[todo]).min(1))
        bad = todo[m < KINK]
        if not len(bad):
            return torch.from_numpy(pts), torch.from_numpy(sdf), torch.from_numpy(tex)
        pts[bad] = draw_pts(len(bad))
        free = bad[~pinned[bad]]
        sdf[free] = draw_sdf(len(free))
        tex[bad] = rng.uniform(0, 1, size=(len(bad), tc)).astype(np.float32)
        d[bad] = draw_d(len(bad))
        todo = bad
    raise RuntimeError(f"{len(bad)} rows stay within {KINK} of a kink")


def _port(sd32, vol, pts, sdf, tex, aabb, cfg, loss):
    import torch
    import torch_port as tp
    sd = {k: v.double().requires_grad_(True) for k, v in sd32.items()}
    fm = tp.ae_encode(sd, vol.double())
    pred = tp.ae_decode(sd, pts.double(), fm, torch.tensor(aabb, dtype=torch.float64), cfg[0])
    losses = tp.ae_losses(pred, sdf.double(), tex.double(), loss["thr"], loss["ratio"], loss["tw"], sdf_loss=loss["sdf_loss"],
                          tex_loss=loss["tex_loss"], sdf_renorm=loss["renorm"])
    (losses["sdf_loss"] + losses["tex_loss"]).backward()
    return ([f.detach() for f in fm], pred.detach(), [float(losses["sdf_loss"].detach()), float(losses["tex_loss"].detach())],
            {k: v.grad for k, v in sd.items()})


def _net(cfg, sd32, net=None):
    import torch
    from sin3dm_amd.encoding.networks import AutoEncoderGroupSkip
    if net is None:
        net = AutoEncoderGroupSkip(*cfg[:5], tex_channels=cfg[5]).to(torch.device("cuda:0"))
    missing, unexpected = net.load_state_dict(sd32, strict=False)
    assert not unexpected and missing == ["aabb"]
    return net


def _check(net, sd32, vol, pts, sdf, tex, aabb, cfg, loss, record):
    """Every comparison of one case on `net`; returns (losses, flat gradient) of the HIP tier."""
    import torch
    from sin3dm_amd.encoding.model import ae_loss_cfg
    fm_r, pred_r, loss_r, grad_r = _port(sd32, vol, pts, sdf, tex, aabb, cfg, loss)
    dev = torch.device("cuda:0")
    vol_c, pts_c, sdf_c, tex_c = (t.to(dev) for t in (vol, pts, sdf, tex))
    net.reset_aabb(torch.tensor(aabb, dtype=torch.float32, device=dev))
    lc = ae_loss_cfg(loss["sdf_loss"], loss["tex_loss"], loss["thr"], loss["ratio"], loss["tw"], loss["renorm"])
    # a larger batch first: the workspace then holds stale values where this batch's padded rows land
    big = torch.arange(2 * len(pts) + 64, device=dev) % len(pts)
    net.loss_and_grads(vol_c, pts_c[big], sdf_c[big], tex_c[big], lc)
    fm = net.encode(vol_c)
    for f, r, k in zip(fm, fm_r, ("xy", "xz", "yz")):
        assert relerr(f.cpu().numpy(), r.numpy()) < 2e-5, k
    pred = net(vol_c, pts_c)
    e_pred = relerr(pred.cpu().numpy(), pred_r.numpy())
    e_dec = relerr(net.decode(pts_c, fm).cpu().numpy(), pred_r.numpy())
    losses, pred2, g = net.loss_and_grads(vol_c, pts_c, sdf_c, tex_c, lc, want_pred=True)
    losses, g = losses.clone(), g.clone()
    losses2, _, g2 = net.loss_and_grads(vol_c, pts_c, sdf_c, tex_c, lc)
    e_loss = [abs(float(a) - b) / abs(b) for a, b in zip(losses.cpu(), loss_r)]
    gmax = max(float(v.norm()) for v in grad_r.values())
    worst, zero = (0.0, ""), 0.0
    for name, view in net.split_flat(g).items():
        ref = grad_r[name]
        if name in ZERO_GRAD:
            zero = max(zero, float(view.double().cpu().norm()) / gmax)
        else:
            worst = max(worst, (float((view.double().cpu() - ref).norm()) / max(float(ref.norm()), 1e-2 * gmax), name))
    record("errors", dict(pred=e_pred, decode=e_dec, loss=e_loss, grad=worst, zero_grad=zero))
    assert e_pred < 2e-5 and e_dec < 2e-5, (e_pred, e_dec)
    assert torch.equal(pred2, pred)
    assert max(e_loss) < 2e-5, (losses.tolist(), loss_r)
    assert worst[0] < 5e-4, worst
    assert zero < 1e-5, zero
    assert torch.equal(losses, losses2) and torch.equal(g, g2)          # fixed reduction orders: same bits again
    return losses, g


# (hwd, cfg, N, placement, aabb, seed)
SHAPES = {
    "7x4x9-A-63-uniform": ((7, 4, 9), CFG_A, 63, "uniform", AABB, 1),
    "13x16x11-B-65-faces-off": ((13, 16, 11), CFG_B, 65, "faces", AABB_OFF, 2),
    "2x33x3-C-64-lattice": ((2, 33, 3), CFG_C, 64, "lattice", AABB_UNIT, 3),
    "1x6x5-D-1-uniform": ((1, 6, 5), CFG_D, 1, "uniform", AABB, 4),
    "1x6x5-A-1000-cell": ((1, 6, 5), CFG_A, 1000, "cell", AABB, 5),
    "2x33x3-B-1000-cell-off": ((2, 33, 3), CFG_B, 1000, "cell", AABB_OFF, 6),
    "13x16x11-D-1000-uniform-off": ((13, 16, 11), CFG_D, 1000, "uniform", AABB_OFF, 7),
    "7x4x9-C-1000-lattice": ((7, 4, 9), CFG_C, 1000, "lattice", AABB_UNIT, 8),
    "7x4x9-B-1000-faces": ((7, 4, 9), CFG_B, 1000, "faces", AABB, 9),
    "63x64x65-A-65553-uniform-off": ((63, 64, 65), CFG_A, 65536 + 17, "uniform", AABB_OFF, 10),
}


@pytest.mark.parametrize("case", list(SHAPES))
def test_shapes_configs_points(case, record_property):
    """Odd and non-cubic volumes, planes narrower than the 5x5 blocks' reach, 1..65 553 points (ragged against the
    64-row padding), points outside the aabb, on its faces, on texel centres / edges, all in one cell; the default losses."""
    hwd, cfg, N, place, aabb, seed = SHAPES[case]
    sd32 = T.synthetic_state_dict(T.ae_param_shapes(*cfg, with_encoder=True), seed)
    vol = _volume(hwd, cfg[5], 1200 + seed)
    pts, sdf, tex = _batch(sd32, vol, hwd, cfg, N, place, aabb, 100 + seed, LOSS)
    _check(_net(cfg, sd32), sd32, vol, pts, sdf, tex, aabb, cfg, LOSS, record_property)


def _modes():
    out = {f"{s}-{t}": dict(LOSS, sdf_loss=s, tex_loss=t) for s in ("l1", "weightedl1") for t in ("l1", "l2", "huber")}
    out["weightedl1-l2-weight0.37-ratio0.5"] = dict(LOSS, tex_loss="l2", tw=0.37, ratio=0.5)
    out["l1-l1-renorm"] = dict(LOSS, sdf_loss="l1", renorm=True)
    out["weightedl1-huber-renorm-ratio0.5"] = dict(LOSS, tex_loss="huber", renorm=True, ratio=0.5, tw=0.37)
    out["weightedl1-l1-band-holds-all"] = dict(LOSS, all_band=True)
    return out


MODES = _modes()


def _public_path(tmp_path, cfg, sd32, loss):
    from types import SimpleNamespace
    from sin3dm_amd.encoding.model import ShapeAutoEncoder
    ns = SimpleNamespace(enc_net_type="skip", fdim_geo=cfg[0], fdim_tex=cfg[1], fdim_up=cfg[2], hidden_dim=cfg[3],
                         n_hidden_layers=cfg[4], data_type="sdftex", sdf_loss=loss["sdf_loss"], tex_loss=loss["tex_loss"],
                         tex_weight=loss["tw"], tex_threshold_ratio=loss["ratio"], sdf_renorm=int(loss["renorm"]), enc_lr=1e-3,
                         enc_lr_split=0.2, enc_lr_decay=0.1, enc_n_iters=10, gpu_id=0)
    ae = ShapeAutoEncoder(str(tmp_path), ns)
    _net(cfg, sd32, ae.net)
    ae.sdf_threshold = loss["thr"]
    return ae


def _train_step_matches(ae, vol, pts, sdf, tex, aabb, losses, g):
    """ShapeAutoEncoder.train_step (its _loss_cfg built from the CLI strings) gives the bits of the direct call."""
    import torch
    dev = torch.device("cuda:0")
    ae.input_grid = vol.to(dev)
    ae.aabb = torch.tensor(aabb, dtype=torch.float32, device=dev)
    ae.net.reset_aabb(ae.aabb)
    ae._set_optimizer(ae.init_lr, ae.min_lr_ratio)
    out = ae.train_step({"pts": pts.to(dev), "sdf": sdf.to(dev), "tex": tex.to(dev)})
    assert torch.equal(out["sdf_loss"], losses[0]) and torch.equal(out["tex_loss"], losses[1])
    assert torch.equal(ae._grad, g)


@pytest.mark.parametrize("mode", list(MODES))
def test_loss_modes(mode, tmp_path, record_property):
    """Every sdf x tex loss pair, tex_weight, ratio, the sdf_renorm band (1.0 * ratio) and a band holding every row, through
    ShapeAutoEncoder's string-to-mode map; huber batches straddle its 0.1 cut-off."""
    import torch
    import torch_port as tp
    loss = MODES[mode]
    hwd, N, aabb, seed = (7, 4, 9), 1000, AABB, 20 + list(MODES).index(mode)
    cfg = CFG_A if loss["sdf_loss"] == "l1" else CFG_B
    sd32 = T.synthetic_state_dict(T.ae_param_shapes(*cfg, with_encoder=True), seed)
    vol = _volume(hwd, cfg[5], 1300)
    pts, sdf, tex = _batch(sd32, vol, hwd, cfg, N, "uniform", aabb, 200 + seed, loss, tex_near=loss["tex_loss"] == "huber")
    s = np.abs(sdf.numpy()[:, 0]) < np.float32((1.0 if loss["renorm"] else loss["thr"]) * loss["ratio"])
    assert s.all() if loss.get("all_band") else 0.1 * N < s.sum() < N
    if loss["tex_loss"] == "huber":                  # texture residuals in the band on both sides of the 0.1 cut-off
        sd64 = {k: v.double() for k, v in sd32.items()}
        with torch.no_grad():
            p = tp.ae_decode(sd64, pts.double(), tp.ae_encode(sd64, vol.double()), torch.tensor(aabb, dtype=torch.float64), cfg[0])
        r = (p[:, 1:] - tex.double()).abs().numpy()[s]
        assert (r < 0.05).any() and ((r > 0.05) & (r < 0.1)).any() and (r > 0.1).any()
    ae = _public_path(tmp_path, cfg, sd32, loss)
    losses, g = _check(ae.net, sd32, vol, pts, sdf, tex, aabb, cfg, loss, record_property)
    _train_step_matches(ae, vol, pts, sdf, tex, aabb, losses, g)


@pytest.mark.parametrize("thr,ratio", [(0.03, 0.9), (0.15, 0.999)])
def test_band_boundary_rows(thr, ratio, tmp_path, record_property):
    """Rows with |sdf| at the reference's float32 band fl32(thr * ratio) and one ulp either side, plus the bound the
    library would form from the two float fields (fl32(fl32(thr) * fl32(ratio)): one ulp below the band at (0.03, 0.9),
    one above at (0.15, 0.999)).  The texture loss and its gradients take exactly the rows the reference takes."""
    f = np.float32
    b = f(thr * ratio)
    vals = np.asarray([np.nextafter(b, f(0)), b, np.nextafter(b, f(1)), f(f(thr) * f(ratio))], f)
    assert vals[3] != b
    rows = np.concatenate([vals, -vals])
    hwd, cfg, N, aabb = (7, 4, 9), CFG_A, 64, AABB
    loss = dict(LOSS, thr=thr, ratio=ratio)
    sd32 = T.synthetic_state_dict(T.ae_param_shapes(*cfg, with_encoder=True), 31)
    vol = _volume(hwd, cfg[5], 1301)
    pts, sdf, tex = _batch(sd32, vol, hwd, cfg, N, "uniform", aabb, 300, loss, band_rows=rows)
    ae = _public_path(tmp_path, cfg, sd32, loss)
    losses, g = _check(ae.net, sd32, vol, pts, sdf, tex, aabb, cfg, loss, record_property)
    _train_step_matches(ae, vol, pts, sdf, tex, aabb, losses, g)
