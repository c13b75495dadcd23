"""CPU-only: the host side of known-region sampling — regions on a triplane (utils/region_util.py), the edit
CLI's parser, and the schedule walker with its fixed noise order."""
import numpy as np
import pytest
import torch

from sin3dm_amd import testing as T
from sin3dm_amd.utils import region_util as R
from sin3dm_amd.utils.triplane_util import compose_featmaps

HWD = (6, 8, 5)


def _src(hwd=HWD, C=3):
    H, W, D = hwd
    return tuple(torch.from_numpy(T.synthetic_noise(s, k)) for k, s in enumerate(((C, H, W), (C, H, D), (C, W, D)), 1))


def test_box_projections_per_plane_and_plane_subsets():
    box = (1, 4, 2, 7, 0, 3)
    m = R.box_mask(HWD, box)
    exp = {p: torch.zeros(s) for p, s in zip(R.PLANES, ((6, 8), (6, 5), (8, 5)))}
    exp["xy"][1:4, 2:7] = 1
    exp["xz"][1:4, 0:3] = 1
    exp["yz"][2:7, 0:3] = 1
    for p in R.PLANES:
        assert torch.equal(m[p], exp[p]), p
    for sub in (("xy",), ("xz", "yz"), "xy,yz", ()):
        ms = R.box_mask(HWD, box, planes=sub)
        names = R._planes(sub)
        for p in R.PLANES:
            assert torch.equal(ms[p], exp[p] if p in names else torch.zeros_like(exp[p])), (sub, p)
    with pytest.raises(ValueError):
        R.box_mask(HWD, box, planes=("zx",))


def test_feather_ramps_inside_the_box():
    # 2 cells of ramp inside each end that has free cells beyond it: 1/3, 2/3, then 1; no ramp at the canvas border
    m = R.box_mask((12, 12, 12), (2, 10, 0, 12, 0, 12), feather=2)["xy"]
    col = m[:, 5]
    exp = torch.tensor([0, 0, 1 / 3, 2 / 3, 1, 1, 1, 1, 2 / 3, 1 / 3, 0, 0])
    assert torch.allclose(col, exp, atol=1e-7)
    assert torch.equal(m[5, :], torch.ones(12))                        # y spans the whole canvas: nothing to blend into
    # two feathered axes: the smaller of the two weights
    m2 = R.box_mask((12, 12, 12), (2, 10, 3, 9, 0, 12), feather=2)["xy"]
    assert abs(float(m2[2, 3]) - 1 / 3) < 1e-7 and abs(float(m2[3, 3]) - 1 / 3) < 1e-7 and abs(float(m2[3, 4]) - 2 / 3) < 1e-7
    assert float(m2[5, 6]) == 1.0 and float(m2[1, 5]) == 0.0
    assert torch.equal(R.box_mask((12, 12, 12), (2, 10, 3, 9, 0, 12), feather=0)["xy"][2:10, 3:9], torch.ones(8, 6))


def test_clipping_and_empty_boxes():
    m = R.box_mask(HWD, (-3, 2, 6, 20, 4, 9))
    assert float(m["xy"].sum()) == 2 * 2 and torch.equal(m["xy"][0:2, 6:8], torch.ones(2, 2))
    assert float(m["xz"].sum()) == 2 * 1 and float(m["yz"].sum()) == 2 * 1
    for bad in ((2, 2, 0, 8, 0, 5), (0, 6, 9, 12, 0, 5), (0, 6, 0, 8, 5, 7), (4, 3, 0, 8, 0, 5)):
        with pytest.raises(ValueError):
            R.box_mask(HWD, bad)
    with pytest.raises(ValueError):
        R.build_known(_src(), HWD, [R.keep((0, 6, 0, 8, 7, 9))])
    with pytest.raises(ValueError):                                    # pasted wholly outside the canvas
        R.build_known(_src(), HWD, [R.paste((0, 2, 0, 2, 0, 2), (6, 0, 0))])


def test_fraction_rounding():
    assert R.cells_from_fractions((0.1, 0.5, 0.26, 0.74, 0.0, 1.0), (10, 8, 5)) == (1, 5, 2, 6, 0, 5)
    assert R.cells_from_fractions((0.33, 0.34, 0.0, 0.01, 0.99, 1.0), (10, 8, 5)) == (3, 4, 0, 1, 4, 5)


def test_keep_and_composition():
    src = _src()
    box = (1, 4, 0, 8, 2, 5)
    y0, mask = R.build_known(src, HWD, [R.keep(box)])
    H, W, D = HWD
    assert y0.shape == (3, H + D, W + D) and mask.shape == (3, H + D, W + D)
    # composition equals compose_featmaps of the per-plane arrays
    planes, masks = [torch.zeros_like(p) for p in src], R.box_mask(HWD, box)
    planes[0][:, 1:4, 0:8] = src[0][:, 1:4, 0:8]
    planes[1][:, 1:4, 2:5] = src[1][:, 1:4, 2:5]
    planes[2][:, 0:8, 2:5] = src[2][:, 0:8, 2:5]
    assert torch.equal(y0, compose_featmaps(*planes)[0])
    assert torch.equal(mask[0], compose_featmaps(masks["xy"], masks["xz"], masks["yz"])[0])
    assert torch.equal(mask[1], mask[0]) and torch.equal(mask[2], mask[0])
    # the D x D corner is zero in both
    assert float(y0[:, H:, W:].abs().max()) == 0.0 and float(mask[:, H:, W:].abs().max()) == 0.0
    # a whole-volume keep still leaves the corner zero
    y0, mask = R.build_known(src, HWD, [R.keep((0, H, 0, W, 0, D))])
    assert torch.equal(y0, compose_featmaps(*src)[0])
    assert float(mask[:, H:, W:].abs().max()) == 0.0 and float(mask[:, :H, :].min()) == 1.0 and float(mask[:, H:, :W].min()) == 1.0


def test_paste_translates_and_later_operations_overwrite_earlier_ones():
    src = _src()
    canvas = (6, 12, 5)                                                # W retargeted 8 -> 12
    ops = [R.keep((0, 6, 0, 5, 0, 5)), R.paste((0, 6, 0, 3, 0, 5), (0, 4, 0)), R.paste((2, 4, 5, 8, 0, 5), (2, 10, 0), planes=("xy",))]
    y0, mask = R.build_known(src, canvas, ops)
    H, W, D = canvas
    xy, xz, yz = y0[:, :H, :W], y0[:, :H, W:], y0[:, H:, :W].transpose(-1, -2)
    mxy, myz = mask[0, :H, :W], mask[0, H:, :W].transpose(-1, -2)
    assert torch.equal(xy[:, :, 0:4], src[0][:, :, 0:4])               # kept in place ...
    assert torch.equal(xy[:, :, 4:7], src[0][:, :, 0:3])               # ... the paste lies on top of the kept column 4
    assert torch.equal(yz[:, 4:7, :], src[2][:, 0:3, :]) and torch.equal(yz[:, 0:4, :], src[2][:, 0:4, :])
    assert torch.equal(xz, src[1])                                     # both operations span x and z: the later wrote the same cells
    # third operation: clipped to the canvas (y 10..13 -> 10..12), xy only
    assert torch.equal(xy[:, 2:4, 10:12], src[0][:, 2:4, 5:7])
    assert float(mxy[2:4, 10:12].min()) == 1.0 and float(mxy[0:2, 10:12].max()) == 0.0 and float(myz[10:12].max()) == 0.0
    assert float(mxy[:, 7:10].max()) == 0.0 and float(mxy[:, 0:7].min()) == 1.0
    assert float(y0[:, H:, W:].abs().max()) == 0.0 and float(mask[:, H:, W:].abs().max()) == 0.0


@pytest.mark.parametrize("grow,planes", [(((0, 0), (0, 3), (0, 0)), ("xy", "yz")),
                                         (((2, 0), (0, 0), (1, 1)), ("xy", "xz", "yz")),
                                         (((1, 1), (2, 0), (0, 2)), ("xy", "xz", "yz")),
                                         (((0, 0), (0, 0), (0, 2)), ("xz", "yz"))])
def test_outpaint_offsets_and_default_planes(grow, planes):
    src = _src()
    canvas = R.outpaint_canvas(HWD, grow)
    assert canvas == tuple(n + a + b for n, (a, b) in zip(HWD, grow))
    assert R.outpaint_planes(grow) == planes
    y0, mask = R.build_known(src, canvas, [R.outpaint(grow)])
    H, W, D = canvas
    got = dict(zip(R.PLANES, (y0[:, :H, :W], y0[:, :H, W:], y0[:, H:, :W].transpose(-1, -2))))
    gm = dict(zip(R.PLANES, (mask[0, :H, :W], mask[0, :H, W:], mask[0, H:, :W].transpose(-1, -2))))
    off = [g[0] for g in grow]
    for k, p in enumerate(R.PLANES):
        r, c = R._AXES[p]
        sl = (slice(off[r], off[r] + HWD[r]), slice(off[c], off[c] + HWD[c]))
        exp_m = torch.zeros_like(gm[p])
        if p in planes:
            exp_m[sl] = 1
            assert torch.equal(got[p][(slice(None),) + sl], src[k]), p
        else:
            assert float(got[p].abs().max()) == 0.0, p               # a plane without a grown axis stays free
        assert torch.equal(gm[p], exp_m), p
    # planes= overrides the default
    _, m2 = R.build_known(src, canvas, [R.outpaint(grow, planes=("xz",))])
    assert float(m2[0, :H, :W].max()) == 0.0 and float(m2[0, :H, W:].max()) == 1.0
    with pytest.raises(ValueError):
        R.build_known(src, HWD if canvas != HWD else (1, 1, 1), [R.outpaint(grow)])


def test_edit_parser_leaves_sample_args_alone(tmp_path):
    from test_formats import reference_experiment
    from sin3dm_amd import edit
    from sin3dm_amd.utils import parser_util as pu
    tag = reference_experiment(str(tmp_path))
    rest = ["--tag", tag, "--n_samples", "2", "--timestep_respacing", "10", "--resize", "1", "1.5", "1", "--reso", "32"]
    argv = rest[:4] + ["--keep", "0", "1", "0", "0.5", "0", "1", "--feather", "2"] + rest[4:] + [
        "--paste", "0", "1", "0", "0.25", "0", "1", "0", "0.75", "0", "--keep", "0", "0.5", "0", "1", "0", "1", "--resample", "3",
        "--planes", "xy,yz"]
    ed, args = edit.edit_args(argv)
    assert vars(args) == vars(pu.sample_args(rest))
    assert ed.keep == [[0, 1, 0, 0.5, 0, 1], [0, 0.5, 0, 1, 0, 1]] and len(ed.paste) == 1 and ed.resample == 3 and ed.feather == 2
    assert ed.planes == "xy,yz" and ed.outpaint is None
    canvas, ops = edit.plan(ed, (8, 12, 6), args.resize)
    assert canvas == (8, 18, 6) and [o["op"] for o in ops] == ["keep", "keep", "paste"]
    assert ops[0]["box"] == (0, 8, 0, 6, 0, 6) and ops[2]["box"] == (0, 8, 0, 3, 0, 6) and ops[2]["dst"] == (0, 13, 0)
    ed, args = edit.edit_args(["--tag", tag, "--outpaint", "0", "0", "0", "0.3", "0", "0"])
    canvas, ops = edit.plan(ed, (8, 12, 6), args.resize)
    assert canvas == (8, 16, 6) and ops[0]["grow"] == ((0, 0), (0, 4), (0, 0))
    for bad in (["--tag", tag], ["--tag", tag, "--outpaint", "0", "0", "0", "1", "0", "0", "--keep", "0", "1", "0", "1", "0", "1"],
                ["--tag", tag, "--keep", "0", "1", "0", "1", "0", "1", "--resample", "0"]):
        with pytest.raises(ValueError):
            edit.edit_args(bad)


@pytest.mark.parametrize("r", [1, 2, 3])
def test_schedule_walker(r):
    from sin3dm_amd.diffusion.gaussian_diffusion import known_region_schedule
    Tn = 10
    ev = list(known_region_schedule(Tn, r))
    assert len(ev) == (Tn - 1) * r + 1
    assert [i for i, _ in ev] == [i for i in range(Tn - 1, 0, -1) for _ in range(r)] + [0]
    assert ev[-1] == (0, False) and not any(rn for i, rn in ev if i == 0)          # no re-noise at i = 0
    for i in range(1, Tn):
        assert [rn for j, rn in ev if j == i] == [True] * (r - 1) + [False]          # between two repeats only
    with pytest.raises(ValueError):
        list(known_region_schedule(Tn, 0))


class _StubModel:
    """A denoiser that needs no GPU: returns its input (the loops call it through _step's unfused branch)."""
    calls = 0

    def parameters(self):
        return iter([torch.zeros(1)])

    def __call__(self, x, ts, **kw):
        type(self).calls += 1
        return x


@pytest.mark.parametrize("r", [1, 2])
def test_loop_asks_noise_fn_in_the_documented_order(r, monkeypatch):
    """The loop itself, with the two library calls replaced by recorders: per evaluation noise_fn is asked for the step's eps, then
    eps_known, then the re-noising's eps when one follows — and the tensors arrive at the calls in those roles."""
    from sin3dm_amd import _lib
    from sin3dm_amd.diffusion import gaussian_diffusion as gd
    from sin3dm_amd.diffusion.script_util import create_gaussian_diffusion
    diff = create_gaussian_diffusion(steps=1000, predict_xstart=True, timestep_respacing="10")
    shape = (2, 3, 5, 6)
    asked, seen = [], []

    def noise_fn(like):
        asked.append(len(asked))
        return torch.full(like.shape, float(len(asked) - 1))
    diff.noise_fn = noise_fn
    monkeypatch.setattr(_lib, "require_gpu", lambda t=None: None)

    def fake_step(self, mode, model, x, t, clip, dfn, mkw, fuse=False, noise=None, carry=0, known=None, **kw):
        seen.append(("step", int(t.host_values[0]), float(noise.flatten()[0]), float(known[2].flatten()[0]), carry))
        assert known[0].shape == tuple(shape) and known[1].shape == tuple(shape)
        return torch.zeros(shape), torch.zeros(shape), None

    def fake_renoise(self, x_prev, t, noise):
        seen.append(("renoise", int(t[0]), float(noise.flatten()[0])))
        return torch.zeros(shape)
    monkeypatch.setattr(gd.GaussianDiffusion, "_step", fake_step)
    monkeypatch.setattr(gd.GaussianDiffusion, "renoise", fake_renoise)
    known = gd.KnownRegion(torch.zeros(shape[1:]), torch.ones((1,) + shape[1:]))
    outs = list(diff.p_sample_loop_progressive(_StubModel(), shape, noise=torch.zeros(shape), device="cpu", known=known, resample=r))
    ev = list(gd.known_region_schedule(10, r))
    assert len(outs) == len(ev) == 9 * r + 1
    k, exp = 0, []
    for n, (i, rn) in enumerate(ev):
        carry = (_lib.CARRY_OUT if n < len(ev) - 1 and not rn else 0) | (_lib.CARRY_IN if n > 0 and not ev[n - 1][1] else 0)
        exp.append(("step", i, float(k), float(k + 1), carry))
        k += 2
        if rn:
            exp.append(("renoise", i, float(k)))
            k += 1
    assert seen == exp
    assert asked == list(range(k))
    with pytest.raises(ValueError):
        list(diff.ddim_sample_loop_progressive(_StubModel(), shape, noise=torch.zeros(shape), device="cpu", known=known,
                                               y0=torch.zeros(shape), mask=torch.zeros(shape)))
