"""GPU: the narrow-band iso-surface extraction (s3d_mcs_*, isosurface.marching_cubes_sparse) against the checkers
of tests/sparse_mc_cases.py — (a) every brick active is the dense device mesh bit for bit, (b) the seeded and grown band is the
dense device mesh restricted to the components of the seed bricks, the occupancy, a random-weight decoder through decode_mesh /
decode_texmesh against the dense path's files, one run beyond the dense path's ceiling, and determinism.
tests/test_sparse_mc_host.py shows on the CPU that the checkers can fail."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

import sparse_mc_cases as SC
from conftest import REPO

pytestmark = pytest.mark.gpu


def _lookup_fn(grid):
    """sample_fn of a stored grid: grid[clip(floor(c), 0, dims - 1)] (sparse_mc_cases.lookup on the device); counts its points"""
    g = torch.tensor(np.asarray(grid), device="cuda")
    g = g if g.dim() == 4 else g[..., None]
    hi = torch.tensor(g.shape[:3], device="cuda") - 1
    calls = []

    def fn(coords):
        calls.append(int(coords.shape[0]))
        idx = torch.minimum(coords.floor().long().clamp_(min=0), hi)
        return g[idx[:, 0], idx[:, 1], idx[:, 2]]
    fn.calls = calls
    return fn


def _np(mesh):
    return tuple(x.cpu().numpy() if x is not None else None for x in mesh[:3])


_dense = {}


def dense_of(oracle, c):
    """the dense DEVICE mesh of a case with the cell of every triangle and the component labels, computed once"""
    if c.name not in _dense:
        from sin3dm_amd.encoding.isosurface import marching_cubes
        v, t, a = _np(marching_cubes(torch.tensor(c.grid, device="cuda"), c.iso, c.pad, n_attr=c.n_attr))
        _dense[c.name] = SC.dense_mesh(c, v, t, a, oracle.mesh_components)
    return _dense[c.name]


@pytest.mark.parametrize("name,B", SC.case_blocks())
def test_all_active_is_the_dense_mesh_bit_for_bit(oracle, name, B):
    from sin3dm_amd.encoding.isosurface import marching_cubes_sparse
    c = SC.case(name)
    d = dense_of(oracle, c)
    fn = _lookup_fn(c.grid)
    v, t, a, info = marching_cubes_sparse(fn, SC.value_of(c).shape, c.iso, c.pad, n_attr=c.n_attr, block=B, all_active=True, return_info=True)
    assert t.dtype == torch.int32 and v.dtype == torch.float32
    SC.check_all_active(d, _np((v, t, a)))
    assert info["closed"] and info["rounds"] == 0 and info["n_active"] == info["n_bricks"] == info["n_seed"]
    assert info["n_samples"] == info["n_bricks"] * B ** 3 == sum(fn.calls)


@pytest.mark.parametrize("name,B", SC.case_blocks())
def test_grown_band_occupancy_and_largest_component(oracle, name, B):
    from sin3dm_amd.encoding.isosurface import largest_component, marching_cubes_sparse
    c = SC.case(name)
    d = dense_of(oracle, c)
    val = SC.value_of(c)
    r = SC.rule(val, c.iso, c.pad, B)
    fn = _lookup_fn(c.grid)
    v, t, a, info = marching_cubes_sparse(fn, val.shape, c.iso, c.pad, n_attr=c.n_attr, block=B, return_info=True, occupancy=True)
    got = _np((v, t, a))
    print(f"{name} B={B}: {info['n_seed']} seeds, {info['n_active']} of {info['n_bricks']} bricks after {info['rounds']} rounds, "
          f"{info['n_samples']} evaluations for {val.size} voxels, {len(got[1])} of {len(d.tris)} triangles")
    assert info["closed"] is True
    assert (info["rounds"], info["n_seed"], info["n_active"], info["n_bricks"]) == (r.rounds, int(r.seed.sum()), int(r.active.sum()), r.active.size)
    assert info["n_samples"] == r.n_samples == sum(fn.calls)
    SC.check_closed_result(d, r, got)
    SC.check_seed_components(d, r, got)
    # occupancy: the dense one wherever nothing was lost
    occ = info["occupancy"].cpu().numpy()
    want = val < np.float32(c.iso)
    assert occ.dtype == np.uint8 and occ.shape == val.shape
    if (name, B) in SC.NO_SEEDS:
        assert not occ.any() and len(got[1]) == 0
    elif name == "pole_speck":
        diff = np.argwhere(occ.astype(bool) != want)
        assert diff.tolist() == [list(SC.SPECK)]                                 # the component the lattice cannot see
        assert got[0][:, 2].max() > 25.0                                         # the pole is there
        assert not (np.abs(got[0] - np.asarray(SC.SPECK)).max(1) <= 1.0).any() and len(got[1]) < len(d.tris)
    else:
        assert len(got[1]) == len(d.tris)
        assert np.array_equal(occ.astype(bool), want)
    # largest_component sees no difference (the largest component of every case with seeds meets a seed brick: the host test)
    if len(d.tris) and (name, B) not in SC.NO_SEEDS:
        dv, dt, _ = largest_component(torch.tensor(d.verts, device="cuda"), torch.tensor(d.tris, device="cuda"))
        sv, st_, _ = largest_component(v, t)
        assert torch.equal(dv.view(torch.int32), sv.view(torch.int32)) and torch.equal(dt, st_)


def test_round_limit_and_dilation(oracle):
    from sin3dm_amd.encoding.isosurface import marching_cubes_sparse
    c = SC.case("pole_speck")
    d = dense_of(oracle, c)
    val = SC.value_of(c)
    *mesh, info = marching_cubes_sparse(_lookup_fn(c.grid), val.shape, block=8, max_rounds=0, return_info=True)
    r0 = SC.rule(val, c.iso, c.pad, 8, max_rounds=0)
    assert info["closed"] is False and info["rounds"] == 0 and info["n_active"] == info["n_seed"] == int(r0.seed.sum())
    SC.same_mesh(_np(mesh), SC.select_cells(d, r0.ext), "seeds only")
    *mesh, info = marching_cubes_sparse(_lookup_fn(c.grid), val.shape, block=8, dilate=1, return_info=True)
    r1 = SC.rule(val, c.iso, c.pad, 8, dilate=1)
    assert info["closed"] and info["n_active"] == int(r1.active.sum()) > int(r0.seed.sum())
    SC.check_closed_result(d, r1, _np(mesh))
    with pytest.raises(AssertionError):
        marching_cubes_sparse(_lookup_fn(c.grid), val.shape, block=5)


def test_same_call_same_bits():
    from sin3dm_amd.encoding.isosurface import marching_cubes_sparse
    c = SC.case("torus_37_attrs")
    runs = [marching_cubes_sparse(_lookup_fn(c.grid), SC.value_of(c).shape, n_attr=3, block=8, return_info=True, occupancy=True) for _ in range(2)]
    for x, y in zip(runs[0][:3], runs[1][:3]):
        assert x.shape[0] > 0 and torch.equal(x.view(torch.int32), y.view(torch.int32))
    assert torch.equal(runs[0][3]["occupancy"], runs[1][3]["occupancy"])
    c = SC.case("fourier")                               # several rounds, many blocks appending their keys at once
    runs = [marching_cubes_sparse(_lookup_fn(c.grid), SC.value_of(c).shape, c.iso, block=4) for _ in range(2)]
    assert torch.equal(runs[0][0].view(torch.int32), runs[1][0].view(torch.int32)) and torch.equal(runs[0][1], runs[1][1])


# ------------------------------------------------------------------ a random-weight decoder through the exports
# weight seed 8: the first of 5..11 for which the CPU port finds both preconditions of decoder_precondition (5, 6, 9, 10 leave a speck
# outside the band whose voxel would differ in voxel.npz)
DEC_HWD, DEC_RESO, DEC_B, DEC_SEED = (16, 12, 10), 40, 4, 8


def decoder_experiment(root, seed=DEC_SEED, hwd=DEC_HWD):
    """an experiment directory with a random-weight sdftex auto-encoder on a small triplane -> (tag, state dict, planes [1,12,h,w], aabb)"""
    from sin3dm_amd import testing as T
    from sin3dm_amd.utils import parser_util as pu
    tag = os.path.join(root, "exp")
    pu.train_args(["--tag", tag, "--data_path", "shape.npz", "--model_channels", "64", "--fm_reso", "16"])
    H, W, D = hwd
    fm = [np.tanh(T.synthetic_noise((12, H, W), 1)), np.tanh(T.synthetic_noise((12, H, D), 2)), np.tanh(T.synthetic_noise((12, W, D), 3))]
    np.savez_compressed(pu.encoding_feat_path(tag), feat_xy=fm[0], feat_xz=fm[1], feat_yz=fm[2])
    net = T.synthetic_state_dict(T.ae_param_shapes(with_encoder=True), seed)
    aabb = torch.tensor([-0.8, -0.6, -0.5, 0.8, 0.6, 0.5])
    net["aabb"] = aabb
    torch.save({"net": net, "aabb": aabb.numpy(), "featmap_size": hwd, "Ka": None, "Kd": None, "Ks": None, "Ns": None},
               os.path.join(pu.encoding_log_dir(tag), "ckpt_final.pth"))
    return tag, net, [torch.from_numpy(f)[None] for f in fm], aabb


def decoder_precondition(net, fm, aabb, reso=DEC_RESO, B=DEC_B):
    """On the CPU, with the torch port of the reference's decoder: the dense field at `reso`, the rule with the decoder on the
    lattice, whether the largest component of the dense mesh has a triangle in a cell of the seed bricks, and whether the band's
    occupancy is the dense one (no voxel outside the band on the other side of the level than its brick's lattice corner).
    -> (holds, dims, triangles of the largest component, all triangles, Rule)"""
    sys.path.insert(0, os.path.join(REPO, "oracle"))
    import oracle as orc
    import torch_port as tp
    size = aabb[3:] - aabb[:3]
    dims = tuple(int(x) for x in (float(reso) * size / size.max()).tolist())

    def field(coords):
        c = torch.as_tensor(np.asarray(coords), dtype=torch.float32)
        pts = (0.5 + c) / torch.tensor(dims, dtype=torch.float32) * size + aabb[:3]
        with torch.no_grad():
            return tp.ae_decode(net, pts, fm, aabb)[:, 0].numpy()
    grid = np.stack(np.meshgrid(*[np.arange(d) for d in dims], indexing="ij"), -1).reshape(-1, 3)
    val = field(grid).reshape(dims).astype(np.float32)
    c = SC.SCase("decoder", val, 0.0, 1.0, 0, (B,))
    v, t = orc.marching_cubes(val, 0.0, 1.0)
    d = SC.dense_mesh(c, v, t, None, orc.mesh_components)
    r = SC.rule(val, 0.0, 1.0, B, lattice_fn=field)
    if not len(t):
        return False, dims, 0, 0, r
    fl = d.labels[d.tris[:, 0]]
    roots, counts = np.unique(fl, return_counts=True)
    big = fl == roots[np.argmax(counts)]
    same_occupancy = np.array_equal(SC.rule_occupancy(val, 0.0, r), val < 0)
    return bool(r.ext0[tuple(d.tri_cell[big].T)].any()) and same_occupancy, dims, int(big.sum()), len(t), r


def _bytes(folder):
    return {os.path.relpath(os.path.join(r, f), folder): open(os.path.join(r, f), "rb").read() for r, _, fs in os.walk(folder) for f in fs}


@pytest.fixture(scope="module")
def decoder(tmp_path_factory):
    from test_pbr_gpu import autoencoder
    from sin3dm_amd.utils import parser_util as pu
    from sin3dm_amd.utils.triplane_util import load_triplane_data
    tag, net, fm_cpu, aabb = decoder_experiment(str(tmp_path_factory.mktemp("sparse_dec")))
    holds, dims, n_big, n_all, r = decoder_precondition(net, fm_cpu, aabb)
    print(f"decoder seed {DEC_SEED}: grid {dims}, largest component {n_big} of {n_all} triangles, {int(r.seed.sum())} seed bricks of {r.seed.size}; "
          f"it meets a seed brick: {holds}")
    assert holds and n_big > 100, "the weight seed no longer gives a largest component the brick lattice sees: choose another DEC_SEED"
    ae = autoencoder(tag)
    fm = [f.unsqueeze(0) for f in load_triplane_data(pu.encoding_feat_path(tag), device="cuda:0", compose=False)]
    return ae, fm, dims


def test_decode_mesh_sparse_writes_the_dense_files(decoder, tmp_path, monkeypatch):
    ae, fm, dims = decoder
    dense = ae.decode_mesh(str(tmp_path / "dense"), fm, DEC_RESO)
    assert len(dense[1]) > 0
    monkeypatch.setattr(type(ae), "decode_grid", lambda *a, **k: pytest.fail("the sparse export decoded the dense grid"))
    monkeypatch.setattr(type(ae.net), "decode_grid", lambda *a, **k: pytest.fail("the sparse export decoded the dense grid"))
    sparse = ae.decode_mesh(str(tmp_path / "sparse"), fm, DEC_RESO, sparse=DEC_B)
    info = ae.last_sparse_info
    print(f"decode_mesh(sparse={DEC_B}): {info}; dense grid {dims} = {int(np.prod(dims))} evaluations")
    assert info["closed"] and info["n_seed"] < info["n_bricks"]
    fa, fb = _bytes(str(tmp_path / "dense")), _bytes(str(tmp_path / "sparse"))
    assert sorted(fa) == sorted(fb) == ["object.obj", "voxel.npz"]
    assert fa["object.obj"] == fb["object.obj"]
    va, vb = np.load(str(tmp_path / "dense" / "voxel.npz"))["vox_grid"], np.load(str(tmp_path / "sparse" / "voxel.npz"))["vox_grid"]
    assert va.dtype == vb.dtype == np.bool_ and va.shape == vb.shape == tuple(dims) and np.array_equal(va, vb)
    assert fa["voxel.npz"] == fb["voxel.npz"]
    for x, y in zip(dense, sparse):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    with pytest.raises(ValueError):
        ae.decode_mesh(str(tmp_path / "bad"), fm, DEC_RESO, sparse=5)


def test_decode_texmesh_sparse_writes_the_dense_files(decoder, tmp_path, monkeypatch):
    ae, fm, dims = decoder
    dense = ae.decode_texmesh(str(tmp_path / "dense"), fm, DEC_RESO, n_faces=200, texture_reso=64)
    monkeypatch.setattr(type(ae), "decode_grid", lambda *a, **k: pytest.fail("the sparse export decoded the dense grid"))
    sparse = ae.decode_texmesh(str(tmp_path / "sparse"), fm, DEC_RESO, n_faces=200, texture_reso=64, sparse=DEC_B)
    assert dense is not None and sparse is not None and 0 < len(dense["tris"]) <= 200
    fa, fb = _bytes(str(tmp_path / "dense")), _bytes(str(tmp_path / "sparse"))
    assert sorted(fa) == sorted(fb) == ["object.mtl", "object.obj", "object.png", "voxel.npz"]
    for name in fa:
        assert fa[name] == fb[name], name
    assert torch.equal(dense["image"], sparse["image"]) and torch.equal(dense["verts"].view(torch.int32), sparse["verts"].view(torch.int32))


# ------------------------------------------------------------------ beyond the dense ceiling
def test_torus_at_1024_cubed():
    """3 * 1026^3 edges do not fit the dense path's 32-bit scans; the band of an analytic torus at 1024^3 does: closed, every edge
    shared by exactly two triangles, Euler characteristic 0, every vertex within one cell of the analytic surface"""
    from sin3dm_amd import _lib
    from sin3dm_amd.encoding.isosurface import _handle, marching_cubes_sparse
    N, B = 1024, 16
    tiny = torch.zeros(8, device="cuda")
    nv, nt = C.c_int64(), C.c_int64()
    with pytest.raises(NotImplementedError, match="too large"):
        _lib.check(_lib.load().s3d_mc_count(_handle(tiny.device), _lib.ptr(tiny), N, N, N, 1, 0.0, 1, 1.0, C.byref(nv), C.byref(nt), _lib.stream_ptr()))
    ctr, R, r = (N - 1) / 2.0, 0.30 * N, 0.10 * N
    evaluated = []

    def sdf(p):
        q = torch.sqrt((p[:, 0] - ctr) ** 2 + (p[:, 1] - ctr) ** 2) - R
        return torch.sqrt(q * q + (p[:, 2] - ctr) ** 2) - r

    def fn(coords):
        evaluated.append(coords.shape[0])
        return sdf(coords)[:, None]
    v, t, a, info = marching_cubes_sparse(fn, (N, N, N), block=B, return_info=True)
    print(f"torus at {N}^3, B={B}: {info}; {v.shape[0]} vertices, {t.shape[0]} triangles, {sum(evaluated) / N ** 3:.4f} of the grid evaluated")
    assert info["closed"] and a is None and sum(evaluated) == info["n_samples"] < 0.06 * N ** 3
    V, F = v.shape[0], t.shape[0]
    assert F > 1_000_000 and int(t.min()) == 0 and int(t.max()) == V - 1
    tl = t.long()
    e = torch.cat([tl[:, [0, 1]], tl[:, [1, 2]], tl[:, [2, 0]]])
    key = torch.minimum(e[:, 0], e[:, 1]) * V + torch.maximum(e[:, 0], e[:, 1])
    _, counts = torch.unique(key, return_counts=True)
    assert bool((counts == 2).all())
    assert V - counts.shape[0] + F == 0                                          # a torus
    assert float(sdf(v).abs().max()) <= 1.0
