"""CPU-only: the host half of the geometry evaluation (sin3dm_amd/evaluation): the package and the library's entry points exist
and agree with the header, the procedural volumes of tests/eval_cases.py regenerate to what tests/golden/eval_geometry.npz was
recorded on, the private Random(1234) stream gives the recorded permutations, the command line's defaults, and the refusal to
run without a GPU."""
import ctypes as C
import os
import random
import re

import numpy as np
import pytest
import torch

import eval_cases as E
from conftest import REPO, golden
from sin3dm_amd import _lib

ENTRY_POINTS = ("s3d_eval_pool_or", "s3d_eval_patch_counts", "s3d_eval_patch_valid", "s3d_eval_pack_patches", "s3d_eval_lp_max",
                "s3d_eval_pack_volumes", "s3d_eval_pairwise_counts")


def test_package_and_entry_points_exist():
    import sin3dm_amd.evaluation as ev
    for name in ("load_voxgrid", "load_sdfgrid2vox", "extract_valid_patches", "lp_metrics", "pairwise_iou_dist", "eval_lp", "eval_div"):
        assert callable(getattr(ev, name)), name
    lib = _lib.load()
    header = open(os.path.join(REPO, "include", "sin3dm_hip.h")).read()
    for name in ENTRY_POINTS:
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
        decl = re.search(r"S3D_API int " + name + r"\(([^;]*)\);", header)
        assert decl, name
        assert len(decl.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name          # header and binding: the same arity
    assert int(re.search(r"#define S3D_ABI_VERSION (\d+)", header).group(1)) == _lib.ABI_VERSION == lib.s3d_abi_version()


def test_argument_errors_launch_nothing():
    """Validation happens before any launch, so it can be checked without a GPU."""
    lib = _lib.load()
    dims, counts = (C.c_int * 3)(48, 40, 36), (C.c_int * 3)()
    assert lib.s3d_eval_patch_counts(dims, 11, 5, counts) == 0 and tuple(counts) == (10, 8, 8)
    assert lib.s3d_eval_patch_counts(dims, 6, 3, counts) == 0 and tuple(counts) == (17, 14, 13)
    for ps in (1, 33, -3):
        assert lib.s3d_eval_patch_counts(dims, ps, 1, counts) == _lib.ERR_INVALID and b"patch_size" in lib.s3d_last_error()
        assert lib.s3d_eval_patch_valid(None, dims, ps, 1, None, None) == _lib.ERR_INVALID
        assert lib.s3d_eval_pack_patches(None, dims, ps, 1, None, 0, 0, None, None, None) == _lib.ERR_INVALID
    assert lib.s3d_eval_patch_counts(dims, 11, 0, counts) == _lib.ERR_INVALID and b"stride" in lib.s3d_last_error()
    assert lib.s3d_eval_lp_max(None, None, 0, None, None, 0, 21, None, None, None) == 0                  # empty sets: a clean return
    assert lib.s3d_eval_lp_max(None, None, 0, None, None, 0, 513, None, None, None) == _lib.ERR_INVALID
    assert lib.s3d_eval_pack_volumes(None, 0, 100, None, None) == 0 and lib.s3d_eval_pairwise_counts(None, 0, 2, None, None, None) == 0
    from sin3dm_amd.evaluation import patch_utils as pu
    assert pu.candidate_counts((48, 40, 36), 6) == (17, 14, 13) and pu.n_words(11) == 21 and pu.n_words(4) == 1 and pu.n_words(32) == 512
    assert pu.pooled_shape((40, 33, 25), 32) == (32, 26, 20) and pu.pooled_shape((128, 104, 88), 128) == (128, 104, 88)
    with pytest.raises(AssertionError, match="patch_size"):
        pu.candidate_counts((48, 40, 36), 40)


def test_procedural_volumes_regenerate():
    g = golden("eval_geometry")
    assert os.path.getsize(os.path.join(REPO, "tests", "golden", "eval_geometry.npz")) < 100 * 1024
    for name, (shape, _, _) in E.VOLUMES.items():
        s = E.sdf(name)
        assert s.shape == shape and s.dtype == np.float32
        assert [int((s <= 0).sum()), int((s < 0).sum())] == g[f"volumes/{name}"].tolist(), name
    for case, (ref_name, gens, *_rest, reso) in E.LP_CASES.items():
        if reso == max(E.VOLUMES[ref_name][0]):                                    # not pooled: the recorded occupancy is the formula's
            assert int(E.reference_occupancy(ref_name).sum()) == int(g[f"{case}/ref/count"])
            for i, name in enumerate(gens):
                assert int(E.generated_occupancy(name, ref_name).sum()) == int(g[f"{case}/gen{i}/count"])
    assert np.array_equal(E.generated_occupancy("ref32", "ref32"), E.reference_occupancy("ref32"))


def test_private_stream_reproduces_the_recorded_permutations():
    from sin3dm_amd.evaluation import shuffled_choice
    g = golden("eval_geometry")
    random.seed(99)
    state = random.getstate()
    for case, (_, gens, _, _, patch_num, _) in E.LP_CASES.items():
        rng = random.Random(1234)                                                  # one stream per run, carried from shape to shape
        for i in range(len(gens)):
            n_valid = len(g[f"{case}/gen{i}/valid"])
            chosen = shuffled_choice(rng, n_valid, patch_num)
            assert len(chosen) == min(n_valid, patch_num)
            assert np.array_equal(chosen, g[f"{case}/gen{i}/chosen"]), (case, i)
    assert random.getstate() == state                                              # the global stream is untouched
    assert len(g["p11_48/gen0/valid"]) > 300 and len(g["p11_32/gen0/valid"]) < 1000      # both sides of patch_num are covered


def test_cli_defaults(tmp_path):
    from sin3dm_amd.evaluation import eval_geometry as eg
    a = eg.parse_args(["-s", "gen", "-r", "ref"])
    assert (a.src, a.ref, a.patch_size, a.stride, a.patch_num, a.output) == ("gen", "ref", 11, 5, 1000, None)
    b = eg.parse_args(["--src", "g", "--ref", "r", "--patch_size", "6", "--stride", "3", "--patch_num", "10", "-o", "x.json"])
    assert (b.patch_size, b.stride, b.patch_num, b.output) == (6, 3, 10, "x.json")
    with pytest.raises(SystemExit):
        eg.parse_args(["-s", "gen"])
    for w in ("SSFID", "SIFID", "LPIPS", "offline"):
        assert w in eg.NOT_COMPUTED
    assert "\n" not in eg.NOT_COMPUTED
    (tmp_path / "src" / "b").mkdir(parents=True)
    (tmp_path / "src" / "a").mkdir()
    (tmp_path / "ref").mkdir()
    for p in ("src/b/voxel.npz", "src/a/r128_voxel.npz", "src/a/other.npz", "ref/z.npz", "ref/m.npz"):
        (tmp_path / p).write_bytes(b"")
    gen, ref = eg.find_inputs(str(tmp_path / "src"), str(tmp_path / "ref"))
    assert [os.path.relpath(p, tmp_path) for p in gen] == ["src/a/r128_voxel.npz", "src/b/voxel.npz"] and ref.endswith("m.npz")
    with pytest.raises(FileNotFoundError):
        eg.find_inputs(str(tmp_path / "ref"), str(tmp_path / "ref"))


def test_no_gpu_is_refused_loudly(tmp_path, monkeypatch):
    import sin3dm_amd.evaluation as ev
    from sin3dm_amd.evaluation import eval_geometry as eg
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    np.savez(tmp_path / "voxel.npz", vox_grid=np.zeros((4, 4, 4), dtype=bool))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ev.load_voxgrid(str(tmp_path / "voxel.npz"))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ev.extract_valid_patches(torch.zeros(8, 8, 8, dtype=torch.bool), 6)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        eg.main(["-s", str(tmp_path), "-r", str(tmp_path), "-o", str(tmp_path / "out.json")])
    assert not (tmp_path / "out.json").exists()
