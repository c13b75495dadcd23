"""CPU-only: the kernels of the geometry evaluation (s3d_eval.hip) keep everything in registers — no scratch memory, no spills —
and use LDS only for their fixed-shape reductions over the workgroup's waves, exactly the declared arrays; read from the
code-object metadata like test_meshprep_resources.py."""
import os
import re
import subprocess

import pytest

from test_kernel_resources import CSRC, HIPCC, _kernel_metadata, _makefile_flags

KERNELS = ("k_eval_pool_or", "k_eval_patch_valid", "k_eval_pack_patches", "k_eval_lp_max", "k_eval_pack_volumes", "k_eval_pairwise_counts")


def test_eval_kernels_use_no_scratch(tmp_path):
    if not os.access(HIPCC, os.X_OK):
        pytest.skip("no hipcc")
    src = open(os.path.join(CSRC, "s3d_eval.hip")).read()
    threads = int(re.search(r"constexpr int kEvalThreads = (\d+);", src).group(1))
    lp_gen = int(re.search(r"constexpr int kLpGen = (\d+);", src).group(1))
    assert "constexpr int kEvalWaves = kEvalThreads / 64;" in src
    waves = threads // 64
    assert "__shared__ float red[kEvalWaves][kLpGen][2]" in src and "__shared__ int wave_count[kEvalWaves]" in src
    assert "__shared__ long long red[kEvalWaves][2]" in src
    lds = {"k_eval_lp_max": waves * lp_gen * 2 * 4, "k_eval_pack_patches": waves * 4, "k_eval_pairwise_counts": waves * 2 * 8}
    assert src.count("__global__") == len(KERNELS) == src.count("__launch_bounds__(kEvalThreads)")
    out = tmp_path / "s3d_eval.s"
    r = subprocess.run([HIPCC, *_makefile_flags(), "--cuda-device-only", "-S", os.path.join(CSRC, "s3d_eval.hip"), "-o", str(out)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    kernels = _kernel_metadata(out.read_text())
    assert sorted(k for k in kernels if k.startswith("k_")) == sorted(KERNELS)
    for name in KERNELS:
        m = kernels[name]
        print(name, {k: m[k] for k in ("vgpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size")})
        assert m["private_segment_fixed_size"] == 0, (name, m)
        assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (name, m)
        assert m["group_segment_fixed_size"] == lds.get(name, 0), (name, m)
        assert m["max_flat_workgroup_size"] == threads == 256, (name, m)           # __launch_bounds__ on every kernel
