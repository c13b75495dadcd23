"""CPU-only: the kernels of the narrow-band iso-surface extraction (s3d_mc_sparse.hip) use no scratch memory and
spill nothing, and every one is bounded to 256 threads — read from the code-object metadata as test_normal_bake_resources.py reads
its kernels.  LDS is allowed: k_mcs_flags stages a brick and its apron there (dynamic, plus a few words of its own), and the
compiler keeps k_mcs_verts' three coordinates there to index them by the edge axis, as it does for k_mc_verts."""
import os
import subprocess

import pytest

from test_kernel_resources import CSRC, HIPCC, _kernel_metadata, _makefile_flags

KERNELS = ("k_mcs_seed", "k_mcs_dilate", "k_mcs_fill", "k_mcs_fill_int", "k_mcs_newflag", "k_mcs_assign", "k_mcs_pending", "k_mcs_flags",
           "k_mcs_cell_ntri", "k_mcs_verts", "k_mcs_tris", "k_mcs_occupancy")
LDS_BUDGET = {"k_mcs_flags": 256, "k_mcs_verts": 256 * 3 * 4}                 # static bytes; every other kernel: none


def test_sparse_mc_kernels_use_no_scratch(tmp_path):
    if not os.access(HIPCC, os.X_OK):
        pytest.skip("no hipcc")
    out = tmp_path / "s3d_mc_sparse.s"
    r = subprocess.run([HIPCC, *_makefile_flags(), "--cuda-device-only", "-S", os.path.join(CSRC, "s3d_mc_sparse.hip"), "-o", str(out)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    kernels = _kernel_metadata(out.read_text())
    ours = sorted(k for k in kernels if k.startswith("k_mcs_"))
    assert ours == sorted(KERNELS), ours                                      # a new kernel of the file is listed here
    for name in KERNELS:
        m = kernels[name]
        print(name, {k: m[k] for k in ("vgpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size")})
        assert m["private_segment_fixed_size"] == 0, (name, m)
        assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (name, m)
        assert m["max_flat_workgroup_size"] == 256, (name, m)                  # __launch_bounds__ on every kernel
        assert m["group_segment_fixed_size"] <= LDS_BUDGET.get(name, 0), (name, m)
