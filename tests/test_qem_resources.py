"""CPU-only: the kernels of the quadric decimation (s3d_qem.hip) keep everything in registers — no scratch memory, no spills, no
LDS — read from the code-object metadata the way test_texmesh_resources.py reads s3d_tex.hip's.  The cost kernel holds ten
doubles of quadric, six cofactors and three points per thread; its register count is printed and bounded."""
import os
import subprocess

import pytest

from test_kernel_resources import CSRC, HIPCC, _kernel_metadata, _makefile_flags

KERNELS = ("k_qem_quadrics", "k_qem_edge_cost", "k_qem_frozen", "k_qem_edge_valid", "k_qem_fill_keys", "k_qem_vertex_min",
           "k_qem_neighbour_min", "k_qem_select", "k_qem_apply", "k_qem_remap_faces")


def test_qem_kernels_use_no_scratch(tmp_path):
    if not os.access(HIPCC, os.X_OK):
        pytest.skip("no hipcc")
    out = tmp_path / "s3d_qem.s"
    r = subprocess.run([HIPCC, *_makefile_flags(), "--cuda-device-only", "-S", os.path.join(CSRC, "s3d_qem.hip"), "-o", str(out)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    kernels = _kernel_metadata(out.read_text())
    for name in KERNELS:
        assert name in kernels, sorted(kernels)
        m = kernels[name]
        print(name, {k: m[k] for k in ("vgpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size")})
        assert m["private_segment_fixed_size"] == 0 and m["group_segment_fixed_size"] == 0, (name, m)
        assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (name, m)
        assert m["max_flat_workgroup_size"] == 256, (name, m)              # __launch_bounds__ on every kernel
        assert m["vgpr_count"] <= 128, (name, m)                           # four waves of 256 threads per SIMD stay resident
