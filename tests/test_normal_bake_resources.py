"""CPU-only: the kernels of the baked normal map (s3d_tex.hip) keep everything in registers — no scratch memory, no
spills, no LDS — and are bounded to 256 threads, read from the code-object metadata as test_texmesh_resources.py reads the other
kernels of that file."""
import os
import subprocess

import pytest

from test_kernel_resources import CSRC, HIPCC, _kernel_metadata, _makefile_flags

KERNELS = ("k_normal_fill", "k_normal_texels", "k_tex_dilate_nearest")


def test_normal_bake_kernels_use_no_scratch(tmp_path):
    if not os.access(HIPCC, os.X_OK):
        pytest.skip("no hipcc")
    out = tmp_path / "s3d_tex.s"
    r = subprocess.run([HIPCC, *_makefile_flags(), "--cuda-device-only", "-S", os.path.join(CSRC, "s3d_tex.hip"), "-o", str(out)],
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
