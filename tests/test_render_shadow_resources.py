"""CPU-only: the kernels of s3d_ray.hip use no scratch memory, spill nothing, hold no LDS and are bounded to 256
threads — read from the code-object metadata as test_sparse_mc_resources.py reads its kernels.  The walk indexes nothing by the
axis it steps along: three named scalars per quantity, so that nothing becomes a private array."""
import os
import subprocess

import pytest

from test_kernel_resources import CSRC, HIPCC, _kernel_metadata, _makefile_flags

KERNELS = ("k_mesh_ray_occluded", "k_render_shadow_mask", "k_render_shade_pbr_lit")


def test_ray_kernels_use_no_scratch(tmp_path):
    if not os.access(HIPCC, os.X_OK):
        pytest.skip("no hipcc")
    out = tmp_path / "s3d_ray.s"
    r = subprocess.run([HIPCC, *_makefile_flags(), "--cuda-device-only", "-S", os.path.join(CSRC, "s3d_ray.hip"), "-o", str(out)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    kernels = _kernel_metadata(out.read_text())
    ours = sorted(k for k in kernels if k.startswith("k_"))
    assert ours == sorted(KERNELS), ours                                      # a new kernel of the file is listed here
    for name in KERNELS:
        m = kernels[name]
        print(name, {k: m[k] for k in ("vgpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size")})
        assert m["private_segment_fixed_size"] == 0, (name, m)
        assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (name, m)
        assert m["max_flat_workgroup_size"] == 256, (name, m)                  # __launch_bounds__ on every kernel
        assert m["group_segment_fixed_size"] == 0, (name, m)
