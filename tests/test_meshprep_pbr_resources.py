"""CPU-only: the kernel of the PBR material lookup (s3d_meshpbr.hip) keeps everything in registers — no scratch memory, no spills,
no LDS — and is compiled for blocks of 256; read from the code-object metadata like test_meshprep_resources.py."""
import os
import subprocess

import pytest

from test_kernel_resources import CSRC, HIPCC, _kernel_metadata, _makefile_flags

KERNELS = ("k_mesh_texture_pbr",)


def test_meshpbr_kernel_uses_no_scratch_and_no_lds(tmp_path):
    if not os.access(HIPCC, os.X_OK):
        pytest.skip("no hipcc")
    with open(os.path.join(CSRC, "Makefile")) as fh:
        assert "s3d_meshpbr.hip" in fh.read()
    out = tmp_path / "s3d_meshpbr.s"
    r = subprocess.run([HIPCC, *_makefile_flags(), "--cuda-device-only", "-S", os.path.join(CSRC, "s3d_meshpbr.hip"), "-o", str(out)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    kernels = _kernel_metadata(out.read_text())
    assert sorted(k for k in kernels if k.startswith("k_")) == sorted(KERNELS)
    for name in KERNELS:
        m = kernels[name]
        print(name, {k: m[k] for k in ("vgpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size")})
        assert m["private_segment_fixed_size"] == 0, (name, m)
        assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (name, m)
        assert m["group_segment_fixed_size"] == 0, (name, m)
        assert m["max_flat_workgroup_size"] == 256, (name, m)              # __launch_bounds__
