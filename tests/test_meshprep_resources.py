"""CPU-only: the kernels of the mesh preprocessing (s3d_meshsdf.hip) keep everything in registers — no scratch memory, no spills —
and only the winding-number kernel uses LDS, exactly its declared triangle tile; read from the code-object metadata like
test_texmesh_resources.py."""
import os
import re
import subprocess

import pytest

from test_kernel_resources import CSRC, HIPCC, _kernel_metadata, _makefile_flags

KERNELS = ("k_mesh_bin_count", "k_mesh_bin_fill", "k_mesh_closest", "k_mesh_winding", "k_mesh_face_areas", "k_mesh_sample_surface",
           "k_mesh_texture")


def test_meshsdf_kernels_use_no_scratch(tmp_path):
    if not os.access(HIPCC, os.X_OK):
        pytest.skip("no hipcc")
    src = open(os.path.join(CSRC, "s3d_meshsdf.hip")).read()
    tile_bytes = int(re.search(r"constexpr int kWindTile = (\d+);", src).group(1)) * 9 * 4      # the declared tile: triangles of nine floats
    assert "__shared__ float tile[kWindTile * 9]" in src
    out = tmp_path / "s3d_meshsdf.s"
    r = subprocess.run([HIPCC, *_makefile_flags(), "--cuda-device-only", "-S", os.path.join(CSRC, "s3d_meshsdf.hip"), "-o", str(out)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    kernels = _kernel_metadata(out.read_text())
    assert sorted(k for k in kernels if k.startswith("k_")) == sorted(KERNELS)
    for name in KERNELS:
        m = kernels[name]
        print(name, {k: m[k] for k in ("vgpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size")})
        assert m["private_segment_fixed_size"] == 0, (name, m)
        assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (name, m)
        assert m["group_segment_fixed_size"] == (tile_bytes if name == "k_mesh_winding" else 0), (name, m)
        assert m["max_flat_workgroup_size"] == 256, (name, m)              # __launch_bounds__ on every kernel
