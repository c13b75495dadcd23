"""CPU-only: the kernels of s3d_render.hip keep everything in registers — no scratch memory, no VGPR or SGPR spills — use exactly
the LDS their declared arrays take and carry their declared workgroup size; read from the code-object metadata like
test_ssfid_resources.py."""
import os
import re
import subprocess

import pytest

from test_kernel_resources import CSRC, HIPCC, _kernel_metadata, _makefile_flags

KERNELS = {"k_render_project": 256, "k_render_bin_count": 256, "k_render_bin_fill": 256, "k_render_raster": 256, "k_render_shade": 256}


def test_render_kernels_use_no_scratch(tmp_path):
    if not os.access(HIPCC, os.X_OK):
        pytest.skip("no hipcc")
    src = open(os.path.join(CSRC, "s3d_render.hip")).read()

    def const(name):
        return int(re.search(r"constexpr int [^;]*\b" + name + r" = (\d+)[,;]", src).group(1))

    threads, chunk = const("kRenderThreads"), const("kRasterChunk")
    assert (threads, chunk) == (256, 128)
    for decl in ("__shared__ long long sC[kRasterChunk][3]", "__shared__ int sAB[kRasterChunk][6]", "__shared__ float sW[kRasterChunk][4]",
                 "__shared__ int sMeta[kRasterChunk][2]", "constexpr int kRasterTile = S3D_RENDER_TILE;"):
        assert decl in src, decl
    assert src.count("__shared__") == 4
    lds = {"k_render_raster": chunk * (3 * 8 + 6 * 4 + 4 * 4 + 2 * 4)}
    assert lds["k_render_raster"] == 9216
    assert src.count("__global__") == 5 == src.count("__launch_bounds__(kRenderThreads)")
    out = tmp_path / "s3d_render.s"
    r = subprocess.run([HIPCC, *_makefile_flags(), "--cuda-device-only", "-S", os.path.join(CSRC, "s3d_render.hip"), "-o", str(out)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    kernels = _kernel_metadata(out.read_text())
    assert sorted(k for k in kernels if k.startswith("k_")) == sorted(KERNELS)
    for name, size in KERNELS.items():
        m = kernels[name]
        print(name, {k: m[k] for k in ("vgpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size")})
        assert m["private_segment_fixed_size"] == 0, (name, m)
        assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (name, m)
        assert m["group_segment_fixed_size"] == lds.get(name, 0), (name, m)
        assert m["max_flat_workgroup_size"] == size, (name, m)
