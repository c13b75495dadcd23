"""CPU-only: the kernels of s3d_imgfeat.hip, those it instantiates from s3d_rowstats.h included, keep everything in registers —
no scratch memory, no VGPR or SGPR spills — use exactly the LDS their declared arrays take and carry their declared workgroup
size; read from the code-object metadata like test_ssfid_resources.py."""
import os
import re
import subprocess

import pytest

from test_kernel_resources import CSRC, HIPCC, _kernel_metadata, _makefile_flags

# kernel (as _kernel_metadata names it; the convolution is a template over the input mode, the shared Gram kernel over the channel
# count and the load)
KERNELS = ("k_if_convILi0", "k_if_convILi1", "k_if_convILi2", "k_if_pool", "k_rows_gramILi64", "k_rows_gramILi192", "k_rows_cov", "k_if_unit",
           "k_if_pairs", "k_if_lpips")


def test_imgfeat_kernels_use_no_scratch(tmp_path):
    if not os.access(HIPCC, os.X_OK):
        pytest.skip("no hipcc")
    src = open(os.path.join(CSRC, "s3d_imgfeat.hip")).read()
    hdr = open(os.path.join(CSRC, "s3d_rowstats.h")).read()

    def const(name):
        return int(re.search(r"constexpr int " + name + r" = (\d+);", src + hdr).group(1))

    threads, tile_m, ld, rows, pad = const("kIfThreads"), const("kIfTileM"), const("kIfLd"), const("kRsStage"), const("kRsPad")
    assert (threads, tile_m, const("kIfTileN"), const("kIfChunk")) == (256, 128, 64, 16) and ld >= 16 and ld % 4 == 0
    assert const("kRsThreads") == threads and const("kIfGramSpan") % rows == 0
    for decl in ("__shared__ float stage[2][kIfTileM * kIfLd]", "__shared__ double red[kIfThreads]"):
        assert decl in src, decl
    for decl in ("__shared__ float a[kRsStage * LD]", "constexpr int LD = C + kRsPad, NI = C / 16, Q = C / 4;"):
        assert decl in hdr, decl
    assert src.count("__shared__") == 2 and hdr.count("__shared__") == 1
    assert src.count("__global__") == 5 == src.count("__launch_bounds__(kIfThreads)")
    assert hdr.count("__global__") == 2 == hdr.count("__launch_bounds__(kRsThreads)")
    lds = {"k_if_pairs": threads * 8, "k_rows_gramILi64": rows * (64 + pad) * 4, "k_rows_gramILi192": rows * (192 + pad) * 4}
    for mode in range(3):
        lds[f"k_if_convILi{mode}"] = 2 * tile_m * ld * 4
    out = tmp_path / "s3d_imgfeat.s"
    r = subprocess.run([HIPCC, *_makefile_flags(), "--cuda-device-only", "-S", os.path.join(CSRC, "s3d_imgfeat.hip"), "-o", str(out)],
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
        assert m["max_flat_workgroup_size"] == threads, (name, m)
    assert max(lds.values()) <= 64 * 1024                                   # static LDS: at least two blocks fit a CU's 160 KB
    for mode in range(3):                                                   # two convolution blocks per SIMD's register file
        assert kernels[f"k_if_convILi{mode}"]["vgpr_count"] <= 256
