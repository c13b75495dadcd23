"""CPU-only: the kernels of s3d_ssfid.hip, those it instantiates from s3d_rowstats.h included, keep everything in registers — no
scratch memory, no VGPR or SGPR spills — use exactly the LDS their declared arrays take and carry their declared workgroup size;
read from the code-object metadata like test_eval_resources.py."""
import os
import re
import subprocess

import pytest

from test_kernel_resources import CSRC, HIPCC, _kernel_metadata, _makefile_flags

# kernel (as _kernel_metadata names it; the shared Gram kernel is a template over the channel count and the load): workgroup size
KERNELS = {"k_ssfid_l1": 256, "k_ssfid_mr": 64, "k_ssfid_l2": 256, "k_rows_gramILi32": 256, "k_rows_gramILi64": 256, "k_rows_cov": 256}


def test_ssfid_kernels_use_no_scratch(tmp_path):
    if not os.access(HIPCC, os.X_OK):
        pytest.skip("no hipcc")
    src = open(os.path.join(CSRC, "s3d_ssfid.hip")).read()
    hdr = open(os.path.join(CSRC, "s3d_rowstats.h")).read()

    def const(name):
        return int(re.search(r"constexpr int [^;]*\b" + name + r" = (\d+)[,;]", src + hdr).group(1))

    threads, c1, c2, taps, rows = const("kSfThreads"), const("kSfC1"), const("kSfC2"), const("kSfTaps"), const("kRsStage")
    tx, ty, tz = const("kSfTx"), const("kSfTy"), const("kSfTz")
    assert (threads, c1, c2, taps) == (256, 32, 64, 64) and const("kRsThreads") == 256 and const("kSfGramSpan") % rows == 0
    pad = const("kRsPad")
    halo = (2 * tx + 2) * (2 * ty + 2) * (2 * tz + 2)
    for decl in ("__shared__ float tile[kSfThreads * (kSfC1 + 1)]", "__shared__ double red[8][kSfC1][2]", "__shared__ f32x4 wl[kSfTaps * kSfC1 / 4]",
                 "__shared__ f32x4 halo[kSfHalo * 2]", "__shared__ double red[4][kSfC2][2]", "kSfHalo = kSfHx * kSfHy * kSfHz"):
        assert decl in src, decl
    for decl in ("__shared__ float a[kRsStage * LD]", "constexpr int LD = C + kRsPad, NI = C / 16, Q = C / 4;"):
        assert decl in hdr, decl
    assert src.count("__shared__") == 5 and hdr.count("__shared__") == 1
    lds = {"k_ssfid_l1": threads * (c1 + 1) * 4 + 8 * c1 * 2 * 8 + taps * c1 * 4,
           "k_ssfid_l2": halo * 2 * 16 + 4 * c2 * 2 * 8,
           "k_rows_gramILi32": rows * (32 + pad) * 4, "k_rows_gramILi64": rows * (64 + pad) * 4}
    assert src.count("__global__") == 3 == src.count("__launch_bounds__(kSfThreads)") + src.count("__launch_bounds__(64)")
    assert hdr.count("__global__") == 2 == hdr.count("__launch_bounds__(kRsThreads)")
    out = tmp_path / "s3d_ssfid.s"
    r = subprocess.run([HIPCC, *_makefile_flags(), "--cuda-device-only", "-S", os.path.join(CSRC, "s3d_ssfid.hip"), "-o", str(out)],
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
    assert max(lds.values()) == lds["k_ssfid_l2"] <= 64 * 1024            # static LDS: two blocks fit a CU's 160 KB
