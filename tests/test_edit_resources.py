"""CPU-only: the known-region instantiations of the output head (k_out_head_px<CQ, true, CARRY, true>, s3d_kernels.hip; DESIGN.md
section 20) keep to the budget of the default ones — no scratch memory, no vector or scalar spills — read from the code-object
metadata the way test_pbr_resources.py reads the decoder's.  The kernel is built for three blocks of 256 threads per CU: 168 vector
registers (512 / 3 at the allocation granularity of 8) and a third of the CU's 160 KiB of LDS.  The widths in use (64 and 128 channels,
CQ = 16 and 32) are held to that; the 256-channel instantiation is held to the figures of its default counterpart, which already
needs more than 168 registers and more than a third of the LDS for its staging area and runs one block per CU with or without the
blend."""
import os
import re
import subprocess

import pytest

from test_kernel_resources import CSRC, HIPCC, _kernel_metadata, _makefile_flags

KEYS = ("vgpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count")


@pytest.fixture(scope="module")
def head_kernels(tmp_path_factory):
    if not os.access(HIPCC, os.X_OK):
        pytest.skip("no hipcc")
    out = tmp_path_factory.mktemp("edit_res") / "s3d_kernels.s"
    r = subprocess.run([HIPCC, *_makefile_flags(), "--cuda-device-only", "-S", os.path.join(CSRC, "s3d_kernels.hip"), "-o", str(out)],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    # k_out_head_px<CQ, FUSED, CARRY, KNOWN> -> k_out_head_px_CQ_F_C_K (the helper keys kernels by their plain name)
    asm = re.sub(r"_ZN3s3d13k_out_head_pxILi(\d+)ELb(\d)ELb(\d)ELb(\d)EEEv\w+", r"k_out_head_px_\1_\2_\3_\4", out.read_text())
    return _kernel_metadata(asm)


@pytest.mark.parametrize("carry", [0, 1])
@pytest.mark.parametrize("cq", [16, 32, 64])
def test_known_region_head_instantiations_keep_the_budget(head_kernels, cq, carry):
    name, base = f"k_out_head_px_{cq}_1_{carry}_1", f"k_out_head_px_{cq}_1_{carry}_0"
    assert name in head_kernels and base in head_kernels, sorted(k for k in head_kernels if "out_head_px" in k)
    m, b = head_kernels[name], head_kernels[base]
    print(name, {k: m.get(k) for k in KEYS}, "| default:", {k: b.get(k) for k in KEYS})
    assert m["private_segment_fixed_size"] == 0, (name, m)
    assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (name, m)
    assert m["max_flat_workgroup_size"] == 256, (name, m)
    assert m["group_segment_fixed_size"] == b["group_segment_fixed_size"], (name, m, b)
    if cq <= 32:
        assert m["vgpr_count"] <= 168 and 3 * m["group_segment_fixed_size"] <= 160 * 1024, (name, m)      # three blocks per CU
    else:
        assert m["vgpr_count"] <= b["vgpr_count"], (name, m, b)


def test_default_head_instantiations_are_still_there(head_kernels):
    for cq in (16, 32, 64):
        for fused, carry in ((0, 0), (1, 0), (1, 1)):
            m = head_kernels[f"k_out_head_px_{cq}_{fused}_{carry}_0"]
            assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0, (cq, fused, carry, m)
