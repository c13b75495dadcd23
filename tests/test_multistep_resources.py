"""CPU-only: the output head's instantiations with the DPM-Solver++ multistep update (k_out_head_px_ms<CQ, CARRY>, s3d_kernels.hip +
s3d_out_head_px_body.h) keep to the budget of the default ones, read from the code-object metadata the way
test_edit_resources.py reads the known-region ones: no private segment, no vector or scalar spills, the launch bound of 256, the same
LDS as the default instantiation of that CQ; at the widths in use (CQ = 16, 32) the 168 vector registers and the third of the CU's
160 KiB of LDS that three blocks per CU leave a block; at CQ = 64 (256 channels — exercised by this test only, no GPU test builds a
model that wide) no more vector registers than the default counterpart, which already runs one block per CU.  The fifteen
k_out_head_px instantiations must still be there under their names."""
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
    out = tmp_path_factory.mktemp("multistep_res") / "s3d_kernels.s"
    r = subprocess.run([HIPCC, *_makefile_flags(), "--cuda-device-only", "-S", os.path.join(CSRC, "s3d_kernels.hip"), "-o", str(out)],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    # k_out_head_px<CQ, FUSED, CARRY, KNOWN> -> k_out_head_px_CQ_F_C_K ; k_out_head_px_ms<CQ, CARRY> -> k_out_head_px_ms_CQ_C
    asm = re.sub(r"_ZN3s3d13k_out_head_pxILi(\d+)ELb(\d)ELb(\d)ELb(\d)EEEv\w+", r"k_out_head_px_\1_\2_\3_\4", out.read_text())
    asm = re.sub(r"_ZN3s3d16k_out_head_px_msILi(\d+)ELb(\d)EEEv\w+", r"k_out_head_px_ms_\1_\2", asm)
    return _kernel_metadata(asm)


@pytest.mark.parametrize("carry", [0, 1])
@pytest.mark.parametrize("cq", [16, 32, 64])
def test_multistep_head_instantiations_keep_the_budget(head_kernels, cq, carry):
    name, base = f"k_out_head_px_ms_{cq}_{carry}", f"k_out_head_px_{cq}_1_{carry}_0"
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


def test_all_fifteen_default_and_known_region_instantiations_are_still_there(head_kernels):
    names = [f"k_out_head_px_{cq}_{f}_{c}_{k}" for cq in (16, 32, 64) for f, c, k in ((0, 0, 0), (1, 0, 0), (1, 1, 0), (1, 0, 1), (1, 1, 1))]
    assert len(names) == 15
    for n in names:
        assert n in head_kernels, (n, sorted(k for k in head_kernels if "out_head_px" in k))
        assert head_kernels[n]["private_segment_fixed_size"] == 0 and head_kernels[n]["vgpr_spill_count"] == 0, (n, head_kernels[n])
    assert sum(1 for k in head_kernels if k.startswith("k_out_head_px_ms_")) == 6
    assert "k_sampler_multistep" in " ".join(head_kernels)
