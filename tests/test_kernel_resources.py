"""CPU-only: the register budgets of the mixed-Winograd 3x3 kernels, read from the code-object metadata hipcc writes.

A CU's SIMD has 512 vector registers per lane: `__launch_bounds__(256, 3)` (three blocks of four waves per CU = three waves per
SIMD) leaves 512 / 3 = 170 -> 168 at the allocation granularity of 8, `(256, 2)` leaves 256.  A kernel over its budget still
builds and runs — it spills to scratch memory and runs 1.5x slower — and k_conv_wino24s sits AT 168: so the
budget is asserted here and not found by reading the ISA (README, round 4)."""
import os
import re
import shutil
import subprocess

import pytest

from conftest import REPO

CSRC = os.path.join(REPO, "sin3dm_amd", "csrc")
HIPCC = shutil.which("hipcc") or os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
VGPR_BUDGET = {"k_conv_wino24s": 168, "k_conv_wino24s_gnb": 168, "k_conv_wino24w": 256}


def _makefile_flags():
    with open(os.path.join(CSRC, "Makefile")) as f:
        text = f.read()
    arch = re.search(r"^ARCH\s*\?=\s*(\S+)", text, re.M).group(1)
    flags = re.search(r"^FLAGS\s*\?=\s*(.+)$", text, re.M).group(1)
    return flags.replace("$(ARCH)", arch).split()


def _kernel_metadata(asm):
    """{kernel name: {key: int}} from the amdhsa.kernels list of an assembly listing (one list entry per kernel)."""
    meta = asm[asm.index("amdhsa.kernels:"):]
    out = {}
    for entry in re.split(r"^  - ", meta, flags=re.M)[1:]:
        sym = re.search(r"^\s+\.name:\s+(\S+)", entry, re.M)
        if not sym:                        # (the amdhsa.version list that follows the kernels)
            continue
        name = re.match(r"_ZN3s3dL?\d+(k_\w+?)E", sym.group(1))      # L: a static kernel of a shared header
        out[name.group(1) if name else sym.group(1)] = {k: int(v) for k, v in re.findall(r"^\s+\.(\w+):\s+(\d+)\s*$", entry, re.M)}
    return out


def test_wino24_kernels_fit_their_launch_bounds_without_spilling(tmp_path):
    if not os.access(HIPCC, os.X_OK):
        pytest.skip("no hipcc")
    out = tmp_path / "s3d_wino24.s"
    r = subprocess.run([HIPCC, *_makefile_flags(), "--cuda-device-only", "-S", os.path.join(CSRC, "s3d_wino24.hip"), "-o", str(out)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    kernels = _kernel_metadata(out.read_text())
    for name, budget in VGPR_BUDGET.items():
        assert name in kernels, sorted(kernels)
        m = kernels[name]
        print(name, {k: m[k] for k in ("vgpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size")})
        assert m["private_segment_fixed_size"] == 0, (name, m)
        assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (name, m)
        assert m["vgpr_count"] <= budget, (name, m)
