"""CPU-only: the decoder's fused gather + MLP-heads point kernel (k_decode in s3d_decoder.hip) keeps its operands, hidden
tiles and outputs in registers in every instantiation — no scratch memory, no spills, blocks of 256 — read from the
code-object metadata the way test_kernel_resources.py reads the Winograd kernels' budgets."""
import os
import re
import subprocess

import pytest

from test_kernel_resources import CSRC, HIPCC, _kernel_metadata, _makefile_flags

INSTANCES = ((2, 8), (1, 1), (1, 8), (1, 2), (3, 4))       # (up tiles, hidden tiles) of run_decode's ladder
SMALL = ("k_inorm_keep", "k_plane_to_nchw")


def test_decode_heads_kernels_use_no_scratch(tmp_path):
    if not os.access(HIPCC, os.X_OK):
        pytest.skip("no hipcc")
    out = tmp_path / "s3d_decoder.s"
    r = subprocess.run([HIPCC, *_makefile_flags(), "--cuda-device-only", "-S", os.path.join(CSRC, "s3d_decoder.hip"), "-o", str(out)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    # template instantiations: k_decode<U, H> -> k_decode_U_H (the helper keys kernels by their plain name)
    asm = re.sub(r"_ZN3s3d8k_decodeILi(\d+)ELi(\d+)EEEvNS_10DecodeArgsE", r"k_decode_\1_\2", out.read_text())
    kernels = _kernel_metadata(asm)
    for upt, hidt in INSTANCES:
        name = f"k_decode_{upt}_{hidt}"
        assert name in kernels, sorted(kernels)
        m = kernels[name]
        print(name, {k: m.get(k) for k in ("vgpr_count", "agpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size")})
        assert m["private_segment_fixed_size"] == 0, (name, m)
        assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (name, m)
        assert m["max_flat_workgroup_size"] == 256, (name, m)
        assert m["group_segment_fixed_size"] == 2 * hidt * 32 * 36 * 4, (name, m)       # two weight slabs of [hidden][36] floats
        assert m["vgpr_count"] <= 512 and m["group_segment_fixed_size"] <= 160 * 1024, (name, m)
    for name in SMALL:
        assert name in kernels, sorted(kernels)
        m = kernels[name]
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (name, m)
