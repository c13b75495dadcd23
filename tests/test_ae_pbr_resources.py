"""CPU-only: the kernels added for the PBR network's training tier — the input-norm backward (k_in_bwd_part / _fin / _apply), the
three-head point-gradient sum (k_add_slices3) and the three-plane keep-both norm (k_inorm_keep3) — use no scratch memory and
spill no register, read from the code-object metadata the way test_edit_resources.py reads the output head's."""
import os
import subprocess

import pytest

from test_kernel_resources import CSRC, HIPCC, _kernel_metadata, _makefile_flags

KEYS = ("vgpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count")
NEW = {"s3d_ae_kernels.hip": ("k_in_bwd_part", "k_in_bwd_fin", "k_in_bwd_apply", "k_add_slices3"),
       "s3d_decoder.hip": ("k_inorm_keep3",)}


@pytest.fixture(scope="module", params=sorted(NEW))
def listing(request, tmp_path_factory):
    if not os.access(HIPCC, os.X_OK):
        pytest.skip("no hipcc")
    src = request.param
    out = tmp_path_factory.mktemp("ae_pbr_res") / (src + ".s")
    r = subprocess.run([HIPCC, *_makefile_flags(), "--cuda-device-only", "-S", os.path.join(CSRC, src), "-o", str(out)],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    return src, _kernel_metadata(out.read_text())


def test_new_kernels_use_no_scratch_and_spill_nothing(listing):
    src, kernels = listing
    for name in NEW[src]:
        assert name in kernels, (name, sorted(k for k in kernels if k.startswith("k_in")))
        m = kernels[name]
        print(name, {k: m.get(k) for k in KEYS})
        assert m["private_segment_fixed_size"] == 0, (name, m)
        assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (name, m)
        assert m["max_flat_workgroup_size"] == 256, (name, m)        # __launch_bounds__(256) on each of them
