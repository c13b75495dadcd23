"""CPU-only: the kernels of s3d_render_pbr.hip keep everything in registers — no scratch memory, no VGPR or SGPR spills, no LDS —
carry their declared workgroup size, leave room for at least four waves per SIMD (at most 128 VGPRs) and use the registers the
table of DESIGN.md §24 states; read from the code-object metadata like test_render_resources.py.  The shade kernel indexes its material table, which travels in the argument
block, per lane: that must stay a load from the argument block and never become a private copy."""
import os
import re
import subprocess

import pytest

from conftest import REPO
from test_kernel_resources import CSRC, HIPCC, _kernel_metadata, _makefile_flags

KERNELS = {"k_render_vertex_normals": 256, "k_render_face_tangents": 256, "k_render_shade_pbr": 256}


def test_pbr_render_kernels_use_no_scratch(tmp_path):
    if not os.access(HIPCC, os.X_OK):
        pytest.skip("no hipcc")
    # both shade kernels take the shared pieces from one header, and the new file is in the library's build list
    for name in ("s3d_render.hip", "s3d_render_pbr.hip"):
        assert '#include "s3d_render_dev.h"' in open(os.path.join(CSRC, name)).read(), name
    assert "s3d_render_pbr.hip" in open(os.path.join(CSRC, "Makefile")).read()
    out = tmp_path / "s3d_render_pbr.s"
    r = subprocess.run([HIPCC, *_makefile_flags(), "--cuda-device-only", "-S", os.path.join(CSRC, "s3d_render_pbr.hip"), "-o", str(out)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    kernels = _kernel_metadata(out.read_text())
    design = open(os.path.join(REPO, "DESIGN.md")).read()
    assert sorted(k for k in kernels if k.startswith("k_")) == sorted(KERNELS)
    for name, size in KERNELS.items():
        m = kernels[name]
        print(name, {k: m[k] for k in ("vgpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size")})
        assert m["private_segment_fixed_size"] == 0, (name, m)
        assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (name, m)
        assert m["group_segment_fixed_size"] == 0, (name, m)
        assert m["max_flat_workgroup_size"] == size, (name, m)
        assert m["vgpr_count"] <= 128, (name, m)
        # the table of DESIGN.md §24 states these numbers: | `kernel` | VGPR | SGPR | LDS | scratch |
        row = re.search(r"\| `" + name + r"` \| (\d+) \| (\d+) \| (\d+) \| (\d+) \|", design)
        assert row, name
        assert [int(x) for x in row.groups()] == [m["vgpr_count"], m["sgpr_count"], m["group_segment_fixed_size"], m["private_segment_fixed_size"]], \
            (name, row.groups(), m)
