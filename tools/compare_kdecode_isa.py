#!/usr/bin/env python3
"""Is k_decode still the kernel it was?  Compiles sin3dm_amd/csrc/s3d_decoder.hip of the working tree and of a git revision to
gfx950 assembly (device side only, the Makefile's flags) and compares the instructions of every k_decode<UPT,HIDT> instantiation
line by line, comments stripped.  k_decode_grad shares gather_plane and mlp_layer with k_decode; its mlp_layer instances carry
the GRAD tag because sharing the instances reordered k_decode's schedule, and the sdf it returns relies on
k_decode's arithmetic staying put.  Run it after touching that file or changing the compiler; exit status 1 on a difference.
Also prints scratch, spills and registers of the k_decode_grad instantiations.

    python tools/compare_kdecode_isa.py [REV]        # REV defaults to HEAD~1
"""
import os
import re
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "sin3dm_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def assembly(source_text, tmp, tag):
    src = os.path.join(CSRC, f".isa_{tag}.hip")          # beside the headers it includes
    out = os.path.join(tmp, tag + ".s")
    with open(src, "w") as fh:
        fh.write(source_text)
    try:
        subprocess.check_call([HIPCC, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-fvisibility=hidden", "-S", "--cuda-device-only",
                               src, "-o", out], stderr=subprocess.DEVNULL)
    finally:
        os.remove(src)
    return open(out).read().split("\n")


def kernels(lines, prefix):
    out = {}
    for i, l in enumerate(lines):
        if l.startswith(prefix) and ":" in l:
            e = next(k for k in range(i, len(lines)) if "s_endpgm" in lines[k])
            out[l.split(":")[0]] = [x.split(";")[0].rstrip() for x in lines[i:e] if not x.strip().startswith(";")]
    return out


def main():
    rev = sys.argv[1] if len(sys.argv) > 1 else "HEAD~1"
    old = subprocess.check_output(["git", "-C", REPO, "show", f"{rev}:sin3dm_amd/csrc/s3d_decoder.hip"], text=True)
    new = open(os.path.join(CSRC, "s3d_decoder.hip")).read()
    with tempfile.TemporaryDirectory() as tmp:
        a, b = assembly(old, tmp, "old"), assembly(new, tmp, "new")
    ka, kb = kernels(a, "_ZN3s3d8k_decodeI"), kernels(b, "_ZN3s3d8k_decodeI")
    same = sorted(ka) == sorted(kb)
    for k in sorted(ka):
        eq = kb.get(k) == ka[k]
        same &= eq
        print(f"{k}: {len(ka[k])} lines, {'identical' if eq else 'DIFFERENT'}")
    text = "\n".join(b)
    for name, priv, spill, vgpr in re.findall(r"\.name:\s+(_ZN3s3d13k_decode_grad\S+)\n\s+\.private_segment_fixed_size: (\d+)[\s\S]*?\.sgpr_spill_count: (\d+)[\s\S]*?\.vgpr_count:\s+(\d+)", text):
        print(f"{name}: scratch {priv} B, sgpr spills {spill}, registers {vgpr}")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
