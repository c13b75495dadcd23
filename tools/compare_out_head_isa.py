#!/usr/bin/env python3
"""Is the output head of the default path still the kernel it was?  Compiles sin3dm_amd/csrc/s3d_kernels.hip of the working tree and
of a git revision to gfx950 assembly (device side only, the Makefile's flags) and compares the instructions of every
k_out_head_px<CQ, FUSED, CARRY, KNOWN> and k_out_head_px_ms<CQ, CARRY> instantiation (the DPM-Solver++ multistep update, DESIGN.md
section 26: the same body, s3d_out_head_px_body.h) line by line, comments stripped (tools/compare_kdecode_isa.py does the same for
k_decode): all twenty-one must keep their code, and none may appear or go.  Exit status 1 on a
difference (the differing line counts and the first differing line are printed).  Also prints registers, LDS, scratch and spills of
the k_out_head_px_ms instantiations next to their default counterparts.  Run it after touching the body or changing the compiler.

    python tools/compare_out_head_isa.py [REV]        # REV defaults to HEAD~1
"""
import os
import re
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "sin3dm_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
KEYS = ("vgpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count")


def assembly(csrc, tmp, tag):
    out = os.path.join(tmp, tag + ".s")
    subprocess.check_call([HIPCC, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-fvisibility=hidden", "-S", "--cuda-device-only",
                           os.path.join(csrc, "s3d_kernels.hip"), "-o", out], stderr=subprocess.DEVNULL)
    return open(out).read().split("\n")


def kernels(lines, prefix):
    out = {}
    for i, l in enumerate(lines):
        if l.startswith(prefix) and ":" in l:
            e = next(k for k in range(i, len(lines)) if ".end_amdhsa_kernel" in lines[k] or lines[k].startswith(".Lfunc_end"))
            # (labels carry the function's number in the file, which moves when a kernel is added in front: .LBB37_3 -> .LBB_3)
            out[l.split(":")[0]] = [re.sub(r"\.LBB\d+_", ".LBB_", x.split(";")[0].rstrip()) for x in lines[i:e] if not x.strip().startswith(";")]
    return out


def metadata(lines, name_re):
    text = "\n".join(lines)
    meta = text[text.index("amdhsa.kernels:"):]
    out = {}
    for entry in re.split(r"^  - ", meta, flags=re.M)[1:]:
        sym = re.search(r"^\s+\.name:\s+(\S+)", entry, re.M)
        if sym and re.match(name_re, sym.group(1)):
            out[sym.group(1)] = {k: int(v) for k, v in re.findall(r"^\s+\.(\w+):\s+(\d+)\s*$", entry, re.M)}
    return out


def main():
    rev = sys.argv[1] if len(sys.argv) > 1 else "HEAD~1"
    with tempfile.TemporaryDirectory() as tmp:
        # the revision's source beside the revision's own headers (the body is one of them)
        tar = subprocess.check_output(["git", "-C", REPO, "archive", rev, "sin3dm_amd/csrc", "include"])
        subprocess.run(["tar", "-x", "-C", tmp], input=tar, check=True)
        a, b = assembly(os.path.join(tmp, "sin3dm_amd", "csrc"), tmp, "old"), assembly(CSRC, tmp, "new")
    ka, kb = ({**kernels(x, "_ZN3s3d13k_out_head_pxI"), **kernels(x, "_ZN3s3d16k_out_head_px_msI")} for x in (a, b))
    same = sorted(ka) == sorted(kb)
    for k in sorted(ka):
        eq = kb.get(k) == ka[k]
        same &= eq
        note = ""
        if not eq and k in kb:
            d = next((i for i, (x, y) in enumerate(zip(ka[k], kb[k])) if x != y), min(len(ka[k]), len(kb[k])))
            note = f" ({len(kb[k])} lines now; first difference at line {d}: {ka[k][d:d + 1]} -> {kb[k][d:d + 1]})"
        print(f"{k}: {len(ka[k])} lines, {'identical' if eq else 'DIFFERENT' + note}")
    ma, mb = (metadata(x, r"_ZN3s3d1[36]k_out_head_px(_ms)?I") for x in (a, b))
    for k in sorted(ma):
        if ma[k] != mb.get(k):
            print(f"{k}: metadata {[ma[k].get(x) for x in KEYS]} -> {[mb.get(k, {}).get(x) for x in KEYS]}")
    for k in sorted(mb):
        if "_ms" in k:
            cq, carry = re.search(r"_msILi(\d+)ELb(\d)E", k).groups()
            base = next(v for n, v in mb.items() if re.search(rf"k_out_head_pxILi{cq}ELb1ELb{carry}ELb0E", n))
            print(f"k_out_head_px_ms<{cq}, {carry}>: " + ", ".join(f"{x} {mb[k].get(x)} ({base.get(x)})" for x in KEYS) + "   (default counterpart in parentheses)")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
