#!/usr/bin/env python3
"""Are a source file's kernels still the kernels they were?  Compiles sin3dm_amd/csrc/SOURCE of the working tree and of a git
revision to gfx950 assembly (device side only, the Makefile's flags; the revision is extracted beside its OWN headers) and compares
every kernel whose mangled name matches --kernels line by line, comments stripped and the numbers of block labels normalised (they
carry the function's position in the file).  Exit status 1 when a kernel differs, appears or goes; the first differing line is
printed.  --report prints registers, LDS, scratch and spills (the code object's metadata) of the working tree's kernels that match
it.  Run it after touching a kernel's file, a header it includes, or the compiler.

    python tools/compare_isa.py SOURCE.hip [--kernels REGEX] [--report REGEX] [REV]        # REV defaults to HEAD~1

    python tools/compare_isa.py s3d_decoder.hip --kernels k_decodeI --report k_decode_grad      # k_decode
    python tools/compare_isa.py s3d_kernels.hip --kernels 'k_out_head_px(_ms)?I' --report k_out_head_px_msI   # the output head (26)
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
KEYS = ("vgpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count")


def assembly(root, source, tmp, tag):
    out = os.path.join(tmp, tag + ".s")
    subprocess.check_call([HIPCC, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-fvisibility=hidden", "-S", "--cuda-device-only",
                           os.path.join(root, "sin3dm_amd", "csrc", source), "-o", out], stderr=subprocess.DEVNULL)
    return open(out).read().split("\n")


def metadata(lines):
    """{kernel symbol: {metadata key: number}} of the code object"""
    text = "\n".join(lines)
    out = {}
    for entry in re.split(r"^  - ", text[text.index("amdhsa.kernels:"):], flags=re.M)[1:]:
        sym = re.search(r"^\s+\.name:\s+(\S+)", entry, re.M)
        if sym:
            out[sym.group(1)] = {k: int(v) for k, v in re.findall(r"^\s+\.(\w+):\s+(\d+)\s*$", entry, re.M)}
    return out


def kernels(lines, names):
    out = {}
    for i, l in enumerate(lines):
        name = l.split(":")[0]
        if ":" in l and name in names:
            e = next(k for k in range(i, len(lines)) if ".end_amdhsa_kernel" in lines[k] or lines[k].startswith(".Lfunc_end"))
            out[name] = [re.sub(r"\.LBB\d+_", ".LBB_", x.split(";")[0].rstrip()) for x in lines[i:e] if not x.strip().startswith(";")]
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("source")
    ap.add_argument("--kernels", default="", help="compare the kernels whose mangled name contains a match (default: all)")
    ap.add_argument("--report", default=None, help="print the metadata of the kernels whose mangled name contains a match")
    ap.add_argument("rev", nargs="?", default="HEAD~1")
    args = ap.parse_intermixed_args()
    with tempfile.TemporaryDirectory() as tmp:
        tar = subprocess.check_output(["git", "-C", REPO, "archive", args.rev, "sin3dm_amd/csrc", "include"])
        subprocess.run(["tar", "-x", "-C", tmp], input=tar, check=True)
        a, b = assembly(tmp, args.source, tmp, "old"), assembly(REPO, args.source, tmp, "new")
    ma, mb = metadata(a), metadata(b)
    ka, kb = (kernels(x, {n for n in m if re.search(args.kernels, n)}) for x, m in ((a, ma), (b, mb)))
    for k in sorted(set(ka) | set(kb)):
        if k not in ka or k not in kb:
            print(f"{k}: {'GONE' if k in ka else 'NEW'}")
        elif ka[k] != kb[k]:
            d = next((i for i, (x, y) in enumerate(zip(ka[k], kb[k])) if x != y), min(len(ka[k]), len(kb[k])))
            print(f"{k}: {len(ka[k])} lines, DIFFERENT ({len(kb[k])} lines now; first difference at line {d}: {ka[k][d:d + 1]} -> {kb[k][d:d + 1]})")
        else:
            print(f"{k}: {len(ka[k])} lines, identical")
        if k in ka and k in kb and ma[k] != mb[k]:
            print(f"{k}: metadata {[ma[k].get(x) for x in KEYS]} -> {[mb[k].get(x) for x in KEYS]}")
    same = ka == kb and (len(kb) > 0 or not args.kernels)   # (a pattern that matches nothing compares nothing)
    print(f"{args.source} against {args.rev}: {len(kb)} kernels, {'all identical' if same else 'NOT the same'}")
    if args.report is not None:
        for k in sorted(mb):
            if re.search(args.report, k):
                print(f"{k}: " + ", ".join(f"{x} {mb[k].get(x)}" for x in KEYS))
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
