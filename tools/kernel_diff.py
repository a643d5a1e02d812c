#!/usr/bin/env python3
"""Are the device kernels of two built trees the same machine code?  No GPU needed.

  python tools/kernel_diff.py OTHER_TREE [THIS_TREE]

For every object under rnnoise_amd/csrc/build of both trees that holds gfx950 code: the kernel names, per kernel the metadata of
llvm-readelf --notes (registers, spills, LDS, scratch, kernarg size) and the disassembled instruction sequence, mnemonics and
operands.  A kernel whose instructions differ only in branch targets is reported as such and counts as equal.  Exit status 0: no
kernel differs.  What a refactor of host code or of a kernel's source text has to show before its speed needs no measuring."""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from test_kernel_budgets_cpu import LLVM, _code_object  # noqa: E402

META = ("agpr_count", "vgpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size",
        "group_segment_fixed_size", "kernarg_segment_size", "max_flat_workgroup_size", "wavefront_size")


def kernels(tree):
    """{object: ({kernel: metadata}, {kernel: [instruction text]})} of a built tree"""
    build, out = os.path.join(tree, "rnnoise_amd", "csrc", "build"), {}
    for name in sorted(n for n in os.listdir(build) if n.endswith(".o")):
        with tempfile.TemporaryDirectory() as td:
            try:
                co = _code_object(os.path.join(build, name), td)
            except subprocess.CalledProcessError:
                continue  # a host-only object
            if not os.path.exists(co) or not os.path.getsize(co):
                continue
            notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", co], capture_output=True, text=True, check=True).stdout
            dis = subprocess.run([f"{LLVM}/llvm-objdump", "-d", co], capture_output=True, text=True, check=True).stdout
        meta = {}
        for blk in notes.split("- .agpr_count:")[1:]:
            blk = ".agpr_count:" + blk
            meta[re.search(r"\.name:\s*(\S+)", blk)[1]] = {k: (re.search(rf"\.{k}:\s*(\S+)", blk) or [None, None])[1] for k in META}
        code, cur = {}, None
        for ln in dis.splitlines():
            m = re.match(r"^[0-9a-f]+ <(\w+)>:", ln)
            if m:
                cur = m.group(1)
                code[cur] = []
            elif cur and "\t" in ln and ln.split("//")[0].strip():
                code[cur].append(re.sub(r"\s+", " ", ln.split("//")[0].strip()))
        out[name] = (meta, code)
    return out


def main():
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2] if len(sys.argv) > 2 else ROOT)
    no_targets = lambda c: [re.sub(r"^(s_c?branch\w*|s_call\w*) .*", r"\1", i) for i in c]
    total = bad = 0
    for obj in sorted(set(a) | set(b)):
        (ma, ca), (mb, cb) = a.get(obj, ({}, {})), b.get(obj, ({}, {}))
        for k in sorted(set(ma) | set(mb)):
            total += 1
            if k not in ma or k not in mb:
                verdict = "ONLY IN ONE TREE"
            elif ma[k] != mb[k]:
                verdict = "METADATA DIFFERS: " + ", ".join(f"{f} {ma[k][f]} / {mb[k][f]}" for f in META if ma[k][f] != mb[k][f])
            elif ca[k] == cb[k]:
                verdict = "identical"
            elif no_targets(ca[k]) == no_targets(cb[k]):
                verdict = "identical but for branch targets"
            else:
                first = next((i for i, (x, y) in enumerate(zip(ca[k], cb[k])) if x != y), min(len(ca[k]), len(cb[k])))
                verdict = f"CODE DIFFERS from instruction {first} ({len(ca[k])} / {len(cb[k])} instructions)"
            bad += not verdict.startswith("identical")
            m = mb.get(k) or ma[k]
            print(f"{obj:18s} {k:28s} {len(cb.get(k) or ca.get(k, [])):6d} instr  vgpr {m['vgpr_count']:>3} sgpr {m['sgpr_count']:>3} "
                  f"lds {m['group_segment_fixed_size']:>6} scratch {m['private_segment_fixed_size']:>3}  {verdict}")
    print(f"{total} kernels, {bad} differ")
    return bad != 0 or total == 0


if __name__ == "__main__":
    sys.exit(main())
