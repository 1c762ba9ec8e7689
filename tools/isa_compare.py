#!/usr/bin/env python3
"""Kernel-by-kernel comparison of the gfx950 code of two builds of the library:

    python tools/isa_compare.py OLD.so NEW.so

Every kernel of OLD must exist in NEW with the same instructions (under its own name, or -- a template that gained a defaulted
parameter -- under a new name that only OLD's kernel maps to) (disassembled without addresses or encodings; branch targets
are printed relative to the kernel, so a kernel that moved inside its code object still compares equal).  Kernels only NEW has are
listed with their VGPR / AGPR / scratch use.  Exit status 1 if a kernel of OLD is missing or differs."""
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import check_isa  # noqa: E402

LLVM = check_isa.LLVM


def kernel_code(lib, tmp):
    """{kernel symbol: instruction text} over every code object of `lib`."""
    out = {}
    for co in check_isa.code_objects(lib, tmp):
        for name in check_isa.kernels(co, r"."):
            if name.endswith(".kd"):
                continue
            dis = subprocess.run([LLVM + "/llvm-objdump", "-d", "--no-show-raw-insn", "--no-leading-addr", co, "--disassemble-symbols=" + name],
                                 capture_output=True, text=True, check=True).stdout
            body = [l.split("//")[0].rstrip() for l in dis.splitlines()]
            body = [re.sub(r"<[^>]*\+0x[0-9a-f]+>", "", l) for l in body if l.strip() and l.strip() != "..." and not l.startswith(("/", "Disassembly", "<"))]
            out[name] = "\n".join(body)
    return out


def resources(lib, tmp):
    """{kernel: (vgpr, agpr, scratch bytes)} from the code objects' metadata notes."""
    res = {}
    for co in check_isa.code_objects(lib, tmp):
        notes = subprocess.run([LLVM + "/llvm-readelf", "--notes", co], capture_output=True, text=True).stdout
        for blk in re.split(r"-\s+\.agpr_count:", notes)[1:]:
            name = re.search(r"\.name:\s+(\S+)", blk)
            if not name:
                continue
            agpr = int(blk.split()[0])
            v = re.search(r"\.vgpr_count:\s+(\d+)", blk)
            sc = re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk)
            res[name.group(1)] = (int(v.group(1)) if v else -1, agpr, int(sc.group(1)) if sc else -1)
    return res


def main(old, new):
    with tempfile.TemporaryDirectory() as ta, tempfile.TemporaryDirectory() as tb:
        a = kernel_code(old, ta)
        b = kernel_code(new, tb)
        res = resources(new, tb)
    bad = 0
    same = 0
    renamed = {}
    for k in sorted(a):
        if k not in b:
            # a template that gained a defaulted parameter keeps its instantiations under a longer name: identical code under a new name is
            # the same kernel
            twin = [n for n in sorted(set(b) - set(a)) if b[n] == a[k] and n not in renamed]
            if twin:
                renamed[twin[0]] = k
                print("RENAMED  %s -> %s (identical instructions)" % (k, twin[0]))
                same += 1
                continue
            print("MISSING  %s" % k)
            bad += 1
        elif a[k] != b[k]:
            print("CHANGED  %s (%d -> %d instructions)" % (k, a[k].count("\n") + 1, b[k].count("\n") + 1))
            bad += 1
        else:
            same += 1
    for k in sorted(set(b) - set(a) - set(renamed)):
        v, ag, sc = res.get(k, (-1, -1, -1))
        print("NEW      %s (%d instructions; vgpr %d, agpr %d, scratch %d B)" % (k, b[k].count("\n") + 1, v, ag, sc))
    print("%s vs %s: %d kernels identical, %d missing or changed, %d new" % (os.path.basename(old), os.path.basename(new), same, bad, len(set(b) - set(a) - set(renamed))))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
