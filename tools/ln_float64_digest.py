"""profiles/layernorm_float64.txt from the output of tests/test_ln_float64_gpu.py:

    python -m pytest -m gpu -s tests/test_ln_float64_gpu.py > ln64.log
    python tools/ln_float64_digest.py ln64.log profiles/layernorm_float64.txt

A full run prints about 5000 lines (K_yard, kernel, bound per case and quantity).  The profile is a digest of them on purpose: the
largest figure and the case closest to its bound per entry, format and quantity, over every line, and one line per test id at 8197 rows."""
import collections
import re
import sys

LINE = re.compile(r"^[.sFE]*\s+(\S+)( \+dres| twice)?\s+(\w+)\s+K_yard\s+([\d.]+)\s+kernel\s+([\d.]+)\s+bound\s+([\d.]+)\s*$")
ORDER = ["z", "y", "mean", "rstd", "dz", "dx_drop", "dgamma", "dbeta"]


def main(log, out):
    mx, big, n, wall, top = collections.OrderedDict(), collections.OrderedDict(), 0, None, (0.0, "")
    for ln in open(log):
        m = LINE.match(ln.rstrip("\n"))
        if m:
            n += 1
            tag, q, ky, k, K = m.group(1), m.group(3), float(m.group(4)), float(m.group(5)), float(m.group(6))
            key = ("f32 stream" if "stream" in tag else "plain + fused", tag.split("-")[0], q)
            e = mx.setdefault(key, [-1, 0, 0, "", -1, 0, 0, "", 0])
            e[8] += 1
            if k > e[0]:
                e[0:4] = [k, ky, K, tag]
            if k / K > e[4]:
                e[4:8] = [k / K, k, K, tag]
            if k / K > top[0]:
                top = (k / K, "%s of %s, %.3f of %.2f" % (q, tag, k, K))
            if "-8197x" in tag:                      # per id and quantity: the judge call that comes closest to its bound
                b = big.setdefault(tag, {})
                if q not in b or k / K > b[q][1] / b[q][2]:
                    b[q] = (ky, k, K)
        w = re.search(r"(\d+) passed.* in ([\d.]+)s", ln)
        if w:
            wall = (int(w.group(1)), float(w.group(2)))
    with open(out, "w") as f:
        f.write("tests/test_ln_float64_gpu.py on an MI355X (gfx950), one full run: f32 rows on the bfloat16 build, bfloat16 rows, IEEE-half rows on the\n"
                "IEEE-half build.  Per case and quantity the test prints K_yard = the largest err / (u A) of the float32 yardstick on the CPU, kernel = the\n"
                "same figure of the HIP kernel, bound = max(1, 4 K_yard) (tests/_ln_ref.py).  This run printed %d such lines over %d test ids, all\n"
                "passed; wall time of the file %.1f s (the float64 references on the host included).  This file is a digest of those lines on purpose\n"
                "(tools/ln_float64_digest.py makes it from the output of `pytest -m gpu -s`, which shows every line): the largest figures over all\n"
                "lines, then every id at 8197 rows.  No kernel figure exceeded its bound: the kernels of csrc/norm.hip are unchanged.\n"
                "The line that comes closest to its bound: %s (%.3f of it).\n\n" % ((n,) + wall + (top[1], top[0])))
        f.write("Largest kernel figure per entry, format and quantity (with the K_yard and bound of its case), and the case closest to its bound:\n")
        for key in sorted(mx, key=lambda k: (k[0], k[1], ORDER.index(k[2]))):
            e = mx[key]
            f.write("  %-13s %-5s %-7s %4d lines  largest %6.3f (K_yard %6.3f, bound %6.2f) %-34s closest %5.3f of %5.2f  %s\n"
                    % (key + (e[8], e[0], e[1], e[2], e[3], e[5], e[6], e[7])))
        f.write("\nEvery id at 8197 rows (three trips of the backward's row loop), K_yard / kernel / bound per quantity; where an id judges a quantity\n"
                "more than once (with and without dres, two calls into one buffer) the call closest to its bound:\n")
        for tag, b in big.items():
            f.write("  %-34s %s\n" % (tag, "  ".join("%s %.2f/%.2f/%.2f" % ((q,) + b[q]) for q in ORDER if q in b)))
    print("%d lines, %d ids in %.1f s, %d ids at 8197 rows" % ((n,) + wall + (len(big),)))


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
