#!/usr/bin/env python3
"""Compare two device-assembly listings kernel by kernel: python tools/isa_diff.py <old.s> <new.s> [--quiet]

The listings come from the Makefile's CXXFLAGS plus `--cuda-device-only -S`.  Comment lines, the comment behind a label, `.ident`,
`.file` and lines that carry the per-compile `__hip_cuid_` symbol are dropped; what is left is cut at the global labels (one piece per kernel symbol,
with its descriptor and metadata lines) and each piece gets one of three results:
  identical         every line equal
  commutative only  same number of lines, and every differing line is a v_add_f64 / v_mul_f64 / v_fma_f64 with the same
                    destination whose first two sources are swapped (the same value, bit for bit)
  different         anything else; the first differing lines are shown
One line per kernel that is not identical, then a summary line.  Exit status 1 if any kernel is different."""
import re
import sys

COMMUTATIVE = ("v_add_f64", "v_mul_f64", "v_fma_f64")
LABEL = re.compile(r"^([^\s.;][^\s:]*):")


def kernels(path):
    """{symbol: [lines]} in file order; lines before the first global label go under '<header>'."""
    out, cur = {}, "<header>"
    out[cur] = []
    for raw in open(path):
        line = raw.rstrip()
        s = line.strip()
        if not s or s.startswith(";") or s.startswith(".ident") or s.startswith(".file") or "__hip_cuid_" in s:
            continue
        m = LABEL.match(line)
        if m:
            cur = m.group(1)
            out.setdefault(cur, [])
            s = s.split(";")[0].rstrip()       # (the "; @symbol" behind a label is padded to a column: a renamed symbol moves it)
        out[cur].append(s)
    return out


def swapped(a, b):
    """True if a and b are the same commutative fp64 instruction with sources 0 and 1 exchanged."""
    pa, pb = a.split(None, 1), b.split(None, 1)
    if len(pa) != 2 or len(pb) != 2 or pa[0] != pb[0] or not pa[0].startswith(COMMUTATIVE):
        return False
    oa, ob = [x.strip() for x in pa[1].split(",")], [x.strip() for x in pb[1].split(",")]
    if len(oa) != len(ob) or len(oa) < 3:
        return False
    return oa[0] == ob[0] and oa[1] == ob[2] and oa[2] == ob[1] and oa[3:] == ob[3:]


def compare(a, b):
    if a == b:
        return "identical", []
    diff = [(i, x, y) for i, (x, y) in enumerate(zip(a, b)) if x != y]
    if len(a) == len(b) and all(swapped(x, y) for _, x, y in diff):
        return "commutative only", diff
    if len(a) != len(b):
        diff.append((min(len(a), len(b)), f"<{len(a)} lines>", f"<{len(b)} lines>"))
    return "different", diff


def main():
    args = [x for x in sys.argv[1:] if x != "--quiet"]
    quiet = len(args) != len(sys.argv) - 1
    if len(args) != 2:
        sys.exit(__doc__)
    old, new = kernels(args[0]), kernels(args[1])
    count = {"identical": 0, "commutative only": 0, "different": 0}
    for name in list(old) + [n for n in new if n not in old]:
        if name not in old or name not in new:
            res, diff = "different", [(0, "<present>" if name in old else "<absent>", "<present>" if name in new else "<absent>")]
        else:
            res, diff = compare(old[name], new[name])
        count[res] += 1
        if res == "identical":
            continue
        print(f"{res}: {name} ({len(diff)} lines differ)")
        if res == "different" and not quiet:
            for i, x, y in diff[:6]:
                print(f"    line {i}:\n      - {x}\n      + {y}")
    print(f"{count['identical']} identical, {count['commutative only']} commutative only, {count['different']} different")
    sys.exit(1 if count["different"] else 0)


if __name__ == "__main__":
    main()
