"""Tabulates hipcc's -Rpass-analysis=kernel-resource-usage remarks of two builds side by side.

    make clean && make HIPFLAGS='-O3 --offload-arch=gfx950 -fPIC -std=c++17 -Iinclude -Rpass-analysis=kernel-resource-usage' 2> before.log
    (the same on the other tree)                                                                                            2> after.log
    python tools/resource_table.py before.log after.log [substring ...] > profiles/table.txt

Kernels are matched by their demangled name without the argument list (an added kernel argument changes the mangled name); with
substrings only the kernels whose name contains one of them are listed.  The exit status is 1 when a kernel gained scratch."""
import re
import subprocess
import sys

FIELDS = ("TotalSGPRs", "VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "SGPRs Spill", "VGPRs Spill",
          "LDS Size [bytes/block]")
SHORT = ("SGPR", "VGPR", "AGPR", "scratch", "occ", "sspill", "vspill", "LDS")


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    res = []
    for d in out[:len(names)]:
        d = d.replace("(anonymous namespace)::", "")
        d = re.sub(r"^void ", "", d)
        depth, cut = 0, len(d)
        for i, ch in enumerate(d):          # cut at the argument list: the first "(" outside template brackets
            if ch == "<":
                depth += 1
            elif ch == ">":
                depth -= 1
            elif ch == "(" and depth == 0:
                cut = i
                break
        res.append(d[:cut])
    return res


def parse(path):
    rows, order, cur = {}, [], {}     # cur: per source file, because a parallel make interleaves the compilers' output
    for line in open(path, errors="replace"):
        m = re.match(r"(\S+?):\d+:\d+: remark: Function Name: (\S+)", line)
        if m:
            cur[m.group(1)] = m.group(2)
            rows[m.group(2)] = {}
            order.append(m.group(2))
            continue
        m = re.match(r"(\S+?):\d+:\d+: remark:\s+(.*?): (\S+) \[-Rpass", line)
        if m and m.group(1) in cur and m.group(2) in FIELDS:
            rows[cur[m.group(1)]][m.group(2)] = m.group(3)
    names = demangle(order)
    return {n: rows[k] for n, k in zip(names, order)}


def main():
    before, after = parse(sys.argv[1]), parse(sys.argv[2])
    want = sys.argv[3:]
    bad = 0
    print(f"{'kernel':78s} " + " ".join(f"{s:>13s}" for s in SHORT) + "   (before -> after)")
    for name in sorted(set(before) | set(after)):
        if want and not any(w in name for w in want):
            continue
        b, a = before.get(name), after.get(name)
        cells = []
        for f in FIELDS:
            vb, va = (b or {}).get(f, "-"), (a or {}).get(f, "-")
            cells.append(f"{vb:>5s} -> {va:<4s}" if vb != va else f"{va:>13s}")
        flag = ""
        if a and int(a.get(FIELDS[3], "0")) > int((b or {}).get(FIELDS[3], "0")):
            flag, bad = "  GAINED SCRATCH", 1
        if b is None:
            flag += "  (new)"
        print(f"{name[:78]:78s} " + " ".join(cells) + flag)
    return bad


if __name__ == "__main__":
    sys.exit(main())
