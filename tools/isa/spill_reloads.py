#!/usr/bin/env python3
"""Does a kernel read spilled scalar registers back inside its loops?

  tools/isa/spill_reloads.py file.s kernel_mangled_name [...]

file.s: a `hipcc -S --cuda-device-only` listing (the product's command: poreover_amd/build.py --cmd OBJECT).  A spilled SGPR
lives in a lane of a VGPR: the VGPRs that `v_writelane_b32 vK, sN, lane` writes are the spill registers, and every
`v_readlane_b32 sN, vK, lane` from one of them is a reload.  Per kernel: the spill VGPRs, and per basic block that lies in a
loop (tools/isa/blocks.py --depth: depth >= 1) the reloads and the spill writes in it."""
import os
import re
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))


def main():
    path = sys.argv[1]
    lines = open(path).read().split("\n")
    for k in sys.argv[2:]:
        start = next(i for i, l in enumerate(lines) if l.startswith(k + ":"))
        end = next(i for i in range(start, len(lines)) if lines[i].strip().startswith("s_endpgm"))
        body = lines[start:end]
        spill = set(re.findall(r"v_writelane_b32 (v\d+), s\d+, \d+", "\n".join(body)))
        census = subprocess.run([sys.executable, os.path.join(HERE, "blocks.py"), path, k, "--depth"], capture_output=True, text=True).stdout
        in_loop = {}
        for l in census.split("\n"):
            m = re.search(r"(\.LBB\d+_\d+)\s+L\s+\d+ n=\s*(\d+).*depth=(\d+)(.*)", l)
            if m and int(m.group(3)) >= 1:
                in_loop[m.group(1)] = (int(m.group(2)), m.group(4).strip())
        cur, per = None, {}
        for l in body:
            m = re.match(r"^(\.LBB\d+_\d+):", l)
            if m:
                cur = m.group(1)
                continue
            if cur in in_loop:
                r = re.search(r"v_readlane_b32 s\d+, (v\d+), \d+", l)
                w = re.search(r"v_writelane_b32 (v\d+), s\d+, \d+", l)
                c = per.setdefault(cur, [0, 0])
                c[0] += bool(r and r.group(1) in spill)
                c[1] += bool(w)
        name = subprocess.run(["c++filt", k], capture_output=True, text=True).stdout.strip() or k
        print("## %s\nspill VGPRs: %s; reloads in loop blocks: %d; spill writes in loop blocks: %d" %
              (name, ", ".join(sorted(spill)) or "none", sum(c[0] for c in per.values()), sum(c[1] for c in per.values())))
        for b, (r, w) in per.items():
            if r or w:
                print("  %-12s n=%4d reloads=%3d writes=%3d %s" % (b, in_loop[b][0], r, w, in_loop[b][1]))


if __name__ == "__main__":
    main()
