#!/usr/bin/env python3
"""Are the kernels of two builds the same instruction streams?

  tools/isa/kernel_diff.py --emit DIR      compile every object of poreover_amd/build.py to DIR/OBJECT.s (the product's command
                                           + -S --cuda-device-only), for the tree this script lies in
  tools/isa/kernel_diff.py DIR_A DIR_B [OLD=NEW]   compare two such directories, kernel by kernel; OLD=NEW rewrites the mangled
                                           names of A first, for a type that was renamed (6X2Args=7RegArgs)

A kernel is the text from its symbol's label to its .Lfunc_end, without comments and blank lines, with `.LBB<n>_` written
`.LBB_` (n is the function's index in its file, so it moves when a kernel moves).  Kernels are matched by mangled name,
whichever file they are in; a name that several objects define (po_zero_kernel) is compared as the set of its bodies.  The
script compares lines: it looks at no instruction."""
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))


def emit(out):
    sys.path.insert(0, os.path.join(HERE, "..", "..", "poreover_amd"))
    import build as B
    os.makedirs(out, exist_ok=True)

    def one(oname):
        subprocess.check_call(B.compile_cmd(oname) + ["-S", "--cuda-device-only", "-o", os.path.join(out, oname + ".s")],
                              stderr=subprocess.DEVNULL)
    with ThreadPoolExecutor(8) as ex:
        list(ex.map(one, [o for o, _, _ in B.OBJECTS]))


def kernels(path):
    """{mangled name: [lines]} of one listing"""
    text = open(path).read()
    names = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M))
    out, cur, body = {}, None, []
    for line in text.split("\n"):
        line = line.split(";", 1)[0].rstrip()
        if cur is None:
            if line.endswith(":") and line[:-1] in names:
                cur, body = line[:-1], []
            continue
        if not line.strip():
            continue
        if re.match(r"\.Lfunc_end\d+:", line):
            out[cur] = body
            cur = None
            continue
        body.append(re.sub(r"\.LBB\d+_", ".LBB_", line))
    return out


def collect(d):
    """{mangled name: sorted list of (object, body)} over a directory of listings"""
    all_ = {}
    for f in sorted(os.listdir(d)):
        if f.endswith(".s"):
            for name, body in kernels(os.path.join(d, f)).items():
                all_.setdefault(name, []).append((f[:-2], body))
    return all_


def main():
    if len(sys.argv) == 3 and sys.argv[1] == "--emit":
        emit(sys.argv[2])
        return 0
    a, b = collect(sys.argv[1]), collect(sys.argv[2])
    if len(sys.argv) > 3:
        old, new = sys.argv[3].split("=")
        a = {name.replace(old, new): [(o, [line.replace(old, new) for line in body]) for o, body in v] for name, v in a.items()}
    same, differ = 0, []
    for name in sorted(set(a) | set(b)):
        if name not in a or name not in b:
            differ.append("only in %s  %s  (%s)" % ("A" if name in a else "B", name, ", ".join(o for o, _ in (a.get(name) or b.get(name)))))
        elif {tuple(x) for _, x in a[name]} != {tuple(x) for _, x in b[name]}:
            differ.append("DIFFERENT  %s  (A: %s, %s lines | B: %s, %s lines)" % (
                name, ", ".join(o for o, _ in a[name]), "/".join(str(len(x)) for _, x in a[name]),
                ", ".join(o for o, _ in b[name]), "/".join(str(len(x)) for _, x in b[name])))
        else:
            same += 1
    for o in sorted({o for v in list(a.values()) + list(b.values()) for o, _ in v}):
        na, nb = (sum(1 for v in t.values() for oo, _ in v if oo == o) for t in (a, b))
        print("%-28s kernels: A %3d  B %3d" % (o, na, nb))
    print("kernel names: A %d, B %d; identical: %d; different or unmatched: %d" % (len(a), len(b), same, len(differ)))
    for d in differ:
        print(d)
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
