#!/usr/bin/env python3
"""Basic-block census of one kernel in a hipcc -S listing: per block the VALU / SALU / LDS / VMEM / scratch /
lane-move counts and the back edges (loops); --depth adds the totals per loop depth.
Usage: blocks.py file.s kernel_mangled_name [--min N] [--depth]"""
import re, sys
def main():
    path, kname = sys.argv[1], sys.argv[2]
    lines = open(path).read().split("\n")
    start = next(i for i, l in enumerate(lines) if l.startswith(kname + ":"))
    end = next(i for i in range(start, len(lines)) if lines[i].strip().startswith("s_endpgm"))
    blocks, cur = [], {"label": "entry", "line": start, "ins": []}
    for i in range(start + 1, end + 1):
        l = lines[i]
        m = re.match(r"^(\.LBB\d+_\d+):", l)
        if m:
            blocks.append(cur); cur = {"label": m.group(1), "line": i, "ins": []}
            continue
        s = l.strip()
        if not s or s.startswith(";") or s.startswith("."): continue
        cur["ins"].append(s)
    blocks.append(cur)
    idx = {b["label"]: k for k, b in enumerate(blocks)}
    tot = {}
    for k, b in enumerate(blocks):
        c = dict(valu=0, salu=0, lds=0, vmem=0, scr=0, lanemv=0, smem=0, wait=0)
        back = []
        for s in b["ins"]:
            op = s.split()[0]
            if op.startswith("scratch_"): c["scr"] += 1
            elif op.startswith("v_readlane") or op.startswith("v_writelane") or op.startswith("v_readfirstlane"): c["lanemv"] += 1; c["valu"] += 1
            elif op.startswith("v_"): c["valu"] += 1
            elif op.startswith("ds_"): c["lds"] += 1
            elif op.startswith("global_") or op.startswith("buffer_") or op.startswith("flat_"): c["vmem"] += 1
            elif op.startswith("s_load") or op.startswith("s_buffer") or op.startswith("s_dcache"): c["smem"] += 1
            elif op.startswith("s_waitcnt"): c["wait"] += 1; c["salu"] += 1
            elif op.startswith("s_"): c["salu"] += 1
            if op.startswith("s_cbranch") or op == "s_branch":
                t = s.split()[-1]
                if t in idx and idx[t] <= k: back.append(t)
        b["c"] = c; b["back"] = back
        for kk, v in c.items(): tot[kk] = tot.get(kk, 0) + v
    print("total", tot, "blocks", len(blocks))
    # natural loops: for a backward branch e -> h the body is h and every block that reaches e without passing h (a branch
    # whose body would take in the kernel's entry is no loop: h does not dominate e); the loops of one header are one loop;
    # loop depth of a block = the loops it lies in
    succ = [set() for _ in blocks]
    for k, b in enumerate(blocks):
        ends = False
        for s_ in b["ins"]:
            op = s_.split()[0]
            if op.startswith("s_cbranch") or op == "s_branch":
                t = s_.split()[-1]
                if t in idx: succ[k].add(idx[t])
        if b["ins"] and b["ins"][-1].split()[0] in ("s_branch", "s_endpgm", "s_setpc_b64"): ends = True
        if not ends and k + 1 < len(blocks): succ[k].add(k + 1)
    pred = [set() for _ in blocks]
    for k, ss in enumerate(succ):
        for t in ss: pred[t].add(k)
    bodies = {}
    for e, b in enumerate(blocks):
        for t in b["back"]:
            h = idx[t]
            body, todo = {h}, [e]
            while todo:
                x = todo.pop()
                if x in body: continue
                body.add(x); todo.extend(pred[x])
            if 0 not in body or h == 0: bodies[h] = bodies.get(h, set()) | body
    depth = [sum(1 for body in bodies.values() if k in body) for k in range(len(blocks))]
    if "--depth" in sys.argv:
        for d in sorted(set(depth)):
            sel = [b["c"] for k, b in enumerate(blocks) if depth[k] == d]
            print("depth %d: blocks %d valu %d (lane moves %d) salu %d lds %d vmem %d scratch %d" % (
                d, len(sel), sum(c["valu"] for c in sel), sum(c["lanemv"] for c in sel), sum(c["salu"] for c in sel),
                sum(c["lds"] for c in sel), sum(c["vmem"] for c in sel), sum(c["scr"] for c in sel)))
    mn = int(sys.argv[sys.argv.index("--min") + 1]) if "--min" in sys.argv else 0
    for k, b in enumerate(blocks):
        c = b["c"]
        if len(b["ins"]) >= mn or b["back"]:
            print(f"{k:4d} {b['label']:12s} L{b['line']:6d} n={len(b['ins']):4d} valu={c['valu']:4d} salu={c['salu']:4d} lds={c['lds']:3d} vmem={c['vmem']:3d} scr={c['scr']:2d} lane={c['lanemv']:3d} wait={c['wait']:2d} depth={depth[k]}" + (f"  BACK->{','.join(b['back'])}" if b["back"] else ""))
main()
