#!/usr/bin/env python3
"""Static instruction counts of a kernel's main loop, from the disassembly kernel_resources.py writes.

    python profiles/scripts/kernel_resources.py --isa-dir DIR > /dev/null
    python profiles/scripts/loop_counts.py DIR SUBSTRING [MIN_X4_LOADS = 10]

For every kernel whose mangled name contains SUBSTRING: the innermost backward branch whose body holds at least
MIN_X4_LOADS 16-byte vector loads (the row loop of the dense passes over W; both trip forms of the loop are inside,
so the counts are per loop body, not per trip taken), and in it the vector loads, vector stores / atomics, LDS
operations, scalar loads, fp64 VALU, other VALU and other scalar instructions.
"""
import collections
import glob
import os
import re
import subprocess
import sys


def kernels(path, want):
    cur, ins = None, []
    for line in open(path):
        m = re.match(r"^[0-9a-f]+ <(.+)>:", line)
        if m:
            if cur:
                yield cur, ins
            cur, ins = None, []
            if want in m.group(1) and not m.group(1).endswith(".kd"):
                cur = m.group(1)
            continue
        if cur:
            m = re.match(r"\s+(\S+)\s.*//\s*([0-9A-Fa-f]+):", line)
            if m:
                ins.append((int(m.group(2), 16), m.group(1), line))
    if cur:
        yield cur, ins


def main_loop(ins, min_x4):
    at = {a: i for i, (a, _, _) in enumerate(ins)}
    best = None
    for i, (a, op, line) in enumerate(ins):
        if not (op.startswith("s_cbranch") or op == "s_branch"):
            continue
        m = re.search(r"<[^>]*\+0x([0-9a-f]+)>\s*$", line)
        if not m:
            continue
        t = ins[0][0] + int(m.group(1), 16)
        if t < a and t in at:
            s = at[t]
            nx4 = sum(1 for _, o, _ in ins[s:i + 1] if o == "global_load_dwordx4")
            if nx4 >= min_x4 and (best is None or i - s < best[1] - best[0]):
                best = (s, i)
    return None if best is None else ins[best[0]:best[1] + 1]


def classify(op):
    if op.startswith("global_load"):
        return "vector loads"
    if op.startswith("global_store") or op.startswith("global_atomic"):
        return "vector stores/atomics"
    if op.startswith("ds_"):
        return "LDS"
    if op.startswith("s_load"):
        return "scalar loads"
    if op.startswith("v_"):
        return "fp64" if "f64" in op else "other VALU"
    return "other scalar"


def main():
    isa_dir, want = sys.argv[1], sys.argv[2]
    min_x4 = int(sys.argv[3]) if len(sys.argv) > 3 else 10
    keys = ["vector loads", "vector stores/atomics", "LDS", "scalar loads", "fp64", "other VALU", "other scalar"]
    print("kernel,loop instructions," + ",".join(keys))
    for path in sorted(glob.glob(os.path.join(isa_dir, "*.s"))):
        for name, ins in kernels(path, want):
            dn = subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip()
            dn = re.sub(r"^void\s+", "", dn.split("(")[0]).replace("lbk::", "")
            body = main_loop(ins, min_x4)
            if body is None:
                print('"%s",no such loop' % dn)
                continue
            c = collections.Counter(classify(op) for _, op, _ in body)
            print('"%s",%d,' % (dn, len(body)) + ",".join(str(c[k]) for k in keys))


if __name__ == "__main__":
    main()
