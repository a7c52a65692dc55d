#!/usr/bin/env python3
"""Static instruction counts of a kernel's main loop in a `hipcc -S --cuda-device-only` listing, by class, and the registers /
scratch / LDS of its kernel descriptor.  The main loop is the widest span between a label and a backward branch to it, so the
loop-back block the compiler places ahead of the loop header (the register copies of the software pipeline) is part of it.
Instructions are classified by opcode prefix only:
  fp64    v_*_f64 (v_fma_f64, v_mul_f64, v_add_f64, v_pk_*_f64 ...)
  valu    every other v_*
  lds     ds_*
  salu    s_* that is neither a wait nor a nop (branches included)
  wait    s_waitcnt*, s_nop
  load    global_load* / buffer_load* / flat_load* / scratch_load*
  store   global_store* / buffer_store* / flat_store* / scratch_store*, atomics
usage: loop_isa_count.py listing.s regex-on-the-mangled-kernel-name"""
import re
import sys

CLASSES = ("fp64", "valu", "lds", "salu", "wait", "load", "store")


def classify(ins):
    op = ins.split()[0]
    if op.startswith("v_"):
        return "fp64" if op.endswith("_f64") or "_f64_" in op else "valu"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith(("s_waitcnt", "s_nop")):
        return "wait"
    if op.startswith("s_"):
        return "salu"
    if op.startswith(("global_", "buffer_", "flat_", "scratch_")):
        return "load" if "_load" in op else "store"
    return "other"


def main():
    txt = open(sys.argv[1]).read().split("\n")
    pat = re.compile(sys.argv[2])
    desc = {}  # kernel -> descriptor fields
    i = 0
    rows = []
    while i < len(txt):
        m = re.match(r"^(_Z\S+):\s", txt[i])
        if not m or not pat.search(m.group(1)):
            i += 1
            continue
        name, labels, ins, j = m.group(1), {}, [], i + 1
        while j < len(txt) and ".Lfunc_end" not in txt[j]:  # (the descriptor sits between the body and .Lfunc_end)
            ln = txt[j]
            j += 1
            dm = re.match(r"^\s*\.amdhsa_(next_free_vgpr|private_segment_fixed_size|group_segment_fixed_size)\s+(\S+)", ln)
            if dm:
                desc.setdefault(name, {})[dm.group(1)] = dm.group(2)
            lm = re.match(r"^(\.LBB\S+):", ln)
            if lm:
                labels[lm.group(1)] = len(ins)
                continue
            s = ln.strip()
            if s and not s.startswith((";", ".")):
                ins.append(s.split(";")[0].strip())
        best = None
        for k, s in enumerate(ins):
            bm = re.match(r"^s_c?branch\S*\s+(\.LBB\S+)", s)
            if bm and bm.group(1) in labels and labels[bm.group(1)] <= k:
                a = labels[bm.group(1)]
                if best is None or k - a > best[1] - best[0]:
                    best = (a, k)
        c = dict.fromkeys(CLASSES + ("other",), 0)
        if best:
            for s in ins[best[0]:best[1] + 1]:
                c[classify(s)] += 1
        rows.append((name, c, desc.get(name, {})))
        i = j
    for name, c, d in rows:
        print(name)
        print("  loop: " + "  ".join(f"{k} {c[k]}" for k in CLASSES) + (f"  other {c['other']}" if c["other"] else "") +
              f"  total {sum(c.values())}")
        print(f"  descriptor: vgpr {d.get('next_free_vgpr', '?')}  scratch {d.get('private_segment_fixed_size', '?')} B/lane"
              f"  static LDS {d.get('group_segment_fixed_size', '?')} B")


if __name__ == "__main__":
    main()
