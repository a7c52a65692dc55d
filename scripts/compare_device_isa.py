#!/usr/bin/env python3
"""Is the device code of some kernel files the same in two revisions?  (CPU only: hipcc cross-compiles.)

    scripts/compare_device_isa.py --base HEAD pa_h1_hex pa_rt_hex ...

For every named file of palace_amd/csrc the base revision (checked out into a temporary directory) and the working tree are
compiled to assembly with `--cuda-device-only -S` and the flags the Makefile of that tree gives the file's object (taken from
`make -n`, so per-file flags are included).  Required per file:
  * the same set of kernel symbols,
  * for every kernel the same text from its label to `.end_amdhsa_kernel` (code and kernel descriptor; the function's position
    in the file is taken out of its local labels and of the comments that name them),
  * for every kernel the same entry in the `amdhsa.kernels` metadata (registers, spills, scratch, LDS, kernarg size).
Text is compared for equality only; the names of the kernels that differ are printed.  Exit status 1 on any difference.
"""
import argparse
import concurrent.futures
import os
import re
import shlex
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join("palace_amd", "csrc")


def compile_cmd(tree, name):
    """The Makefile's compile line for build/<name>.o, turned into a device-only assembly listing on stdout."""
    out = subprocess.run(["make", "-C", os.path.join(tree, CSRC), "-n", "-B", f"build/{name}.o"], check=True,
                         capture_output=True, text=True).stdout
    line = next(l for l in out.splitlines() if f"{name}.hip" in l and " -c " in l)
    words = shlex.split(line)
    i = words.index("-o")
    del words[i:i + 2]
    words[words.index("-c")] = "-S"
    return words + ["--cuda-device-only", "-o", "-"]


def listing(tree, name):
    cmd = compile_cmd(tree, name)
    res = subprocess.run(cmd, cwd=os.path.join(tree, CSRC), check=True, capture_output=True, text=True)
    return " ".join(cmd), res.stdout


def kernels(asm):
    """name -> (text from the label to .end_amdhsa_kernel, metadata entry)"""
    lines = asm.splitlines()
    if "amdhsa.kernels:" not in lines:  # a file of host code only
        return {}
    names = [m.group(1) for l in lines if (m := re.match(r"\s*\.amdhsa_kernel\s+(\S+)", l))]
    start, wanted = {}, set(names)
    for i, l in enumerate(lines):
        m = re.match(r"(\S+):", l)
        if m and m.group(1) in wanted and m.group(1) not in start:
            start[m.group(1)] = i
    text = {}
    for n in names:
        j = start[n]
        while not lines[j].strip().startswith(".end_amdhsa_kernel"):
            j += 1
        # local labels carry the function's position in the file (.LBB<function>_<block>): drop it, so that adding or removing
        # another kernel does not make every kernel after it differ
        # (the assembler's loop comments name the same blocks without the dot, `Header=BB37_3`, and are aligned behind the label)
        text[n] = re.sub(r"(\.LBB|\.Lfunc_end|\bBB)\d+", r"\1", "\n".join(lines[start[n]:j + 1]))
        text[n] = re.sub(r"[ \t]+;", " ;", text[n])
    # metadata: the items of the amdhsa.kernels list
    meta, i = {}, lines.index("amdhsa.kernels:") + 1
    item = []
    while i < len(lines) and (lines[i].startswith("  ") or not lines[i].strip()):
        if lines[i].startswith("  - ") and item:
            meta[_name(item)] = "\n".join(item)
            item = []
        item.append(lines[i])
        i += 1
    if item:
        meta[_name(item)] = "\n".join(item)
    return {n: (text[n], meta.get(n)) for n in names}


def _name(item):
    return next(m.group(1) for l in item if (m := re.match(r"\s+(?:- )?\.name:\s+(\S+)", l)))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--base", default="HEAD", help="revision to compare the working tree against")
    ap.add_argument("-j", type=int, default=4, help="compilations at a time")
    ap.add_argument("files", nargs="+", help="names under palace_amd/csrc without .hip")
    args = ap.parse_args()
    rev = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", args.base], check=True, capture_output=True,
                         text=True).stdout.strip()
    print("command: scripts/compare_device_isa.py --base " + args.base + " " + " ".join(args.files))
    print(f"base {rev} against the working tree")
    bad = 0
    with tempfile.TemporaryDirectory() as tmp:
        ar = subprocess.run(["git", "-C", ROOT, "archive", args.base, CSRC, "include"], check=True, capture_output=True).stdout
        subprocess.run(["tar", "-x", "-C", tmp], input=ar, check=True)
        with concurrent.futures.ThreadPoolExecutor(args.j) as pool:
            jobs = {n: (pool.submit(listing, tmp, n), pool.submit(listing, ROOT, n)) for n in args.files}
            for n, (fb, fw) in jobs.items():
                (cmd_b, asm_b), (cmd_w, asm_w) = fb.result(), fw.result()
                kb, kw = kernels(asm_b), kernels(asm_w)
                same = [k for k in kb if k in kw and kb[k] == kw[k]]
                print(f"{n}: {len(kb)} kernels in the base, {len(kw)} in the working tree, {len(same)} identical")
                print(f"  flags: {cmd_w}")
                if cmd_b != cmd_w:
                    print(f"  flags of the base: {cmd_b}")
                for k in sorted(set(kb) ^ set(kw)):
                    print(f"  only in {'the base' if k in kb else 'the working tree'}: {k}")
                for k in kb:
                    if k in kw and kb[k] != kw[k]:
                        what = [w for w, a, b in (("text", kb[k][0], kw[k][0]), ("metadata", kb[k][1], kw[k][1])) if a != b]
                        print(f"  differs ({', '.join(what)}): {k}")
                bad += len(set(kb) | set(kw)) - len(same)
    print("all identical" if bad == 0 else f"{bad} kernels differ")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
