#!/usr/bin/env python3
"""Static census of one whole instantiation of the fp32 step kernel, split by
the source file and, inside csrc/glibc_math.h, by the function each
instruction's line information names.

Compiles csrc/sflx_kernel.hip to gfx950 assembly with the engine's own flags
(build.FLAGS + build.SOURCE_FLAGS) plus -gline-tables-only, or reads such an
assembly file already made, and prints for one kernel (default
sflx_step_kernel<float, true, false, 5>, config #3's no-diagnostics kernel)

  instructions, VALU, SALU, conditional branches (s_cbranch_*) and IEEE fp32
  division sequences (v_div_fmas_f32: one per division)

in total, per source file, and per glibc_math.h function.  An inlined call's
instructions carry the line of the innermost inlined function, so the libm
restatements' share is what the `.loc` directives attribute to glibc_math.h.
Counts are static: one pass over the kernel, every branch arm counted once.

    python tools/kernel_census.py [--asm FILE] [--kernel IfLb1ELb0ELi5E] [--tree DIR]

profiles/libm_outloop/kernel_census.txt keeps the output for the parent and for
this tree.
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile
from collections import Counter, defaultdict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from loop_census import B, opcode  # noqa: E402  (the shared parser helpers and build flags)

KEYS = ["instructions", "VALU", "SALU", "cond. branches", "IEEE divisions"]


def compile_asm(tree, out):
    csrc = os.path.join(tree, "noahmp-1_amd", "csrc")
    flags = [f for f in B.FLAGS if f not in ("-shared", "-fPIC")]
    subprocess.run([B.HIPCC, *flags, *B.SOURCE_FLAGS["sflx_kernel.hip"], "-gline-tables-only",
                    '-DNMP_BUILD_HASH="kernelcensus0000"', "-I", os.path.join(tree, "include"),
                    "-I", csrc, "--offload-device-only", "-S", "-o", out,
                    os.path.join(csrc, "sflx_kernel.hip")], check=True)


def file_table(lines):
    """{file number: base name} from the .file directives."""
    files = {}
    for ln in lines:
        m = re.match(r'\s*\.file\s+(\d+)\s+"([^"]*)"(?:\s+"([^"]*)")?', ln)
        if m:
            files[int(m.group(1))] = os.path.basename(m.group(3) or m.group(2))
    return files


def located_instructions(lines, tag):
    """[(instruction text, file number, line)] of one kernel."""
    start = next(i for i, ln in enumerate(lines)
                 if re.match(r"^_ZN3nmp16sflx_step_kernel" + tag + r"\w*:", ln))
    out, loc = [], (0, 0)
    for ln in lines[start + 1:]:
        if ln.startswith(".Lfunc_end"):
            break
        m = re.match(r"\s*\.loc\s+(\d+)\s+(\d+)", ln)
        if m:
            loc = (int(m.group(1)), int(m.group(2)))
            continue
        t = ln.split(";")[0].strip()
        if t and not t.startswith(".") and not t.endswith(":"):
            out.append((t, *loc))
    return out


def gm_functions(tree):
    """[(first line, name)] of the function definitions of glibc_math.h."""
    defs = []
    path = os.path.join(tree, "noahmp-1_amd", "csrc", "glibc_math.h")
    for n, ln in enumerate(open(path), 1):
        m = re.match(r"^GM_HDM?\s+[\w:<>]+\s+(\w+)\s*\(", ln) or \
            re.match(r"^\s+GM_HDM\s+\w+\s+(operator\(\))", ln)
        if m:
            defs.append((n, m.group(1)))
    return defs


def function_at(defs, line):
    name = "(before the first function)"
    for first, fn in defs:
        if first > line:
            break
        name = fn
    return name


def tally(rows):
    c = Counter()
    for t, _, _ in rows:
        op = opcode(t)
        c["instructions"] += 1
        c["VALU"] += op.startswith("v_")
        c["SALU"] += op.startswith("s_") and op not in ("s_waitcnt", "s_nop")
        c["cond. branches"] += op.startswith("s_cbranch_")
        c["IEEE divisions"] += op == "v_div_fmas_f32"
    return c


def table(title, groups):
    print(f"{title:34s}" + "".join(f"{k:>16s}" for k in KEYS))
    for name, rows in sorted(groups.items(), key=lambda kv: -len(kv[1])):
        c = tally(rows)
        print(f"{name:34s}" + "".join(f"{c[k]:16d}" for k in KEYS))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--asm")
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--kernel", default="IfLb1ELb0ELi5E",
                    help="mangled template arguments (default <float,true,false,5>)")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as td:
        path = a.asm
        if not path:
            path = os.path.join(td, "k.s")
            compile_asm(a.tree, path)
        lines = open(path).read().splitlines()
    files = file_table(lines)
    ins = located_instructions(lines, a.kernel)
    if not any(f for _, f, _ in ins):
        raise SystemExit("no .loc directives: the assembly was made without -gline-tables-only")
    defs = gm_functions(a.tree)
    by_file, by_fn = defaultdict(list), defaultdict(list)
    for row in ins:
        name = files.get(row[1], f"(file {row[1]})")
        by_file[name].append(row)
        if name == "glibc_math.h":
            by_fn[function_at(defs, row[2])].append(row)
    print(f"kernel sflx_step_kernel{a.kernel}")
    table("whole kernel", {"total": ins})
    print()
    table("by source file", by_file)
    print()
    table("glibc_math.h by function", by_fn)


if __name__ == "__main__":
    main()
