#!/usr/bin/env python3
"""Static opcode census of the canopy Newton loop in the fp32 step kernel.

Compiles csrc/sflx_kernel.hip to gfx950 assembly with the engine's own flags
(build.FLAGS + build.SOURCE_FLAGS), or reads an assembly file already made, and
prints the instruction mix of the two canopy loops of one instantiation
(default sflx_step_kernel<float, true, false, 1>, config #3's kernel on output
steps; --kernel IfLb1ELb0ELi5E is its no-diagnostics copy, OS 1 | kNoDiag):

  fast  the DivFast32 loop: short divisions and the in-range libm cores
  ref   the DivRef loop a lane outside the proven domain re-runs: IEEE
        division and the full libm functions

    python tools/loop_census.py [--asm FILE] [--kernel IfLb1ELb0ELi1E] [--tree DIR]

A loop is a backward branch and the code it spans.  The canopy loops are the
two loops of 500 to 3000 instructions that hold the loop's reciprocals
(>= 15 v_rcp_f32: one per shared denominator, or one per IEEE sequence) and its
fp64 libm arithmetic (>= 10 v_fma_f64): the fast one has the fewest IEEE
sequences (v_div_scale_f32; none, in fact), the DivRef one is the next such
loop after it.  (Until the short divisions dropped their fix-up the loops were
found by their 30-odd v_div_fixup_f32; the fast loop now keeps two, EVC's and
TR's.)  "short quotients" counts the sequence q = a*r; e = fma(-b, q, a);
q' = fma(e, r, q) by its two fmas, "without fix-up" those of them whose q' no
v_div_fixup_f32 reads: DivFast32::divn.  Counts are static:
one pass over the loop body, every branch arm counted once.
profiles/libm_inrange/loop_census.txt keeps the output for the parent and for
this tree.
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile
from collections import Counter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import noahmp_pkg  # noqa: E402,F401
from noahmp_amd import build as B  # noqa: E402


def compile_asm(tree, out):
    csrc = os.path.join(tree, "noahmp-1_amd", "csrc")
    flags = [f for f in B.FLAGS if f not in ("-shared", "-fPIC")]
    subprocess.run([B.HIPCC, *flags, *B.SOURCE_FLAGS["sflx_kernel.hip"],
                    '-DNMP_BUILD_HASH="loopcensus000000"', "-I", os.path.join(tree, "include"),
                    "-I", csrc, "--offload-device-only", "-S", "-o", out,
                    os.path.join(csrc, "sflx_kernel.hip")], check=True)


def kernel_instructions(path, tag):
    """-> (instructions, {label: index of the next instruction}) of one kernel."""
    lines = open(path).read().splitlines()
    start = next(i for i, ln in enumerate(lines)
                 if re.match(r"^_ZN3nmp16sflx_step_kernel" + tag + r"\w*:", ln))
    ins, labels = [], {}
    for ln in lines[start + 1:]:
        if ln.startswith(".Lfunc_end"):
            break
        m = re.match(r"^(\.LBB\d+_\d+):", ln)
        if m:
            labels[m.group(1)] = len(ins)
            continue
        t = ln.split(";")[0].strip()
        if t and not t.startswith(".") and not t.endswith(":"):
            ins.append(t)
    return ins, labels


def loops(ins, labels):
    """Outermost extent per loop header: {start: end}."""
    ext = {}
    for i, t in enumerate(ins):
        m = re.match(r"s_c?branch\w*\s+(\.LBB\d+_\d+)", t)
        if m and labels.get(m.group(1), i + 1) <= i:
            a = labels[m.group(1)]
            ext[a] = max(ext.get(a, 0), i)
    return ext


def opcode(t):
    return re.sub(r"_(e32|e64|dpp|sdwa)$", "", t.split()[0])


def classify(op):
    if op.startswith("v_"):
        if re.match(r"v_(mov|cndmask|cmp|cmpx|readfirstlane|readlane|writelane)", op):
            return "VALU moves/selects/compares"
        if re.search(r"_(f64|b64|u64|i64)\b", op) or op.startswith("v_lshlrev_b64"):
            return "VALU 64-bit"
        if re.search(r"_f32\b", op):
            return "VALU f32"
        return "VALU integer/other"
    if op.startswith("s_"):
        if op in ("s_waitcnt", "s_nop"):
            return "waits"
        return "SALU"
    if op.startswith("ds_"):
        return "LDS"
    return "memory"


def short_quotients(body):
    """-> (short quotients, of them without a fix-up).  e = fma(-b, q, a) with a
    not the constant 1.0 (that is the reciprocal's own Newton step), then
    fma(e, r, q) -- as v_fma_f32 or the accumulating v_fmac_f32 -- before e or q
    is written again; with a fix-up when a v_div_fixup_f32 reads that result
    as its first source.  The IEEE sequence holds the same two fmas: there a
    v_div_fmas_f32 reads the result, and the pair is not counted.  A pattern
    count: a quotient whose registers the scheduler interleaves otherwise is
    missed (29 of the fast loop's 34 are found)."""
    fma = re.compile(r"v_fma_f32\s+(\S+), (\S+), (\S+), (\S+)$")
    fmac = re.compile(r"v_fmac_f32(?:_e32|_e64)?\s+(\S+), (\S+), (\S+)$")
    n = nofix = 0
    for i, t in enumerate(body):
        m = fma.match(t)
        if not m or not m.group(2).startswith("-") or m.group(4) in ("1.0", "-1.0"):
            continue
        e, q = m.group(1), m.group(3)
        for j in range(i + 1, min(i + 60, len(body))):
            u = body[j]
            m2, m3 = fma.match(u), fmac.match(u)
            if (m2 and e in m2.group(2, 3) and m2.group(4) == q) or \
                    (m3 and m3.group(1) == q and e in m3.group(2, 3)):
                res = m2.group(1) if m2 else q
                fixed = ieee = False
                for k in range(j + 1, min(j + 60, len(body))):
                    w = [x.rstrip(",") for x in body[k].split()]
                    if w[0].startswith("v_div_fmas_f32") and res in w[2:]:
                        ieee = True     # the IEEE sequence's own refinement step
                        break
                    if w[0].startswith("v_div_fixup_f32") and len(w) > 2 and w[2] == res:
                        fixed = True
                        break
                    if len(w) > 1 and w[1] == res:
                        break
                n += not ieee
                nofix += not ieee and not fixed
                break
            w = u.split()
            if len(w) > 1 and w[1].rstrip(",") in (e, q):
                break
    return n, nofix


def census(body):
    ops = Counter(opcode(t) for t in body)
    cls = Counter()
    for op, n in ops.items():
        cls[classify(op)] += n
    valu = sum(n for k, n in cls.items() if k.startswith("VALU"))
    const_moves = sum(1 for t in body if re.match(
        r"(s_mov_b32|s_mov_b64|v_mov_b32(_e32)?)\s+\S+\s+(0x[0-9a-fA-F]+|-?\d+(\.\d+)?)$", t))
    rows = [("instructions", len(body)), ("VALU", valu)]
    rows += [("  " + k[5:], cls[k]) for k in ("VALU f32", "VALU 64-bit",
                                               "VALU moves/selects/compares",
                                               "VALU integer/other")]
    rows += [("SALU", cls["SALU"]), ("LDS", cls["LDS"]), ("memory", cls["memory"]),
             ("waits", cls["waits"]),
             ("s_and_saveexec", sum(n for o, n in ops.items() if o.startswith("s_and_saveexec"))),
             ("s_cbranch_execz/execnz", ops["s_cbranch_execz"] + ops["s_cbranch_execnz"]),
             ("s_cbranch_scc/vcc", sum(n for o, n in ops.items()
                                       if re.match(r"s_cbranch_(scc|vcc)", o))),
             ("constant moves", const_moves),
             ("v_div_scale_f32", ops["v_div_scale_f32"]),
             ("v_div_fixup_f32", ops["v_div_fixup_f32"]),
             ("v_rcp_f32", ops["v_rcp_f32"]),
             ("v_fma_f64", ops["v_fma_f64"])]
    sq, nofix = short_quotients(body)
    rows += [("short quotients", sq), ("  without fix-up (divn)", nofix)]
    return rows


def canopy_loops(ins, labels):
    cand = []
    for a, b in loops(ins, labels).items():
        ops = Counter(opcode(t) for t in ins[a:b + 1])
        if 500 <= b - a + 1 <= 3000 and ops["v_rcp_f32"] >= 15 and ops["v_fma_f64"] >= 10:
            cand.append((ops["v_div_scale_f32"], a, b))
    fast = min(cand, default=None)
    after = sorted(c[1:] for c in cand if fast and c[1] > fast[2])
    if not after:
        raise SystemExit(f"canopy loops not found ({len(cand)} candidates)")
    return {"fast": fast[1:], "ref": after[0]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--asm")
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--kernel", default="IfLb1ELb0ELi1E",
                    help="mangled template arguments (default <float,true,false,1>)")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as td:
        path = a.asm
        if not path:
            path = os.path.join(td, "k.s")
            compile_asm(a.tree, path)
        ins, labels = kernel_instructions(path, a.kernel)
    found = canopy_loops(ins, labels)
    tabs = {k: census(ins[s:e + 1]) for k, (s, e) in found.items()}
    print(f"kernel sflx_step_kernel{a.kernel}: {len(ins)} instructions")
    print(f"{'':30s}{'fast loop':>12s}{'ref loop':>12s}")
    for (name, f), (_, r) in zip(tabs["fast"], tabs["ref"]):
        print(f"{name:30s}{f:12d}{r:12d}")
    # the fast loop's branches and what each skips: the wave-level skips of the
    # unstable blocks (MOZ < 0, MOZG < 0) and of the 2-m chain must be among them
    s, e = found["fast"]
    print("branches of the fast loop (offset, branch, instructions skipped, of them "
          "v_fma_f64 / LDS reads):")
    for i in range(s, e + 1):
        m = re.match(r"s_c?branch\w*\s+(\.LBB\d+_\d+)", ins[i])
        if not m:
            continue
        tgt = labels[m.group(1)]
        if tgt <= i:
            print(f"  {i - s:5d}  {ins[i].split()[0]:18s} back edge")
            continue
        ops = Counter(opcode(t) for t in ins[i + 1:tgt])
        print(f"  {i - s:5d}  {ins[i].split()[0]:18s} {tgt - i - 1:5d}  {ops['v_fma_f64']:3d} / "
              f"{sum(n for o, n in ops.items() if o.startswith('ds_read')):2d}")


if __name__ == "__main__":
    main()
