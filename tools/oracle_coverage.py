#!/usr/bin/env python3
"""Which lines and branches of the C restatement do the golden fixtures execute?

Developer aid (no test runs it).  Builds oracle/noahmp_oracle.c with
`-O0 --coverage` into a temporary directory, runs every single-call fixture
once (a grouped fixture: every group), and every step of every trajectory
fixture through it, then reads
`gcov -b`: line and branch percentages, the lines never executed and the
branch directions never taken.  The parity claim of the project is only as
wide as this coverage: a branch no reference-generated fixture takes is
pinned to nothing (tests/golden/make_branch_golden.py and make_layers_golden.py
exist to close those).

  python tools/oracle_coverage.py                 # every fixture
  python tools/oracle_coverage.py --skip branch_  # without the branch_*.npz fixtures
  python tools/oracle_coverage.py --branches      # also list the untaken branch directions
"""
from __future__ import annotations

import argparse
import glob
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import noahmp_pkg  # noqa: E402,F401
import port  # noqa: E402
from golden_io import GOLDEN, fixture_params, layer_group, layer_groups, load  # noqa: E402

SRC = os.path.join(ROOT, "oracle", "noahmp_oracle.c")


def run_launch(name, g):
    """One single-call fixture (or group) once, or every step of a trajectory."""
    P, opts = fixture_params(g), tuple(g["options"])
    common = (g["zsoil"], float(g["dt"]), int(g["yearlen"]))
    if "states" in g:
        st, isn = g["state0"], g["isnow0"]
        for s in range(g["forcing"].shape[0]):
            # the day each fixture's generator and test give step s (fp32 arithmetic
            # for the branch and layers trajectories, as the engine's time loop advances it)
            if name.startswith(("branch_", "layers_")):
                jul = float(g["julian0"] + np.float32(s) * g["dt"] / np.float32(86400.0))
            else:
                jul = float(g["julian0"]) + s * float(g["dt"]) / 86400.0
            st, isn, _, _ = port.step(P, opts, *common, jul, st, isn, g["static_f"],
                                      g["static_i"], g["forcing"][s])
    else:
        port.step(P, opts, *common, float(g["julian"]), g["state0"], g["isnow0"],
                  g["static_f"], g["static_i"], g["forcing"])


def run_fixtures(skip):
    n = 0
    for path in sorted(glob.glob(os.path.join(GOLDEN, "*.npz"))):
        name = os.path.basename(path)
        if any(name.startswith(s) for s in skip):
            continue
        g = load(name)
        if "state0" not in g:
            continue
        # a grouped fixture (tests/golden/make_layers_golden.py) is several launches,
        # each with its own zsoil, dt, yearlen and julian
        for q in ([layer_group(g, k) for k in layer_groups(g)] if "group" in g else [g]):
            run_launch(name, q)
        n += 1
    return n


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--skip", action="append", default=[],
                    help="leave out fixtures whose file name starts with this (repeatable)")
    ap.add_argument("--branches", action="store_true", help="list the untaken branch directions")
    ap.add_argument("--run", metavar="LIB", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.run:
        port.LIBS[4] = a.run
        print(run_fixtures(a.skip))
        return
    with tempfile.TemporaryDirectory(prefix="oracle_cov_") as d:
        lib = os.path.join(d, "liboracle_cov.so")
        obj = os.path.join(d, "noahmp_oracle.o")
        subprocess.run(["gcc", "-O0", "--coverage", "-fPIC", "-ffp-contract=off", "-std=c11", "-w",
                        "-DORACLE_REAL=float", "-I", os.path.join(ROOT, "oracle"), "-c", "-o", obj,
                        SRC], check=True, cwd=d)
        subprocess.run(["gcc", "--coverage", "-shared", "-o", lib, obj, "-lm"], check=True, cwd=d)
        # the counters are written when the process that loaded the library exits
        child = subprocess.run([sys.executable, os.path.abspath(__file__), "--run", lib]
                               + [x for s in a.skip for x in ("--skip", s)], check=True,
                               capture_output=True, text=True)
        n = int(child.stdout.split()[-1])
        out = subprocess.run(["gcov", "-b", "-c", "-o", obj, SRC], cwd=d, check=True,
                             capture_output=True, text=True).stdout
        text = open(os.path.join(d, "noahmp_oracle.c.gcov")).read().splitlines()
    m = re.search(r"File '[^']*noahmp_oracle\.c'\n((?:.+\n)+)", out)
    print(f"{n} fixtures run")
    print(m.group(1).rstrip() if m else out)
    missed, untaken, line = [], [], 0
    for t in text:
        head = t.split(":", 2)
        if len(head) == 3 and head[1].strip().isdigit():
            line = int(head[1])
            if head[0].strip() in ("#####", "====="):
                missed.append((line, head[2].rstrip()))
        elif t.startswith("branch") and ("taken 0" in t or "never executed" in t):
            untaken.append((line, t.strip()))
    print(f"\n{len(missed)} lines never executed:")
    for ln, src in missed:
        print(f"  {ln:5d}: {src.strip()}")
    print(f"\n{len(untaken)} branch directions never taken")
    if a.branches:
        for ln, b in untaken:
            print(f"  {ln:5d}: {b}")


if __name__ == "__main__":
    main()
