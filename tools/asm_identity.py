#!/usr/bin/env python3
"""Device-assembly identity of two source trees, unit by unit.

  python tools/asm_identity.py emit TREE OUTDIR     # compile every unit of TREE to OUTDIR/*.s
  python tools/asm_identity.py record PARENT_DIR PR_DIR > profiles/..._asm_identity.txt

Units: each .hip of build.SOURCES with its own SOURCE_FLAGS, tests/routines.hip
with the flags of __graft_entry__.build(), and sflx_kernel.hip with the probe
library's flags (__graft_entry__._build_probe_midloop).  Every unit is compiled
with --offload-device-only -S and the same -DNMP_BUILD_HASH string, from inside
TREE with relative paths.  The lines naming the __hip_cuid_<hash> symbol (a hash
of the source text) are dropped before the text is hashed.
"""
import hashlib
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import noahmp_pkg  # noqa: E402,F401
from noahmp_amd import build as B  # noqa: E402

HASH = '-DNMP_BUILD_HASH="asmidentity00000"'
CSRC = os.path.join("noahmp-1_amd", "csrc")
INC = ["-I", "include", "-I", CSRC]
PROBE = ["-DNMP_COUNT_FALLBACK", "-DNMP_DOM_TV_HI=295.0", "-DNMP_DOM_TGB_HI=295.0",
         "-DNMP_DOM_RAHG_HI=300.0", "-DNMP_DOM_NUM_LO_EXP=2"]


def units():
    common = [f for f in B.FLAGS if f not in ("-shared", "-fPIC")]
    for src in B.SOURCES:
        if src.endswith(".hip"):
            yield src, os.path.join(CSRC, src), common + B.SOURCE_FLAGS[src] + [HASH]
    yield ("sflx_kernel.hip+probe", os.path.join(CSRC, "sflx_kernel.hip"),
           common + B.SOURCE_FLAGS["sflx_kernel.hip"] + PROBE + [HASH])
    yield ("tests/routines.hip", os.path.join("tests", "routines.hip"),
           ["-O3", f"--offload-arch={B.ARCH}", "-std=c++17", "-ffp-contract=off",
            "-mllvm", "-disable-machine-licm"])


def asm_name(unit):
    return unit.replace("/", "_").replace("+", "_") + ".s"


def emit(tree, outdir):
    os.makedirs(outdir, exist_ok=True)
    outdir = os.path.abspath(outdir)

    def one(u):
        unit, path, flags = u
        subprocess.run([B.HIPCC, *flags, *INC, "--offload-device-only", "-S", "-o",
                        os.path.join(outdir, asm_name(unit)), path], cwd=tree, check=True)
        print("emitted", unit, flush=True)

    with ThreadPoolExecutor(int(os.environ.get("MAX_JOBS", "0")) or os.cpu_count() or 1) as ex:
        list(ex.map(one, units()))


def filtered_sha(path):
    h = hashlib.sha256()
    n = 0
    with open(path, "rb") as f:
        for line in f:
            if b"__hip_cuid_" not in line:
                h.update(line)
                n += 1
    return h.hexdigest(), n


def record(parent_dir, pr_dir):
    same = True
    for unit, _, flags in units():
        if not os.path.exists(os.path.join(parent_dir, asm_name(unit))):
            b, nb = filtered_sha(os.path.join(pr_dir, asm_name(unit)))
            print(f"unit   {unit}\nflags  {' '.join(flags)}\nparent (no such unit)\n"
                  f"pr     {b} ({nb} lines)\nNEW\n")
            continue
        a, na = filtered_sha(os.path.join(parent_dir, asm_name(unit)))
        b, nb = filtered_sha(os.path.join(pr_dir, asm_name(unit)))
        same &= a == b
        print(f"unit   {unit}\nflags  {' '.join(flags)}\nparent {a} ({na} lines)\n"
              f"pr     {b} ({nb} lines)\n{'IDENTICAL' if a == b else 'DIFFERENT'}\n")
    return 0 if same else 1


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "emit":
        emit(sys.argv[2], sys.argv[3])
    elif len(sys.argv) == 4 and sys.argv[1] == "record":
        sys.exit(record(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
