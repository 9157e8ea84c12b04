"""The in-range libm cores of csrc/glibc_math.h vs the host glibc float libm.

expf_inrange, logf_inrange, powf_inrange (y = +-0.25, the two exponents the
Newton loops use) and atanf_ge1 are the main paths of the full functions
without their special-case exits; the canopy and bare Newton loops call them
under DivFast32 (csrc/sflx_math.h MthInRange32) where tools/div_proof.py proves
the arguments in range.  Here each is compiled for the host (g++ and ROCm's
clang++, -ffp-contract=off) and compared bit for bit with libm over its
interval:

  expf    |x| < 88, both signs (zero and the subnormals included)
  logf    every positive normal finite x
  pow_q   powf(x, 0.25f), every positive normal finite x
  pow_mq  powf(x, -0.25f), the same
  atanf   1 <= x < 2^25

Default run: every bit pattern within +-4096 of each interval end and each
internal breakpoint (clipped to the interval), plus every 61st pattern of the
rest; atanf's interval (2.1e8 patterns) in full.  NMP_EXHAUSTIVE=1 checks every
float of every interval.  tests/test_gpu_libm_inrange.py runs the device build
over the same sets.
"""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "glibc_math_inrange_check.cpp")
NBHD = 4096


def bits(v):
    return int(np.array(v, np.float32).view(np.uint32))


_B88 = bits(88.0)
_NORMAL = (0x00800000, 0x7f7fffff)
# inclusive ranges of bit patterns
INTERVALS = {
    "expf": [(0x00000000, _B88 - 1), (0x80000000, 0x80000000 + _B88 - 1)],
    "logf": [_NORMAL], "pow_q": [_NORMAL], "pow_mq": [_NORMAL],
    "atanf": [(0x3f800000, 0x4c000000 - 1)],
}
# internal breakpoints: logf / powf: x = 1 and the 16 table subintervals from
# OFF = 0x3f330000 (index = bits 19..22 of ix - OFF); atanf: fdlibm's 19/16 and
# 39/16; expf: the subnormal border and |x| = 1 (it has no breakpoint of its own)
_TAB = [0x3f800000] + [0x3f330000 + (i << 19) for i in range(17)]
BREAKS = {
    "expf": [0x00800000, 0x3f800000, 0x80800000, 0xbf800000],
    "logf": _TAB, "pow_q": _TAB, "pow_mq": _TAB,
    "atanf": [0x3f980000, 0x401c0000],
}
STRIDE = {"expf": 61, "logf": 61, "pow_q": 61, "pow_mq": 61, "atanf": 1}
FUNCS = list(INTERVALS)


def ranges(fn, exhaustive=False):
    """[(first, count, stride)]: the neighbourhoods, then the strided rest."""
    stride = 1 if exhaustive else STRIDE[fn]
    out = []
    for lo, hi in INTERVALS[fn]:
        if stride > 1:
            for c in [lo, hi] + [b for b in BREAKS[fn] if lo <= b <= hi]:
                a, z = max(lo, c - NBHD), min(hi, c + NBHD)
                out.append((a, z - a + 1, 1))
        out.append((lo, (hi - lo) // stride + 1, stride))
    return out


def test_ranges_stay_inside_the_intervals():
    for fn in FUNCS:
        for ex in (False, True):
            for first, count, stride in ranges(fn, ex):
                last = first + (count - 1) * stride
                assert any(lo <= first and last <= hi for lo, hi in INTERVALS[fn]), (fn, first)
        if STRIDE[fn] > 1:  # both ends of every interval have their dense neighbourhood
            for lo, hi in INTERVALS[fn]:
                assert (lo, NBHD + 1, 1) in ranges(fn) and (hi - NBHD, NBHD + 1, 1) in ranges(fn)
    assert ranges("atanf") == [(0x3f800000, 0x4c000000 - 0x3f800000, 1)]


def _compilers():
    import noahmp_pkg  # noqa: F401
    from noahmp_amd import build
    llvm_bin = os.path.dirname(build.LLVM_MC)
    clang = os.path.join(llvm_bin, "clang++")
    libdir = os.path.join(os.path.dirname(llvm_bin), "lib")
    omp = ["-fopenmp", f"-Wl,-rpath,{libdir}"] if os.path.exists(
        os.path.join(libdir, "libomp.so")) else []
    return {"g++": ["g++", "-fopenmp"], "clang++": [clang, *omp]}


@pytest.fixture(scope="module", params=["g++", "clang++"])
def checker(request, tmp_path_factory):
    cmd = _compilers()[request.param]
    if not (os.path.exists(cmd[0]) or request.param == "g++"):
        pytest.fail(f"{cmd[0]} missing")
    exe = str(tmp_path_factory.mktemp("gmi") / "glibc_math_inrange_check")
    subprocess.run([*cmd, "-O2", "-ffp-contract=off", "-std=c++17",
                    "-I", os.path.join(ROOT, "noahmp-1_amd", "csrc"), "-o", exe, SRC, "-lm"],
                   check=True)
    return exe


@pytest.mark.parametrize("fn", FUNCS)
def test_core_bit_exact_vs_host_libm(checker, fn):
    total = 0
    for first, count, stride in ranges(fn, os.environ.get("NMP_EXHAUSTIVE") == "1"):
        r = subprocess.run([checker, fn, str(first), str(count), str(stride)],
                           capture_output=True, text=True, timeout=1200)
        assert r.returncode == 0 and f" mismatches 0 of {count}" in r.stdout, \
            (hex(first), count, stride, r.stdout + r.stderr)
        total += count
    assert total >= 3e7
