"""The Newton loops' in-range libm cores on the GPU (csrc/glibc_math.h
expf_inrange / logf_inrange / powf_inrange / atanf_ge1, csrc/sflx_math.h
MthInRange32), in three parts.

 1. The device build of each core (atanf's division by DivFast32) equals its
    host build (atanf's division IEEE) bit for bit on the sets of the CPU test
    (tests/test_glibc_math_inrange.py, which ties the host build to libm): the
    +-4096 neighbourhoods of every interval end and breakpoint and the strided
    rest (atanf's interval in full), at 256 and 64 threads per block.
 2. A probe library with the new windows narrowed sends lanes out through
    each of them part way through the loops; every column still equals the C
    restatement bit for bit and each new fb_why counter is non-zero.
 3. With the shipped windows (a counting build of the same sources) no lane
    of the same columns leaves through a new window: the fast path is the one
    that runs, and is the one being timed.
Parts 2 and 3 run tests/probe_libm.py in a child process each, because each
loads its own engine library.
"""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from test_glibc_math_inrange import FUNCS, ranges

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
LI_LIB = os.path.join(HERE, "lib", "libnmp_libm_inrange.so")
VARIANTS = os.path.join(ROOT, "noahmp-1_amd", "lib", "variants")
FN = {"expf": 0, "logf": 1, "pow_q": 2, "pow_mq": 3, "atanf": 4}  # libm_inrange.hip


@pytest.fixture(scope="module")
def li():
    if not os.path.exists(LI_LIB):
        pytest.fail(f"{LI_LIB} missing: run __graft_entry__.build()")
    lib = C.CDLL(LI_LIB)
    lib.li_sweep.argtypes = [C.c_int, C.c_uint, C.c_ulonglong, C.c_uint, C.c_int,
                             np.ctypeslib.ndpointer(np.uint64, flags="C_CONTIGUOUS")]
    return lib


@pytest.mark.gpu
@pytest.mark.parametrize("threads", [256, 64])
@pytest.mark.parametrize("fn", FUNCS)
def test_device_core_equals_host_core(li, fn, threads):
    total = 0
    for first, count, stride in ranges(fn):
        res = np.zeros(5, np.uint64)
        rc = li.li_sweep(FN[fn], first, count, stride, threads, res)
        assert rc == 0, rc
        n, bad, u, dev, host = (int(v) for v in res)
        assert n == count and bad == 0, (
            f"{fn} at {threads} threads: {bad} mismatches in {n} inputs from 0x{first:08x} stride "
            f"{stride}; first at x = 0x{u:08x}: device 0x{dev:08x}, host 0x{host:08x}")
        total += n
    assert total >= 3e6


def _probe(libname, expect):
    path = os.path.join(VARIANTS, libname)
    if not os.path.exists(path):
        pytest.fail(f"probe library missing ({path}): run __graft_entry__.build()")
    env = dict(os.environ, NOAHMP_ENGINE_LIB=path)
    r = subprocess.run([sys.executable, os.path.join(HERE, "probe_libm.py"), "--expect", expect],
                       env=env, capture_output=True, text=True, timeout=110)
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert line, f"probe produced no result (rc {r.returncode}): {r.stderr[-2000:]}"
    res = json.loads(line[-1])
    for run in res["runs"]:
        print(run)
    assert len(res["runs"]) == 8
    assert r.returncode == 0 and res["ok"], res
    return res


@pytest.mark.gpu
def test_lanes_leaving_through_the_libm_windows_stay_bit_exact():
    res = _probe("lib_probe_libm.so", "fire")
    for run in res["runs"]:
        assert run["columns_differing"] == 0 and min(run["windows"].values()) > 0, run


@pytest.mark.gpu
def test_no_lane_leaves_through_the_shipped_libm_windows():
    res = _probe("lib_count_libm.so", "none")
    for run in res["runs"]:
        assert run["columns_differing"] == 0 and max(run["windows"].values()) == 0, run
