"""The math policy of the fp32 libm calls outside the Newton loops on the GPU
(csrc/sflx_math.h MthGuard32), in two parts.

 1. tests/native/libm_outloop.hip calls the policy's exp, log, log10, pow and
    pow_pair after stage_math_tables(), at 256 and 64 threads per block, and
    every result must equal the host build of the full functions (gm::expf,
    ...: tied to libm by tests/test_glibc_math.py) bit for bit, on
      (a) arrays with every lane inside the core's interval,
      (b) the same with exactly one lane per wave outside it: NaN, +-inf, +-0,
          negative, subnormal, |x| = 88 and its two neighbours (pow: also
          y = 0, inf, NaN); exp's interval is one-sided (x < 88), so its values
          at and below -88 count as inside,
      (d) a call under a divergent branch whose inactive lanes hold
          out-of-range operands: the active lanes' results are the host's, the
          inactive lanes' outputs stay untouched,
    each with a length that is no multiple of 64 (c), so the last wave has
    inactive lanes.  The same source built with the policy's counters shows
    which arm ran: (a) and (d) never the full function, (b) in every wave
    that holds an operand outside.
 2. The step kernel's full-function arms (tests/probe_libm_outloop.py, a child
    process per library): a probe library with the policy's intervals narrowed
    sends most waves through the full functions at most sites and every
    column still equals the reference fixtures bit for bit; a counting build
    with the shipped intervals prints the share of wave-level calls that took
    a full function on mixed day, night and snow columns.
"""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from test_glibc_math_outloop import exponents

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
VARIANTS = os.path.join(ROOT, "noahmp-1_amd", "lib", "variants")
FN = {"exp": 0, "log": 1, "log10": 2, "pow": 3, "pow_pair": 4}  # libm_outloop.hip
N = 32768 + 17          # 513 waves, the last with 17 lanes
SENTINEL = 0xDEADBEEF
U32 = np.ctypeslib.ndpointer(np.uint32, flags="C_CONTIGUOUS")


def _load(name):
    path = os.path.join(HERE, "lib", name)
    if not os.path.exists(path):
        pytest.fail(f"{path} missing: run __graft_entry__.build()")
    lib = C.CDLL(path)
    lib.lo_eval.argtypes = [C.c_int, C.c_uint, C.c_int, U32, U32, U32, C.c_void_p, U32, U32, U32,
                            U32, np.ctypeslib.ndpointer(np.uint64, flags="C_CONTIGUOUS")]
    return lib


@pytest.fixture(scope="module")
def plain():
    lib = _load("libnmp_libm_outloop.so")
    assert lib.lo_counting() == 0
    return lib


@pytest.fixture(scope="module")
def counting():
    lib = _load("libnmp_libm_outloop_count.so")
    assert lib.lo_counting() == 1
    return lib


def f2u(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32).copy()


def inside(fn, rng):
    """x, y, y2 (bit patterns) with every lane inside the core's interval."""
    if fn == "exp":  # x < 88: uniform in |x| < 88, a log-uniform part down to the
        # subnormals, and a tenth below -88 (through the underflow bound to -inf)
        x = rng.uniform(-87.99, 87.99, N).astype(np.float32)
        small = rng.integers(0, 0x42b00000, N, dtype=np.uint32) | \
            (rng.integers(0, 2, N, dtype=np.uint32) << 31)
        xu = np.where(rng.random(N) < 0.5, f2u(x), small).astype(np.uint32)
        low = rng.integers(0xc2b00000, 0xff800001, N, dtype=np.uint32)
        xu = np.where(rng.random(N) < 0.1, low, xu).astype(np.uint32)
        assert (xu.view(np.float32) < 88.0).all()
    else:            # every positive normal float, by bit pattern
        xu = rng.integers(0x00800000, 0x7f800000, N, dtype=np.uint32)
        if fn in ("pow", "pow_pair"):  # half near the physical range (0.01 .. 10)
            near = f2u(np.exp(rng.uniform(np.log(0.01), np.log(10.0), N)))
            xu = np.where(rng.random(N) < 0.5, near, xu).astype(np.uint32)
    ys = f2u(exponents())
    y = ys[rng.integers(0, len(ys), N)]
    y2 = ys[rng.integers(0, len(ys), N)]
    return np.ascontiguousarray(xu), np.ascontiguousarray(y), np.ascontiguousarray(y2)


def outside_values(fn):
    """(x, y or None, truly outside the interval) for the one bad lane per wave."""
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    sub = np.float32(1.0e-40)
    b88 = np.float32(88.0)
    if fn == "exp":
        # (the policy's exp is one-sided: x < 88; the negative side, -inf included,
        # runs the core with the underflow exit as a select)
        vals = [(nan, None, True), (inf, None, True), (-inf, None, False), (b88, None, True),
                (-b88, None, False), (np.nextafter(b88, inf), None, True),
                (np.nextafter(b88, np.float32(0)), None, False),
                (-np.nextafter(b88, np.float32(0)), None, False),
                (np.float32(89.0), None, True), (np.float32(-104.0), None, False),
                (np.float32(-103.9), None, False), (np.float32(-1.0e30), None, False),
                (np.float32(1.0e30), None, True)]
    else:
        vals = [(v, None, True) for v in (nan, inf, -inf, np.float32(0.0), np.float32(-0.0),
                                          np.float32(-1.5), sub, -sub, -b88)]
        vals += [(np.float32(1.1754944e-38), None, False), (np.float32(3.4028235e38), None, False)]
        if fn in ("pow", "pow_pair"):
            vals += [(np.float32(0.5), v, True) for v in (np.float32(0.0), np.float32(-0.0), inf,
                                                          -inf, nan)]
            vals += [(np.float32(-2.0), np.float32(3.0), True), (np.float32(-2.0), np.float32(2.0), True),
                     (np.float32(1.0), nan, True), (nan, np.float32(0.0), True)]
    return vals


def run(lib, fn, threads, x, y, y2, active=None):
    out = np.full(N, SENTINEL, np.uint32)
    out2 = np.full(N, SENTINEL, np.uint32)
    host, host2 = np.zeros(N, np.uint32), np.zeros(N, np.uint32)
    counts = np.zeros(2, np.uint64)
    act = None if active is None else np.ascontiguousarray(active, np.uint8)
    rc = lib.lo_eval(FN[fn], N, threads, x, y, y2, None if act is None else act.ctypes.data, out,
                     out2, host, host2, counts)
    assert rc == 0, rc
    return out, out2, host, host2, [int(c) for c in counts]


def check(fn, threads, x, y, y2, out, out2, host, host2, active=None):
    act = np.ones(N, bool) if active is None else np.asarray(active, bool)
    pairs = [(out, host)] + ([(out2, host2)] if fn == "pow_pair" else [])
    for got, want in pairs:
        # equal bits, or both NaN (tests/test_gpu_math.py's rule: an invalid operation's
        # default NaN has the host's sign on the host and the device's on the device)
        both_nan = np.isnan(got.view(np.float32)) & np.isnan(want.view(np.float32))
        bad = np.flatnonzero(act & (got != want) & ~both_nan)
        assert bad.size == 0, (
            f"{fn} at {threads} threads: {bad.size} mismatches; first at lane {bad[0]}: x = "
            f"0x{x[bad[0]]:08x}, y = 0x{y[bad[0]]:08x}: device 0x{got[bad[0]]:08x}, host "
            f"0x{want[bad[0]]:08x}")
        assert (got[~act] == SENTINEL).all(), f"{fn}: an inactive lane's output was written"
    if fn != "pow_pair":
        assert (out2 == SENTINEL).all()


def with_one_outside_lane_per_wave(fn, x, y, y2):
    x, y, y2 = x.copy(), y.copy(), y2.copy()
    vals = outside_values(fn)
    nwave = (N + 63) // 64
    truly = np.zeros(nwave, bool)
    for w in range(nwave):
        i = w * 64 + (w * 7) % min(64, N - w * 64)
        xv, yv, t = vals[w % len(vals)]
        x[i] = f2u([xv])[0]
        if yv is not None:
            y[i] = f2u([yv])[0]
            if fn == "pow_pair" and w % 2:   # the second exponent's turn
                y[i], y2[i] = y2[i], f2u([yv])[0]
        truly[w] = t
    return x, y, y2, truly


CASES = [(fn, t) for fn in FN for t in (256, 64)]


@pytest.mark.gpu
@pytest.mark.parametrize("fn,threads", CASES)
def test_policy_equals_host_full_functions(plain, counting, fn, threads):
    rng = np.random.default_rng(1234 + FN[fn])
    nwave = (N + 63) // 64
    x, y, y2 = inside(fn, rng)
    # (a), (c): every lane inside
    for lib in (plain, counting):
        out, out2, host, host2, cnt = run(lib, fn, threads, x, y, y2)
        check(fn, threads, x, y, y2, out, out2, host, host2)
    assert cnt == [nwave, 0], f"(a) {fn}: calls, full-function calls = {cnt}"
    # (b): one lane per wave outside
    xb, yb, y2b, truly = with_one_outside_lane_per_wave(fn, x, y, y2)
    for lib in (plain, counting):
        out, out2, host, host2, cnt = run(lib, fn, threads, xb, yb, y2b)
        check(fn, threads, xb, yb, y2b, out, out2, host, host2)
    assert cnt == [nwave, int(truly.sum())], f"(b) {fn}: {cnt} vs {int(truly.sum())} waves outside"
    # (d): half the lanes inactive, holding out-of-range operands
    active = rng.random(N) < 0.5
    active[:64] = False            # a whole wave inactive: no call at all
    active[64:128] = True
    vals = outside_values(fn)
    xd, yd, y2d = x.copy(), y.copy(), y2.copy()
    idx = np.flatnonzero(~active)
    pick = [vals[k % len(vals)] for k in range(idx.size)]
    xd[idx] = f2u([p[0] for p in pick])
    if fn in ("pow", "pow_pair"):
        yd[idx] = f2u([np.float32(0.0) if p[1] is None else p[1] for p in pick])
        y2d[idx] = f2u([np.float32(np.nan)] * idx.size)
    for lib in (plain, counting):
        out, out2, host, host2, cnt = run(lib, fn, threads, xd, yd, y2d, active)
        check(fn, threads, xd, yd, y2d, out, out2, host, host2, active)
    waves_active = int(np.add.reduceat(active.astype(int), np.arange(0, N, 64)).astype(bool).sum())
    assert cnt == [waves_active, 0], f"(d) {fn}: {cnt}, {waves_active} waves with an active lane"


def _probe(libname, mode):
    path = os.path.join(VARIANTS, libname)
    if not os.path.exists(path):
        pytest.fail(f"probe library missing ({path}): run __graft_entry__.build()")
    env = dict(os.environ, NOAHMP_ENGINE_LIB=path)
    r = subprocess.run([sys.executable, os.path.join(HERE, "probe_libm_outloop.py"), mode],
                       env=env, capture_output=True, text=True, timeout=110)
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert line, f"probe produced no result (rc {r.returncode}): {r.stderr[-2000:]}"
    res = json.loads(line[-1])
    assert r.returncode == 0 and res["ok"], res
    return res


@pytest.mark.gpu
def test_full_function_arms_in_the_step_kernel_stay_bit_exact():
    """Intervals narrowed (exp x < -1e30; log, log10 and pow's base x >= 1e30): on a
    reference fixture set's NONE, NONE, OUT trajectory every column equals the
    fixtures bit for bit, and most wave-level calls took a full function."""
    res = _probe("lib_probe_libm_outloop.so", "fixtures")
    print(res)
    assert res["columns_differing"] == 0 and res["ncol"] <= 512
    for fn, (calls, slow) in res["calls"].items():
        print(f"{fn}: {slow} of {calls} wave-level calls took the full function")
    assert sum(s for _, s in res["calls"].values()) > 0.5 * sum(c for c, _ in res["calls"].values())


@pytest.mark.gpu
def test_shipped_intervals_full_function_share():
    """Shipped intervals, counting build: 4,096 mixed columns over 8 steps (day,
    night, snow) equal the C restatement bit for bit; the share of wave-level
    calls that took a full function is printed, not asserted (the soil pow
    underflow and exp underflows are legitimately reachable)."""
    res = _probe("lib_count_libm.so", "shares")
    assert res["columns_differing"] == 0
    for fn, (calls, slow) in res["calls"].items():
        print(f"{fn}: {slow} of {calls} wave-level calls took the full function "
              f"({100.0 * slow / max(calls, 1):.3f} %)")
