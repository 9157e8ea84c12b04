"""The gfx950 build of the exact float libm (csrc/glibc_math.h), on its own.

tests/test_glibc_math.py ties the header as compiled for the host (g++ and
ROCm's clang++) to the host libm.  Here the DEVICE compilation of the same
header -- through nmp::Mth<float, true> and nmp::pow_pair<float, true>, after
stage_math_tables() as in the step kernel (tests/routines.hip k_m32) -- is
tied to the host compilation, bit for bit: equal bits, or both NaN.  So
libm = host header (g++) = host header (clang) = device header.

Four input sets per function, each with 0 mismatches, each at 256, 64 and 32
threads per block (stage_math_tables strides by blockDim.x over 48 int4 words:
32 threads take its loop's second trip):
 (a) the CPU checker's own set: every 61st of the 2^32 patterns (univariate),
     every 997th for powf's 30 exponents and powf_pair's 23 pairs, and the
     first 2^22 pairs of its hashed random sequence;
 (b) edges, dense: every pattern within +-4096 of every literal the header
     compares its argument against (parsed from the header), and both signs
     of 0, the smallest / largest subnormal, FLT_MIN, FLT_MAX, inf, a quiet
     and a signalling NaN;
 (c) subnormal results, contiguous (where a flushing build would differ), with
     the number of subnormal host results asserted;
 (d) domain: gm::cosf and gm::tanf restate glibc only for |x| < 120 (beyond
     that they call the double function, "not reached by the physics"), so
     their sets (a) and (b) are restricted to |x| < 120, as the CPU checker
     does.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
RT_LIB = os.path.join(HERE, "lib", "libnmp_routines.so")
HEADER = os.path.join(ROOT, "noahmp-1_amd", "csrc", "glibc_math.h")

# function ids of tests/routines.hip (enum MathFn)
FN = {"exp": 0, "exp2": 1, "log": 2, "log10": 3, "tanh": 4, "atan": 5, "tan": 6, "acos": 7,
      "cos": 8, "expm1": 9, "pow": 10, "pow_q": 11, "pow_mq": 12, "pow_pair": 13}
UNIVARIATE = ["exp", "exp2", "log", "log10", "tanh", "atan", "tan", "acos", "cos", "expm1"]
DOM120 = ("cos", "tan")  # (d)
THREADS = [256, 64, 32]
NBHD = 4096

f32 = np.float32
INF, NAN = f32(np.inf), f32(np.nan)
# check_powf's exponents and check_powf_pair's pairs (tests/native/
# glibc_math_check.cpp), evaluated in fp32 as the C literals are
POWF_YS = [f32(0.25), f32(-0.25), f32(1.7), f32(0.667), f32(4.0), f32(2.0) / f32(3.0), f32(0.5),
           f32(2.0), f32(3.0), f32(-1.0), f32(-0.5), f32(1.5), f32(0.2857143), f32(-0.0890),
           f32(-0.1222), f32(11.5), f32(7.25), f32(5.08), f32(-1.0) / f32(4.26),
           f32(-1.0) / f32(11.55), f32(2.0) * f32(5.25) + f32(3.0), f32(5.25) + f32(2.0),
           f32(0.1), f32(-3.0), f32(10.0), f32(1e-3), f32(-7.5), f32(0.0), f32(1.0), f32(33.0)]
_BEXPS = [f32(v) for v in (2.79, 4.26, 4.74, 5.33, 5.25, 6.77, 8.72, 8.17, 10.73, 10.39, 11.55,
                           12.61, 2.79, 4.26, 11.55, 2.5)]
POWF_PAIRS = ([(b + f32(2.0), f32(2.0) * b + f32(3.0)) for b in _BEXPS]
              + [(f32(0.0), f32(1.0)), (f32(1.0), f32(0.0)), (f32(-2.0), f32(3.0)),
                 (f32(0.25), f32(-0.25)), (INF, f32(2.0)), (f32(2.0), NAN), (f32(1e-3), f32(33.0))])
assert len(POWF_YS) == 30 and len(POWF_PAIRS) == 23


def bits(v):
    return int(np.array(v, np.float32).view(np.uint32))


def as_f32(u):
    return np.asarray(u, np.uint32).view(np.float32)


# both signs of: 0, smallest / largest subnormal, FLT_MIN, FLT_MAX, inf, qNaN, sNaN
SPECIALS = [s | p for p in (0x00000000, 0x00000001, 0x007fffff, 0x00800000, 0x7f7fffff,
                            0x7f800000, 0x7fc00000, 0x7fa00000) for s in (0, 0x80000000)]

# ---- (b): the literals of the header ----------------------------------------
# the header functions whose comparisons a call of each function can reach
BODIES = {
    "exp": ["expf", "top12"], "exp2": ["exp2f", "top12"], "log": ["logf"],
    "log10": ["log10f", "logf"], "expm1": ["expm1f"], "tanh": ["tanhf", "expm1f"],
    "atan": ["atanf"], "acos": ["acosf"], "cos": ["cosf", "sinf_poly", "abstop12"],
    "tan": ["tanf", "kernel_tanf", "abstop12"],
    "pow": ["powf", "powf_tail", "powf_log2", "powf_exp2", "powf_checkint", "powf_issnan",
            "powf_zeroinfnan"],
}
_NOT_IN = r"(?<![\w.])"
_HEXI = re.compile(_NOT_IN + r"0x([0-9a-fA-F]{8})u?(?![\w.])")
_HEXF = re.compile(_NOT_IN + r"(0x[0-9a-fA-F]*\.?[0-9a-fA-F]*p[+-]?\d+)(f?)(?![\w.])")
_DEC = re.compile(_NOT_IN + r"(\d+\.\d*(?:[eE][+-]?\d+)?|\d+[eE][+-]?\d+)(f?)(?![\w.])")


def header_bodies():
    text = open(HEADER).read()
    text = re.sub(r"//[^\n]*", "", text)
    heads = list(re.finditer(r"^GM_HD [\w:<>]+&? (\w+)\(", text, re.M))
    return {m.group(1): text[m.start():(heads[i + 1].start() if i + 1 < len(heads) else len(text))]
            for i, m in enumerate(heads)}


def literal_patterns(fn):
    """Bit patterns of every 32-bit hex literal and every literal with a float
    value in the header functions behind `fn`: each breakpoint an argument is
    compared against is among them (so are masks and coefficients, which only
    add points).  tanhf passes 2|x| to expm1f, so expm1f's literals are also
    taken at half their value."""
    bodies = header_bodies()
    pats = set()
    for name in BODIES[fn]:
        body = bodies[name]
        found = {int(h, 16) for h in _HEXI.findall(body)}
        for rx, conv in ((_HEXF, float.fromhex), (_DEC, float)):
            for lit, suffix in rx.findall(body):
                v = conv(lit)
                with np.errstate(over="ignore"):
                    if suffix or float(f32(v)) == v:  # a double that is a float: (float)pio4
                        found.add(bits(f32(v)))
        if fn == "tanh" and name == "expm1f":
            found |= {p - 0x00800000 for p in found if 0x01000000 <= p < 0x7f800000}
        pats |= found
    if fn == "tan":
        pats.add(0x42f00000)  # |x| < 120 is spelled abstop12(x) <= 0x42e: no 32-bit literal
    return pats


def edge_patterns(fn):
    """+-NBHD patterns around every literal, around the 2^20-aligned pattern
    below it (top12 / abstop12 compare the top 12 bits) and around the
    specials, for both signs."""
    centres = set(SPECIALS)
    for p in literal_patterns(fn):
        for q in (p, p & 0xfff00000):
            centres |= {q & 0x7fffffff, q | 0x80000000}
    off = np.arange(-NBHD, NBHD + 1, dtype=np.int64)
    u = (np.array(sorted(centres), np.int64)[:, None] + off[None, :]) % (1 << 32)
    u = np.unique(u.astype(np.uint32))
    if fn in DOM120:
        with np.errstate(invalid="ignore"):
            u = u[np.abs(as_f32(u)) < f32(120.0)]
    return u


def test_header_literals_are_found():
    """The parser sees the breakpoints the header is known to have (it would
    silently cover nothing if the header's spelling of literals changed)."""
    want = {
        "exp": [bits(88.0), bits(float.fromhex("0x1.62e42ep6")),
                bits(-float.fromhex("0x1.9fe368p6")) & 0x7fffffff],
        "exp2": [bits(128.0), bits(150.0)],
        "log": [0x3f800000, 0x00800000, 0x7f800000, 0x3f330000],
        "log10": [0x00800000, 0x7f800000, 0x3f800000],
        "expm1": [0x4195b844, 0x42b17218, 0x3eb17218, 0x3f851592, 0x33000000,
                  bits(8.8721679688e+01)],
        "tanh": [0x41b00000, 0x24000000, 0x3f800000, 0x4195b844 - 0x00800000],
        "atan": [0x4c000000, 0x3ee00000, 0x31000000, 0x3f980000, 0x3f300000, 0x401c0000],
        "acos": [0x3f800000, 0x3f000000, 0x23000000],
        "cos": [bits(float.fromhex("0x1.921FB6p-1")), bits(2.0 ** -12), bits(120.0)],
        "tan": [0x39000000, 0x3f2ca140, 0x3f490fda, bits(2.0 ** -13)],
        "pow": [0x00800000, 0x7f800000, 0x3f800000, 0x3f330000, 0x7fc00000],
    }
    for fn, pats in want.items():
        got = literal_patterns(fn)
        assert set(pats) <= got, (fn, [hex(p) for p in set(pats) - got])
    assert 0x42f00000 in literal_patterns("tan") and bits(120.0) == 0x42f00000


@pytest.fixture(scope="module")
def rt():
    if not os.path.exists(RT_LIB):
        pytest.fail(f"{RT_LIB} missing: run __graft_entry__.build()")
    lib = C.CDLL(RT_LIB)
    u32p = np.ctypeslib.ndpointer(np.uint32, flags="C_CONTIGUOUS")
    u64p = np.ctypeslib.ndpointer(np.uint64, flags="C_CONTIGUOUS")
    lib.rt_math32_sweep.argtypes = [C.c_int, C.c_uint, C.c_ulonglong, C.c_uint, C.c_float,
                                    C.c_float, C.c_int, C.c_int, u64p]
    lib.rt_math32_list.argtypes = [C.c_int, C.c_int, u32p, C.c_void_p, C.c_void_p, C.c_int, u32p,
                                   u32p, C.c_void_p, C.c_void_p]
    return lib


def sweep(rt, fn, first, count, stride, threads, y1=0.0, y2=0.0):
    """-> (inputs compared, subnormal nonzero host results); asserts 0 mismatches."""
    res = np.zeros(7, np.uint64)
    rc = rt.rt_math32_sweep(FN[fn], first, count, stride, float(y1), float(y2),
                            int(fn in DOM120), threads, res)
    assert rc == 0, rc
    n, bad, u, dev, host, nsub, which = (int(v) for v in res)
    assert bad == 0, (
        f"{fn}(y1={float(y1)!r}, y2={float(y2)!r}) at {threads} threads: {bad} mismatches in {n} "
        f"inputs; first at x = 0x{u:08x} ({float(as_f32(u))!r}), result {which}: "
        f"device 0x{dev:08x} ({float(as_f32(dev))!r}), host 0x{host:08x} ({float(as_f32(host))!r})")
    return n, nsub


def run_list(rt, fn, threads, x, y1=None, y2=None):
    """-> host bits (one array, or two for pow_pair); asserts device == host."""
    x = np.ascontiguousarray(x, np.uint32)
    ys = [None if y is None else np.ascontiguousarray(np.broadcast_to(y, x.shape), np.uint32)
          for y in (y1, y2)]
    pair = fn == "pow_pair"
    out = [np.zeros(x.size, np.uint32) for _ in range(4)]
    ptr = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    rc = rt.rt_math32_list(FN[fn], x.size, x, ptr(ys[0]), ptr(ys[1]), threads, out[0], out[1],
                           ptr(out[2]) if pair else None, ptr(out[3]) if pair else None)
    assert rc == 0, rc
    for k, (dev, host) in enumerate(((out[0], out[1]), (out[2], out[3]))[:2 if pair else 1]):
        with np.errstate(invalid="ignore"):
            same = (dev == host) | (np.isnan(as_f32(dev)) & np.isnan(as_f32(host)))
        if not same.all():
            i = int(np.flatnonzero(~same)[0])
            yy = [None if y is None else hex(int(y[i])) for y in ys]
            raise AssertionError(
                f"{fn} at {threads} threads: {int((~same).sum())} mismatches in {x.size} inputs; "
                f"first at x = 0x{int(x[i]):08x} ({float(as_f32(x[i]))!r}), y = {yy}, result {k}: "
                f"device 0x{int(dev[i]):08x} ({float(as_f32(dev[i]))!r}), "
                f"host 0x{int(host[i]):08x} ({float(as_f32(host[i]))!r})")
    return (out[1], out[3]) if pair else out[1]


def subnormal(h):
    return ((h & 0x7f800000) == 0) & ((h & 0x007fffff) != 0)


def strided_count(stride):
    return ((1 << 32) + stride - 1) // stride


# ---- (a) the CPU checker's own set ----------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("threads", THREADS)
@pytest.mark.parametrize("fn", UNIVARIATE)
def test_univariate_every_61st_pattern(rt, fn, threads):
    n, _ = sweep(rt, fn, 0, strided_count(61), 61, threads)
    # (d): cosf / tanf only inside |x| < 120 (2 * 0x42f00000 of the 2^32 patterns)
    assert n == strided_count(61) if fn not in DOM120 else abs(n - 2 * 0x42f00000 / 61) < 2


@pytest.mark.gpu
@pytest.mark.parametrize("threads", THREADS)
@pytest.mark.parametrize("y", POWF_YS, ids=lambda y: f"y={float(y):.7g}")
def test_powf_every_997th_pattern(rt, y, threads):
    n, _ = sweep(rt, "pow", 0, strided_count(997), 997, threads, y1=y)
    assert n == strided_count(997)


@pytest.mark.gpu
@pytest.mark.parametrize("threads", THREADS)
def test_powf_hashed_random_pairs(rt, threads):
    """The first 2^22 (x, y) of check_powf's hashed sequence: x any pattern,
    |y| in [2^-7, 2^9) (exponent field 0x3c000000 + 27 random bits)."""
    i = np.arange(1 << 22, dtype=np.uint64)
    h = i * np.uint64(0x9E3779B97F4A7C15)
    h ^= h >> np.uint64(29)
    h *= np.uint64(0xBF58476D1CE4E5B9)
    h ^= h >> np.uint64(32)
    ux = (h & np.uint64(0xffffffff)).astype(np.uint32)
    uy = (h >> np.uint64(32)).astype(np.uint32)
    uy = (uy & np.uint32(0x80000000)) | (np.uint32(0x3c000000) + (uy & np.uint32(0x07ffffff)))
    ay = np.abs(as_f32(uy))
    assert ay.min() >= 2.0 ** -7 and ay.max() < 2.0 ** 9
    run_list(rt, "pow", threads, ux, uy)


@pytest.mark.gpu
@pytest.mark.parametrize("threads", THREADS)
@pytest.mark.parametrize("pair", POWF_PAIRS, ids=lambda p: f"y={float(p[0]):.6g},{float(p[1]):.6g}")
def test_powf_pair_every_997th_pattern(rt, pair, threads):
    n, _ = sweep(rt, "pow_pair", 0, strided_count(997), 997, threads, y1=pair[0], y2=pair[1])
    assert n == strided_count(997)


@pytest.mark.gpu
@pytest.mark.parametrize("threads", THREADS)
@pytest.mark.parametrize("fn", ["pow_q", "pow_mq"])
def test_pow_q_is_pow_of_a_quarter(rt, fn, threads):
    """Mth<float, true>::pow_q / pow_mq == pow(x, +-0.25f) bit for bit: the
    entry's host value for them is gm::powf(x, +-0.25f)."""
    n, _ = sweep(rt, fn, 0, strided_count(997), 997, threads)
    assert n == strided_count(997)
    x = np.arange(0, 1 << 32, 997 * 64, dtype=np.uint64).astype(np.uint32)
    y = bits(0.25 if fn == "pow_q" else -0.25)
    assert np.array_equal(run_list(rt, fn, threads, x), run_list(rt, "pow", threads, x, y))


# ---- (b) edges, dense ---------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("threads", THREADS)
@pytest.mark.parametrize("fn", UNIVARIATE)
def test_univariate_edges(rt, fn, threads):
    x = edge_patterns(fn)
    lits = np.array(sorted(literal_patterns(fn) | set(SPECIALS)), np.uint32)
    with np.errstate(invalid="ignore"):
        inside = np.abs(as_f32(lits)) < f32(120.0) if fn in DOM120 else np.ones(lits.size, bool)
    assert inside.sum() >= 8 and np.isin(lits[inside], x).all()
    run_list(rt, fn, threads, x)


# powf's exponent classes: odd integers, even integers, non-integers, the
# checkint breakpoints (|y| < 1, 2^23 <= |y| < 2^24 all integers, >= 2^24 all
# even) and the zero / inf / NaN class, both signs
POW_EDGE_YS = np.array(
    [1, 3, 5, 33, 8388607, 8388609, 16777215,                      # odd integers
     2, 4, 8388608, 8388610, 16777216, 16777218, 2.0 ** 31, 1e30,  # even integers
     0.5, 1.5, 2.5, 0.25, 1.7, 1e-3, 4194303.5, 8388607.5,         # non-integers
     float.fromhex("0x1.fffffep-1"), float.fromhex("0x1.000002p0"),
     float.fromhex("0x1.fffffep127"), float.fromhex("0x1p-126"), float.fromhex("0x1p-149")],
    np.float32)
POW_EDGE_YS = np.concatenate([POW_EDGE_YS, -POW_EDGE_YS]).view(np.uint32)
POW_EDGE_YS = np.unique(np.concatenate([POW_EDGE_YS, np.array(SPECIALS, np.uint32)]))


@pytest.mark.gpu
@pytest.mark.parametrize("threads", THREADS)
def test_powf_edges_in_x(rt, threads):
    """x (both signs) around powf's literals and the specials, against every
    exponent class: negative x with odd, even and non-integer y included."""
    x = edge_patterns("pow")
    assert (x >> 31).any() and set(SPECIALS) <= set(x.tolist())
    for y in POW_EDGE_YS:
        run_list(rt, "pow", threads, x, y)


@pytest.mark.gpu
@pytest.mark.parametrize("threads", THREADS)
def test_powf_edges_in_y(rt, threads):
    """y (both signs) around checkint's and zeroinfnan's breakpoints -- 0, 1,
    2^23, 2^24, inf -- against negative, zero, subnormal, normal and special x."""
    off = np.arange(-NBHD, NBHD + 1, dtype=np.int64)
    c = np.array([s | p for p in (0, 0x3f800000, 0x4b000000, 0x4b800000, 0x7f800000)
                  for s in (0, 0x80000000)], np.int64)
    y = np.unique(((c[:, None] + off[None, :]) % (1 << 32)).astype(np.uint32))
    xs = np.array([-2.0, -1.0, -0.5, -1.5, 0.5, 1.0, 2.0, 1.5], np.float32).view(np.uint32)
    for x in np.concatenate([xs, np.array(SPECIALS, np.uint32)]):
        run_list(rt, "pow", threads, np.full(y.size, x, np.uint32), y)


@pytest.mark.gpu
@pytest.mark.parametrize("threads", THREADS)
def test_powf_pair_edges(rt, threads):
    """powf_pair's choice between the shared log2 and two powf calls: x around
    powf's literals, pairs with and without a zero / inf / NaN exponent."""
    x = edge_patterns("pow")
    for y1, y2 in POWF_PAIRS[:2] + POWF_PAIRS[16:]:
        run_list(rt, "pow_pair", threads, x, bits(y1), bits(y2))


# ---- (c) subnormal results, contiguous ------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("threads", THREADS)
def test_expf_subnormal_results(rt, threads):
    """Every x from -87.0f down to expf's underflow bound -0x1.9fe368p6f."""
    lo, hi = bits(-87.0), bits(-float.fromhex("0x1.9fe368p6"))
    assert (lo, hi) == (0xc2ae0000, 0xc2cff1b4)
    n, nsub = sweep(rt, "exp", lo, hi - lo + 1, 1, threads)
    assert n == hi - lo + 1 and nsub >= n // 2, (n, nsub)


@pytest.mark.gpu
@pytest.mark.parametrize("threads", THREADS)
def test_exp2f_subnormal_results(rt, threads):
    """Every x from -125 to -150."""
    lo, hi = bits(-125.0), bits(-150.0)
    n, nsub = sweep(rt, "exp2", lo, hi - lo + 1, 1, threads)
    assert n == hi - lo + 1 and nsub >= n // 2, (n, nsub)


POW_SUB_X0, POW_SUB_N = 0x3f000000, 1 << 14  # [0.5, 0.5 + 2^-10): 2^14 patterns of 2^-24


@pytest.mark.gpu
@pytest.mark.parametrize("threads", THREADS)
def test_powf_subnormal_results(rt, threads):
    """Bases in the contiguous run [0.5, 0.5 + 2^-10) against integer y from 127
    to 149: results from 2^-127 (1 + 2^-9)^127 down to 2^-149."""
    assert float(as_f32(POW_SUB_X0 + POW_SUB_N)) == 0.5 + 2.0 ** -10
    tot = sub = 0
    for y in range(127, 150):
        n, nsub = sweep(rt, "pow", POW_SUB_X0, POW_SUB_N, 1, threads, y1=float(y))
        tot, sub = tot + n, sub + nsub
    assert tot == 23 * POW_SUB_N and sub >= tot // 2, (tot, sub)


@pytest.mark.gpu
@pytest.mark.parametrize("threads", THREADS)
def test_powf_pair_straddles_the_subnormal_border(rt, threads):
    """x**126 is normal (>= 2^-126 = FLT_MIN) and x**127 subnormal for every x
    of the run: one shared log2, results on both sides of the border."""
    x = np.arange(POW_SUB_X0, POW_SUB_X0 + POW_SUB_N, dtype=np.uint32)
    h1, h2 = run_list(rt, "pow_pair", threads, x, bits(126.0), bits(127.0))
    assert not subnormal(h1).any() and (as_f32(h1) >= f32(2.0 ** -126)).all()
    assert subnormal(h2).all()
