"""The fp64 engine's math primitives (csrc/sflx_math.h Mth<double, true>,
pow_pair<double, true>) on the device against a high-precision reference.

The reference is mpmath at 160 bits, committed as double-double (hi, lo) pairs
in tests/golden/math64.npz (generator: tests/golden/make_math64_golden.py,
pinned by tests/test_math64_golden.py); the inputs are the ranges the step
kernel's call sites give.  Errors are in ulps of the correctly rounded double
hi: |got - (hi + lo)| / spacing(hi).

 * sqrt: 0 ulp (IEEE).
 * the ocml functions exp, exp2, log, log10, tanh, atan, tan, acos, cos: the
   maximum measured on an MI355X (profiles/math64/ulp.json, written by running
   this file as a program, with an optional output path) plus 1 ulp of margin
   for another ROCm patch level.
   A measured maximum above 3 ulp would be a finding, not a bound.
 * pow(x, y) = exp(y log x), derived from the bounds just asserted for log and
   exp, E_log and E_exp: log x is within E_log ulp, i.e. relative error
   <= E_log 2^-52 (an ulp is at most 2^-52 of its value); the product y log x
   adds half an ulp, so t = y log x carries a relative error
   <= (E_log + 0.5) 2^-52 and an absolute one <= |t| (E_log + 0.5) 2^-52.
   exp turns an absolute error of its argument into the same relative error of
   its result, and an ulp is at least 2^-53 of its value, so that is
   <= 2 (E_log + 0.5) |t| ulp, and exp's own error adds E_exp:
       |pow error| <= 2 (E_log + 0.5) |y ln x| + E_exp  ulp.
 * pow_q(x) = sqrt(sqrt(x)): the inner root's relative error <= 2^-53 is halved
   by the outer root, which adds its own <= 2^-53: <= 1.5 2^-53 relative,
   <= 1.5 ulp.  pow_mq(x) = 1 / pow_q(x): one more rounding, <= 2.5 ulp.
 * pow_pair<double>: bit-equal to two Mth<double, true>::pow calls.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
RT_LIB = os.path.join(HERE, "lib", "libnmp_routines.so")
NPZ = os.path.join(HERE, "golden", "math64.npz")
ULP_JSON = os.path.join(ROOT, "profiles", "math64", "ulp.json")

# function ids of tests/routines.hip (enum MathFn; 9 is sqrt in the fp64 entry)
FN = {"exp": 0, "exp2": 1, "log": 2, "log10": 3, "tanh": 4, "atan": 5, "tan": 6, "acos": 7,
      "cos": 8, "sqrt": 9, "pow": 10, "pow_q": 11, "pow_mq": 12, "pow_pair": 13}
OCML = ["exp", "exp2", "log", "log10", "tanh", "atan", "tan", "acos", "cos"]
MARGIN = 1.0       # ulp, for a different ROCm patch level
FINDING = 3.0      # a measured ocml maximum above this is reported, not absorbed
THREADS = 256


def load_lib():
    lib = C.CDLL(RT_LIB)
    f64p = np.ctypeslib.ndpointer(np.float64, flags="C_CONTIGUOUS")
    lib.rt_math64_list.argtypes = [C.c_int, C.c_int, f64p, C.c_void_p, C.c_void_p, C.c_int, f64p,
                                   C.c_void_p]
    return lib


@pytest.fixture(scope="module")
def rt():
    if not os.path.exists(RT_LIB):
        pytest.fail(f"{RT_LIB} missing: run __graft_entry__.build()")
    return load_lib()


@pytest.fixture(scope="module")
def gold():
    with np.load(NPZ) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def measured():
    with open(ULP_JSON) as f:
        return json.load(f)["max_ulp"]


def device(lib, fn, x, y1=None, y2=None, threads=THREADS):
    x = np.ascontiguousarray(x, np.float64)
    ys = [None if y is None else np.ascontiguousarray(y, np.float64) for y in (y1, y2)]
    o1, o2 = np.zeros_like(x), np.zeros_like(x)
    ptr = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    rc = lib.rt_math64_list(FN[fn], x.size, x, ptr(ys[0]), ptr(ys[1]), threads, o1,
                            ptr(o2) if fn == "pow_pair" else None)
    assert rc == 0, rc
    return (o1, o2) if fn == "pow_pair" else o1


def ulp_error(got, hi, lo):
    """|got - (hi + lo)| in ulps of hi; got - hi is exact for a got within a
    factor of two of hi."""
    return np.abs((got - hi) - lo) / np.spacing(np.abs(hi))


def worst(err, *cols):
    i = int(np.argmax(err))
    return f"max {err[i]:.4f} ulp at " + ", ".join(f"{float(c[i]).hex()} ({c[i]!r})" for c in cols)


def pow_bound(x, y, e_log, e_exp):
    return 2.0 * (e_log + 0.5) * np.abs(y * np.log(x)) + e_exp


def measure(lib, gold):
    """Maximum ulp error per function on the committed points."""
    out = {}
    for fn in OCML + ["sqrt", "pow_q", "pow_mq"]:
        got = device(lib, fn, gold[fn + "_x"])
        out[fn] = float(ulp_error(got, gold[fn + "_hi"], gold[fn + "_lo"]).max())
    got = device(lib, "pow", gold["pow_x"], gold["pow_y"])
    out["pow"] = float(ulp_error(got, gold["pow_hi"], gold["pow_lo"]).max())
    return out


@pytest.mark.gpu
def test_sqrt_is_correctly_rounded(rt, gold):
    got = device(rt, "sqrt", gold["sqrt_x"])
    bad = got.view(np.uint64) != gold["sqrt_hi"].view(np.uint64)
    assert not bad.any(), (int(bad.sum()), float(gold["sqrt_x"][bad][0]).hex())


@pytest.mark.gpu
@pytest.mark.parametrize("fn", OCML)
def test_ocml_function_within_measured_bound(rt, gold, measured, fn):
    assert measured[fn] <= FINDING, f"{fn}: recorded maximum {measured[fn]} ulp is a finding"
    x = gold[fn + "_x"]
    err = ulp_error(device(rt, fn, x), gold[fn + "_hi"], gold[fn + "_lo"])
    print(f"{fn}: {worst(err, x)}; recorded {measured[fn]:.4f}")
    assert err.max() <= measured[fn] + MARGIN, f"{fn}: {worst(err, x)}"


@pytest.mark.gpu
def test_pow_within_derived_bound(rt, gold, measured):
    """2 (E_log + 0.5) |y ln x| + E_exp ulp (module docstring), point by point,
    with E_log and E_exp the bounds asserted above."""
    e_log, e_exp = measured["log"] + MARGIN, measured["exp"] + MARGIN
    x, y = gold["pow_x"], gold["pow_y"]
    err = ulp_error(device(rt, "pow", x, y), gold["pow_hi"], gold["pow_lo"])
    bound = pow_bound(x, y, e_log, e_exp)
    print(f"pow: {worst(err, x, y)}; largest error/bound {float((err / bound).max()):.4f}; "
          f"bound there {float(bound[np.argmax(err / bound)]):.3f}")
    over = err > bound
    assert not over.any(), (int(over.sum()), worst(err - bound, x, y))


@pytest.mark.gpu
@pytest.mark.parametrize("fn,bound", [("pow_q", 1.5), ("pow_mq", 2.5)])
def test_fourth_roots_within_derived_bound(rt, gold, fn, bound):
    x = gold[fn + "_x"]
    err = ulp_error(device(rt, fn, x), gold[fn + "_hi"], gold[fn + "_lo"])
    print(f"{fn}: {worst(err, x)}")
    assert err.max() <= bound, f"{fn}: {worst(err, x)}"


@pytest.mark.gpu
def test_pow_pair_is_two_pow_calls(rt, gold, measured):
    """The header's claim: each result equal to Mth::pow's bit for bit; and so
    inside pow's bound against the reference."""
    x, y1, y2 = gold["pow_pair_x"], gold["pow_pair_y1"], gold["pow_pair_y2"]
    r1, r2 = device(rt, "pow_pair", x, y1, y2)
    p1, p2 = device(rt, "pow", x, y1), device(rt, "pow", x, y2)
    for k, (r, p) in enumerate(((r1, p1), (r2, p2))):
        bad = r.view(np.uint64) != p.view(np.uint64)
        assert not bad.any(), (k, int(bad.sum()), float(x[bad][0]).hex())
    e_log, e_exp = measured["log"] + MARGIN, measured["exp"] + MARGIN
    for r, y, k in ((r1, y1, "1"), (r2, y2, "2")):
        err = ulp_error(r, gold["pow_pair_hi" + k], gold["pow_pair_lo" + k])
        assert (err <= pow_bound(x, y, e_log, e_exp)).all(), worst(err, x, y)


@pytest.mark.gpu
def test_launch_shape_does_not_matter(rt, gold):
    """An fp64 entry at 64 and 32 threads per block gives the same bits."""
    x, y = gold["pow_x"], gold["pow_y"]
    ref = device(rt, "pow", x, y)
    for threads in (64, 32):
        assert np.array_equal(device(rt, "pow", x, y, threads=threads).view(np.uint64),
                              ref.view(np.uint64))


if __name__ == "__main__":
    # measure on the device and write profiles/math64/ulp.json
    import subprocess
    with np.load(NPZ) as z:
        g = {k: z[k] for k in z.files}
    m = measure(load_lib(), g)
    try:
        ver = open("/opt/rocm/.info/version").read().strip()
    except OSError:
        ver = subprocess.run(["hipconfig", "--version"], capture_output=True,
                             text=True).stdout.strip()
    import sys
    path = sys.argv[1] if len(sys.argv) > 1 else ULP_JSON
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump({"what": "maximum error of Mth<double, true> in ulps of the correctly rounded "
                           "double, on the points of tests/golden/math64.npz",
                   "device": "MI355X (gfx950)", "rocm": ver, "max_ulp": m}, f, indent=1)
        f.write("\n")
    print(json.dumps(m, indent=1))
