"""tests/golden/math64.npz (the fp64 math primitives' high-precision
reference, read by tests/test_gpu_math64.py) is what its generator produces.

Where mpmath imports, everything is regenerated and compared bit for bit with
the committed file, and each double-double (hi, lo) is checked against the
mpmath value: hi is its correctly rounded double and hi + lo reconstructs it
to 2^-100 relative.  Without mpmath only the file's shape is checked.
"""
import importlib.util
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
NPZ = os.path.join(HERE, "golden", "math64.npz")
GEN = os.path.join(HERE, "golden", "make_math64_golden.py")


def _generator():
    spec = importlib.util.spec_from_file_location("make_math64_golden", GEN)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_golden_file_shape():
    gen = _generator()
    with np.load(NPZ) as z:
        keys = set(z.files)
        for k in keys:
            assert z[k].dtype == np.float64 and z[k].ndim == 1 and np.isfinite(z[k]).all(), k
            assert 0 < z[k].size <= gen.MAX_POINTS, k
        for fn in ("exp", "exp2", "log", "log10", "tanh", "atan", "tan", "acos", "cos", "sqrt",
                   "pow", "pow_q", "pow_mq"):
            assert {fn + "_x", fn + "_hi", fn + "_lo"} <= keys, fn
            assert z[fn + "_x"].size == z[fn + "_hi"].size == z[fn + "_lo"].size
            # lo is the remainder below hi's rounding: at most half an ulp of hi
            assert (np.abs(z[fn + "_lo"]) <= 0.5 * np.spacing(np.abs(z[fn + "_hi"]))).all(), fn
        assert {"pow_y", "pow_pair_x", "pow_pair_y1", "pow_pair_y2", "pow_pair_hi1",
                "pow_pair_lo1", "pow_pair_hi2", "pow_pair_lo2"} <= keys
    assert os.path.getsize(NPZ) < 1 << 20


def test_golden_file_is_the_generators_output():
    mpmath = pytest.importorskip("mpmath")
    gen = _generator()
    want = gen.generate()
    with np.load(NPZ) as z:
        assert set(z.files) == set(want)
        for k, v in want.items():
            assert z[k].dtype == v.dtype and z[k].shape == v.shape, k
            assert np.array_equal(z[k].view(np.uint64), v.view(np.uint64)), k
        got = {k: z[k] for k in z.files}
    # the double-double against mpmath itself, on every function's points
    mpmath.mp.prec = gen.PREC
    mp = mpmath
    fns = {"exp": mp.exp, "exp2": lambda x: mp.power(2, x), "log": mp.log, "log10": mp.log10,
           "tanh": mp.tanh, "atan": mp.atan, "tan": mp.tan, "acos": mp.acos, "cos": mp.cos,
           "sqrt": mp.sqrt, "pow_q": lambda x: mp.root(x, 4),
           "pow_mq": lambda x: 1 / mp.root(x, 4)}
    cases = [(fn, [(x,) for x in got[fn + "_x"]], got[fn + "_hi"], got[fn + "_lo"], f)
             for fn, f in fns.items()]
    cases.append(("pow", list(zip(got["pow_x"], got["pow_y"])), got["pow_hi"], got["pow_lo"],
                  mp.power))
    for k in "12":
        cases.append(("pow_pair" + k, list(zip(got["pow_pair_x"], got["pow_pair_y" + k])),
                      got["pow_pair_hi" + k], got["pow_pair_lo" + k], mp.power))
    tol = mp.mpf(2) ** -100
    for name, args, hi, lo, f in cases:
        for a, h, l in zip(args, hi, lo):
            v = f(*[mp.mpf(float(t)) for t in a])
            assert float(v) == h, (name, a)  # mpmath rounds to nearest on conversion
            if v != 0:
                assert abs((mp.mpf(float(h)) + mp.mpf(float(l))) - v) <= tol * abs(v), (name, a)
