"""Generator of tests/golden/math64.npz: inputs and high-precision expected
values for the fp64 engine's math primitives (csrc/sflx_math.h
Mth<double, *> and pow_pair<double, *>).

    python tests/golden/make_math64_golden.py      # rewrites math64.npz

Needs mpmath (the GPU test does not: it reads the committed file).  Every
expected value is computed at PREC bits and stored as a double-double
(hi, lo): hi the correctly rounded double, lo the rounded remainder, so
hi + lo carries ~106 bits.  Inputs are float64, taken log-uniformly (interval
ends included) from the ranges the step kernel's call sites give; at most
4096 points per function.  tests/test_math64_golden.py regenerates everything
where mpmath imports and asserts the committed file holds the same bits.

Keys: <fn>_x, <fn>_hi, <fn>_lo (and <fn>_y for pow; pow_pair_{x,y1,y2,hi1,
lo1,hi2,lo2}).
"""
import os

import numpy as np

PREC = 160
MAX_POINTS = 4096
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "math64.npz")

# the soil table's BEXP and QUARTZ values (fp32 table entries, as the kernel
# converts them) and the vegetation table's Q10 bases
BEXP = [float(np.float32(v)) for v in
        (2.79, 4.26, 4.74, 5.33, 5.25, 6.77, 8.72, 8.17, 10.73, 10.39, 11.55)]
QUARTZ = [float(np.float32(v)) for v in (0.92, 0.82, 0.60, 0.25, 0.10, 0.40, 0.35, 0.52, 0.05, 0.07)]
Q10 = [2.0] + [float(np.float32(v)) for v in (2.1, 1.2, 2.4)]  # arm, akc, ako, avcmx
RAIR, CPAIR = 287.04, 1004.64


def _mp():
    import mpmath
    mpmath.mp.prec = PREC
    return mpmath


def logspace(lo, hi, n):
    """n float64 points from lo to hi, uniform in log, the ends exactly lo and
    hi (both of one sign); evaluated in mpmath so that the points do not depend
    on the host's libm."""
    mp = _mp()
    a, b = mp.mpf(lo), mp.mpf(hi)
    sgn = -1 if lo < 0 else 1
    a, b = abs(a), abs(b)
    pts = [sgn * float(a * (b / a) ** (mp.mpf(i) / (n - 1))) for i in range(n)]
    pts[0], pts[-1] = float(lo), float(hi)
    return pts


def linspace(lo, hi, n):
    mp = _mp()
    a, b = mp.mpf(lo), mp.mpf(hi)
    pts = [float(a + (b - a) * i / (n - 1)) for i in range(n)]
    pts[0], pts[-1] = float(lo), float(hi)
    return pts


def univariate_inputs():
    """The ranges the call sites give (sflx_kernel.hip, sflx_routines.h)."""
    acos001 = 1.5607961601207294  # acos(0.01): tan's largest argument
    return {
        # canopy gaps, two-stream, esat, photosynthesis, snow ageing and
        # compaction, runoff: large negative arguments down to underflow-free
        # -100, positive ones up to exp(cwpc) and the Arrhenius terms
        "exp": [0.0] + logspace(-1e-6, -100.0, 1023) + logspace(1e-6, 25.0, 1024),
        # 2**(1 - quartz) and 2**((stc - 283.16)/10)
        "exp2": logspace(-1e-3, -10.0, 512) + logspace(1e-3, 10.0, 512),
        # height ratios up to 1e6, the stability functions' (1 + x)/2, canopy
        # gap fractions down to 0.01, frh2o's -(T - TFRZ)/T down to 1e-6, and
        # both sides of 1
        "log": (logspace(1e-6, 1e6, 1024) + [1.0 - d for d in logspace(1e-8, 0.5, 256)]
                + [1.0 + d for d in logspace(1e-8, 0.5, 256)]),
        # the Kersten number: satratio in (0.1, 1]
        "log10": logspace(0.1, 1.0, 512) + logspace(1e-3, 10.0, 512),
        # fsno = tanh(snowh / (2.5 z0 fmelt))
        "tanh": logspace(1e-6, 50.0, 1024),
        # the stability functions' x in [1, 10] and the canopy gap's
        # bb/rc tan(acos(cosz))
        "atan": logspace(1e-3, 1e3, 1024),
        # tan(acos(max(0.01, cosz)))
        "tan": logspace(1e-4, acos001, 1024),
        "acos": logspace(0.01, 1.0, 1024),
        # cos(thetap), thetap = atan(...) in [0, pi/2)
        "cos": logspace(1e-4, 1.5707, 1024),
        "sqrt": logspace(1e-12, 1e12, 1024),
        # the stability functions (1 - 16 zeta, 1 - 15 zeta) and, pow_q only,
        # the radiative temperature's quartic
        "pow_q": logspace(1.0, 1e4, 1024) + logspace(1e7, 1e11, 1024),
        "pow_mq": logspace(1.0, 1e4, 1024),
    }


def pow_inputs():
    """(x, y) of the kernel's pow call sites."""
    xs, ys = [], []

    def add(x, y):
        xs.append(float(x))
        ys.append(float(y))

    # wdfcnd / wcnd: factr in [0.01, 1], y = BEXP + 2 and 2 BEXP + 3
    for b in BEXP:
        for f in logspace(0.01, 1.0, 64):
            add(f, b + 2.0)
            add(f, 2.0 * b + 3.0)
    for r in logspace(0.8, 1.25, 256):          # (sfcprs/pair)**(RAIR/CPAIR)
        add(r, RAIR / CPAIR)
    for x in logspace(1e-8, 10.0, 256):         # wstar2: x**(2/3)
        add(x, 2.0 / 3.0)
    for x in logspace(0.01, 1.0, 256):          # albsod: cosz**1.7
        add(x, 1.7)
    for x in logspace(1e-6, 1.0, 256):          # fwet**0.667
        add(x, 0.667)
    for x in logspace(0.01, 1.0, 128):          # fsat: x**4
        add(x, 4.0)
    for b in BEXP:
        for x in logspace(1e-2, 1e6, 32):       # frh2o / supercool / wd2: x**(-1/BEXP)
            add(x, -1.0 / b)
        for x in logspace(0.01, 1.0, 16):       # psi: (sh2o/smcmax)**(-BEXP)
            add(x, -b)
    for a in Q10:                               # arm**((tv - 298.16)/10) and the Q10 terms
        for t in linspace(200.0, 330.0, 64):
            add(a, (t - 298.16) / 10.0)
    for q in QUARTZ + linspace(0.05, 0.92, 64):  # thkqtz**quartz
        add(7.7, q)
    for x in logspace(0.5, 4.0, 64):            # fmelt: (bdsno/100)**mltfct
        add(x, 2.5)
    for u in linspace(0.0, 0.5, 64):            # TKICE**(smcmax - xu), thkw**xu
        add(2.2, u)
        add(0.57, u)
    return xs, ys


def pow_pair_inputs():
    xs, y1, y2 = [], [], []
    for b in BEXP:
        for f in logspace(0.01, 1.0, 64):
            xs.append(f)
            y1.append(b + 2.0)
            y2.append(2.0 * b + 3.0)
    return xs, y1, y2


def dd(v):
    """mpf -> (hi, lo): hi the nearest double, lo the nearest double of v - hi."""
    mp = _mp()
    hi = float(v)
    return hi, float(v - mp.mpf(hi))


def generate():
    mp = _mp()
    fns = {
        "exp": mp.exp, "exp2": lambda x: mp.power(2, x), "log": mp.log, "log10": mp.log10,
        "tanh": mp.tanh, "atan": mp.atan, "tan": mp.tan, "acos": mp.acos, "cos": mp.cos,
        "sqrt": mp.sqrt, "pow_q": lambda x: mp.root(x, 4), "pow_mq": lambda x: 1 / mp.root(x, 4),
    }
    out = {}
    for name, xs in univariate_inputs().items():
        assert len(xs) <= MAX_POINTS, name
        pairs = [dd(fns[name](mp.mpf(x))) for x in xs]
        out[name + "_x"] = np.array(xs, np.float64)
        out[name + "_hi"] = np.array([p[0] for p in pairs], np.float64)
        out[name + "_lo"] = np.array([p[1] for p in pairs], np.float64)
    xs, ys = pow_inputs()
    assert len(xs) <= MAX_POINTS, len(xs)
    pairs = [dd(mp.power(mp.mpf(x), mp.mpf(y))) for x, y in zip(xs, ys)]
    out["pow_x"], out["pow_y"] = np.array(xs, np.float64), np.array(ys, np.float64)
    out["pow_hi"] = np.array([p[0] for p in pairs], np.float64)
    out["pow_lo"] = np.array([p[1] for p in pairs], np.float64)
    xs, y1, y2 = pow_pair_inputs()
    out["pow_pair_x"] = np.array(xs, np.float64)
    for k, ys in (("1", y1), ("2", y2)):
        pairs = [dd(mp.power(mp.mpf(x), mp.mpf(y))) for x, y in zip(xs, ys)]
        out["pow_pair_y" + k] = np.array(ys, np.float64)
        out["pow_pair_hi" + k] = np.array([p[0] for p in pairs], np.float64)
        out["pow_pair_lo" + k] = np.array([p[1] for p in pairs], np.float64)
    return out


if __name__ == "__main__":
    data = generate()
    np.savez_compressed(OUT, **data)
    print(f"{OUT}: {len(data)} arrays, {os.path.getsize(OUT)} bytes")
