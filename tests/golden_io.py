"""Fixture loading and comparison helpers shared by the CPU and GPU tests."""
from __future__ import annotations

import glob
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load(name: str) -> dict:
    with np.load(os.path.join(GOLDEN, name), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def load_params(veg: str = "USGS", soil: str = "STAS") -> dict:
    return load(f"params_ref_{veg}_{soil}.npz")


def fixture_tags(g: dict) -> tuple[str, str]:
    """(soil, veg) parameter-table tags a fixture was generated with (default STAS/USGS)."""
    return (str(g["soil"]) if "soil" in g else "STAS", str(g["veg"]) if "veg" in g else "USGS")


def fixture_params(g: dict) -> dict:
    """The table values a fixture was generated with: stored in the fixture
    itself (param_<name> arrays) where the reference read an edited table,
    else the dump of the shipped tables the fixture's tags name."""
    if any(k.startswith("param_") for k in g):
        return {k[6:]: (v if v.ndim else v[()]) for k, v in g.items() if k.startswith("param_")}
    soil, veg = fixture_tags(g)
    return load_params(veg, soil)


def single_names() -> list[str]:
    return sorted(os.path.basename(p)[7:-4] for p in glob.glob(os.path.join(GOLDEN, "single_*.npz")))


# Grouped fixtures (tests/golden/make_layers_golden.py): several launches in one
# file, each with its own soil layering and time step.  zsoil (G, 4), dt,
# yearlen, julian or julian0 (G,) are per group; group (ncol,) holds each
# column's group number 1..G; the arrays below carry the columns on their last axis.
GROUP_SCALARS = ("zsoil", "dt", "yearlen", "julian", "julian0")
GROUP_COLUMNS = ("state0", "isnow0", "static_f", "static_i", "forcing", "state1", "isnow1", "diag",
                 "status", "states", "isnows", "diags", "statuses")


def layer_groups(g: dict) -> list[int]:
    """The group numbers of a grouped fixture (1..G, as its generator's table counts them)."""
    return list(range(1, g["zsoil"].shape[0] + 1))


def layer_group(g: dict, k: int) -> dict:
    """Group k (1..G) of a grouped fixture as a dict in the single-call (or
    trajectory) format: its own zsoil (4,), scalar dt, yearlen and julian, and
    the columns of the group."""
    assert 1 <= k <= g["zsoil"].shape[0], k
    cols = g["group"] == k
    out = {}
    for key, v in g.items():
        if key == "group":
            continue
        if key in GROUP_SCALARS:
            out[key] = v[k - 1]
        elif key in GROUP_COLUMNS:
            out[key] = np.ascontiguousarray(v[..., cols])
        else:
            out[key] = v
    return out


def bit_equal(a, b) -> np.ndarray:
    """Elementwise identical (NaN == NaN), per element."""
    a = np.asarray(a)
    b = np.asarray(b)
    return (a == b) | (np.isnan(a) & np.isnan(b)) if a.dtype.kind == "f" else (a == b)


def close(got, exp, rtol, atol) -> np.ndarray:
    got = np.asarray(got, np.float64)
    exp = np.asarray(exp, np.float64)
    same = (got == exp) | (np.isnan(got) & np.isnan(exp))
    with np.errstate(invalid="ignore", over="ignore"):
        return same | (np.abs(got - exp) <= atol + rtol * np.abs(exp))


def column_mismatch(got, exp, rtol, atol, names=None):
    """(bad-column mask, per-field worst report) for SoA arrays (nfield, n)."""
    ok = close(got, exp, rtol, atol)
    bad_cols = ~ok.all(axis=0)
    rep = []
    for f in np.nonzero(~ok.all(axis=1))[0]:
        i = np.nonzero(~ok[f])[0]
        d = np.abs(np.asarray(got[f, i], np.float64) - np.asarray(exp[f, i], np.float64))
        j = i[np.nanargmax(d)] if np.isfinite(d).any() else i[0]
        rep.append(f"{names[f] if names else f}: {i.size} cols, worst col {j} "
                   f"got {got[f, j]!r} exp {exp[f, j]!r}")
    return bad_cols, rep


def as_ref_status(status) -> np.ndarray:
    """Engine status bits as the reference harness can observe them.

    The reference raises FIRE<=0 (module_noahmp_func.f90:1291) and ZLVL<=ZPD
    (:3414) with the same message "STOP in Noah-MP", so its harness
    (oracle/ref_harness.f90) records both as ST_STOP (128)."""
    s = np.asarray(status, np.int32).copy()
    hit = (s & (4 | 16)) != 0
    s[hit] = (s[hit] & ~(4 | 16)) | 128
    return s


# Parity bar against the reference fixtures (SURVEY.md 8c tolerances).  A
# one-ulp libm difference can change a Newton iteration count or a limiter
# branch (H12), so the bar is per column: TOL_FRAC of the columns must be
# inside the tight tolerance and every column inside the loose envelope,
# except for columns where the reference itself sits on a threshold tie (ISNOW
# or a fatal-status flip), which are counted separately.
STATE_TOL = (1e-5, 1e-4)    # rel, abs (K, m, mm, m3/m3 ...)
DIAG_TOL = (1e-4, 1e-2)     # rel, abs (W/m2, mm/s ...)
STATE_LOOSE = (1e-3, 1e-3)
DIAG_LOOSE = (2e-2, 1.0)
TOL_FRAC = 0.97     # columns inside the tight tolerance
LOOSE_FRAC = 0.995  # non-tie columns inside the loose envelope
TIE_FRAC = 0.02     # columns with an ISNOW or fatal-status flip


def parity_vs_reference(st, isn, dg, status, g, state_key="state1", diag_key="diag",
                        isnow_key="isnow1", status_key="status", tol_frac=TOL_FRAC,
                        loose_frac=LOOSE_FRAC, tie_frac=TIE_FRAC):
    """Returns a dict of per-column fractions and a failure message (or '')."""
    est, edg = g[state_key], g[diag_key]
    tie = (isn != g[isnow_key]) | (as_ref_status(status) != g[status_key])
    tight = close(st, est, *STATE_TOL).all(0) & close(dg, edg, *DIAG_TOL).all(0)
    loose = close(st, est, *STATE_LOOSE).all(0) & close(dg, edg, *DIAG_LOOSE).all(0)
    exact = (bit_equal(st, est).all(0) & bit_equal(dg, edg).all(0))
    r = dict(n=int(isn.size), exact=float(exact.mean()), tight=float(tight.mean()),
             loose_nontie=float(loose[~tie].mean()) if (~tie).any() else 1.0,
             tie=float(tie.mean()))
    msg = []
    if r["tight"] < tol_frac and (~tight).sum() > 1:
        msg.append(f"only {r['tight']:.3f} of columns within the tight tolerance")
    if r["loose_nontie"] < loose_frac and (~loose & ~tie).sum() > 1:
        msg.append(f"{int((~loose & ~tie).sum())} non-tie columns outside the loose envelope")
    if r["tie"] > tie_frac and tie.sum() > 1:
        msg.append(f"{int(tie.sum())} columns with ISNOW/status flips")
    if msg:
        _, rep_s = column_mismatch(st[:, ~tie], est[:, ~tie], *STATE_LOOSE)
        _, rep_d = column_mismatch(dg[:, ~tie], edg[:, ~tie], *DIAG_LOOSE)
        msg.append("loose-envelope misses: " + "; ".join(rep_s[:6] + rep_d[:6]))
    return r, " | ".join(msg)


# fp64 engine vs the fp32 reference ("fp64 build vs fp32 oracle:
# same thresholds x10").  The reference cannot be built in fp64 (H11,
# core/module_noahmp_func.f90:392-393, :442, :2765), so the fp64 path is held
# to the fp32 reference with the tolerances widened tenfold.  Residual misses
# are columns whose Newton/bisection loops exit on a different iteration in
# fp64 than in fp32 (the exit tests compare against fixed thresholds, e.g.
# vege_flux :2870-2875); tests/test_oracle_golden.py pins that explanation with
# the oracle's trip-count builds.  Status: the energy/radiation balance checks
# (ERRSW/ERRENG, :688-721) fire on fp32 round-off of ~1e3 W/m2 terms against a
# 0.01 W/m2 threshold, so only the hard-stop bits are compared in fp64.
FP64_STATE_TOL = (1e-4, 1e-3)   # x10 of STATE_TOL
FP64_DIAG_TOL = (1e-3, 1e-1)    # x10 of DIAG_TOL
FP64_STATE_ENV = (1e-2, 1e-2)   # envelope for the loop-exit residuals
FP64_DIAG_ENV = (5e-2, 2.0)
FP64_TOL_FRAC = 0.97            # per fixture, non-tie columns inside the x10 bar
FP64_POOLED_FRAC = 0.985        # pooled over every fixture
HARD_STATUS = 4 | 8 | 16 | 64 | 128   # FIRE, HCAN, ZLVL, OPTVEG, STOP


def parity_fp64_vs_reference(st, isn, dg, status, g, state_key="state1", diag_key="diag",
                             isnow_key="isnow1", status_key="status"):
    """fp64 result vs an fp32 reference fixture at SURVEY 8c's x10 bar.

    Returns (summary dict, per-column miss mask of non-tie columns outside the
    x10 bar, per-column envelope-miss mask, field report of the misses)."""
    est, edg = g[state_key], g[diag_key]
    hard = lambda s: as_ref_status(s) & HARD_STATUS
    tie = (isn != g[isnow_key]) | (hard(status) != hard(g[status_key]))
    tight = close(st, est, *FP64_STATE_TOL).all(0) & close(dg, edg, *FP64_DIAG_TOL).all(0)
    env = close(st, est, *FP64_STATE_ENV).all(0) & close(dg, edg, *FP64_DIAG_ENV).all(0)
    miss = ~tight & ~tie
    env_miss = ~env & ~tie
    nt = max(int((~tie).sum()), 1)
    r = dict(n=int(isn.size), nontie=int((~tie).sum()), tight=int((tight & ~tie).sum()),
             frac=float((tight & ~tie).sum() / nt), miss=int(miss.sum()),
             env_miss=int(env_miss.sum()), tie=int(tie.sum()))
    rep = []
    if miss.any():
        from noahmp_amd import layout as L
        names = [f"{n}[{k}]" if w > 1 else n for n, w in L.STATE_FIELDS for k in range(w)]
        rep = (column_mismatch(st[:, miss], est[:, miss], *FP64_STATE_TOL, names)[1]
               + column_mismatch(dg[:, miss], edg[:, miss], *FP64_DIAG_TOL, L.DIAG_FULL)[1])
    return r, miss, env_miss, rep


def check_fp64_trajectory_step(name, s, st, isn, dg, g, k):
    """Shared by the CPU (fp64 restatement) and GPU (fp64 engine) trajectory tests."""
    from noahmp_amd import layout as L
    exp, edg = g["states"][k], g["diags"][k]
    ok = close(st, exp, 1e-3, 1e-3).all(0) & close(dg, edg, 1e-3, 1e-1).all(0) & \
        (isn == g["isnows"][k])
    if name == "snow":
        for f in ("SNEQV", "SNOWH"):
            a, b = st[L.si(f)].mean(), exp[L.si(f)].mean()
            assert abs(a - b) <= 0.01 * abs(b) + 1e-3, (s, f, a, b)
        assert abs((isn < 0).mean() - (g["isnows"][k] < 0).mean()) <= 0.01 + 1.0 / isn.size
    else:
        if name == "casenml":
            assert ok[0], (name, s, "the run/case.nml column is outside the x10 trajectory bar")
        assert ok.mean() >= 0.9, (name, s, ok.mean())
    return float(ok.mean())


# fp64 engine vs the fp64 restatement.  The engine differs from the
# restatement only where it evaluates an expression differently: ocml instead
# of glibc, exp(y log x) powers, square-root fourth roots, the Newton loops'
# reciprocal division, tdfcnd's fused exp (oracle/noahmp_oracle.c
# ORACLE_PERTURB lists the sites).  oracle/port.py step_ensemble runs the
# restatement with each of those values moved within its device bound, 28
# members; per column that gives `discrete` (a member changed ISNOW, status or
# a loop trip count) and q (the largest member deviation in units of the bar).
# One rule, no fractions:
#  * a column that is not discrete has the base's ISNOW and status, and every
#    value within FP64_BAR max(1, FP64_Q_MARGIN q) (1 + |base|).  The factor 2
#    is the margin over the ensemble: the engine's fixed error pattern can
#    exceed 28 random sign patterns.  For q <= 0.5 that is the plain bar.
#  * discrete columns are named, stay inside the loop-exit envelope
#    (FP64_STATE_ENV / FP64_DIAG_ENV), and number at most FP64_DISCRETE_FRAC of
#    a fixture and FP64_DISCRETE_POOLED of all fixture columns pooled.
FP64_BAR = 1e-9
FP64_Q_MARGIN = 2.0
FP64_DISCRETE_FRAC = 0.01
FP64_DISCRETE_POOLED = 0.001


def perturb_bounds() -> dict:
    """Bounds in ulps of the perturbed restatement's site kinds: what
    tests/test_gpu_math64.py asserts of the device functions (the recorded
    maxima of profiles/math64/ulp.json plus its MARGIN; 1.5 / 2.5 for the
    square-root fourth roots), 1 ulp for the reciprocal division
    (tests/test_gpu_routines.py) and ocml's stated 1 ulp plus MARGIN for the
    one double pow of the water-table routine."""
    import json
    from test_gpu_math64 import MARGIN, OCML, ULP_JSON
    with open(ULP_JSON) as f:
        m = json.load(f)["max_ulp"]
    b = {fn: m[fn] + MARGIN for fn in OCML}
    b.update(pow_q=1.5, pow_mq=2.5, div=1.0, pow_d=1.0 + MARGIN)
    return b


def bar_units(got, base) -> np.ndarray:
    """|got - base| / (FP64_BAR (1 + |base|)) per element; identical elements
    (NaN == NaN, inf == inf) are 0, a non-finite one against a finite one inf."""
    got, base = np.asarray(got, np.float64), np.asarray(base, np.float64)
    same = (got == base) | (np.isnan(got) & np.isnan(base))
    with np.errstate(invalid="ignore", over="ignore"):
        u = np.abs(got - base) / (FP64_BAR * (1.0 + np.abs(base)))
    return np.where(same, 0.0, np.where(np.isnan(u), np.inf, u))


def check_fp64_rule(what, groups, isn, status, base_isn, base_status, discrete, q, pool=None):
    """The rule above.  groups: [(got(nf, n), base(nf, n), field names,
    (rtol, atol) envelope)].  Prints and returns the record
    {n, worst (in units of the column's tolerance), column, field, q_max,
    discrete: [columns]}, appends it to `pool` (for check_fp64_pooled and the
    envelope record) and asserts the rule."""
    n = int(q.size)
    scale = np.maximum(1.0, FP64_Q_MARGIN * np.asarray(q, np.float64))
    ratio = np.zeros(n)
    field = np.full(n, "", dtype=object)
    env_ok = np.ones(n, bool)
    for got, base, names, env in groups:
        u = bar_units(got, base) / scale
        k = u.argmax(axis=0)
        best = u[k, np.arange(n)]
        up = best > ratio
        ratio = np.where(up, best, ratio)
        field[up] = np.asarray(names, dtype=object)[k[up]]
        env_ok &= close(got, base, *env).all(0)
    held = ~discrete
    flip = held & ((isn != base_isn) | (status != base_status))
    masked = np.where(held, ratio, 0.0)
    c = int(masked.argmax()) if n else 0
    rec = dict(what=what, n=n, worst=float(masked[c]) if n else 0.0, column=c,
               field=str(field[c]) if n else "", q_max=float(np.max(q)) if n else 0.0,
               q_at_worst=float(q[c]) if n else 0.0,
               discrete=[int(i) for i in np.nonzero(discrete)[0]])
    print(f"{what}: worst {rec['worst']:.4f} of the tolerance at column {c} ({rec['field']}, "
          f"q {rec['q_at_worst']:.3f}); q max {rec['q_max']:.3f}; discrete {rec['discrete']}")
    if pool is not None:
        pool.append(rec)
    assert not flip.any(), f"{what}: ISNOW or status differs on held columns " \
        f"{list(np.nonzero(flip)[0][:8])}"
    over = held & ~(ratio <= 1.0)
    assert not over.any(), \
        f"{what}: {int(over.sum())} columns outside 1e-9 max(1, 2q)(1 + |x|): " + "; ".join(
            f"col {i} {field[i]} {ratio[i]:.3g}x (q {q[i]:.3g})" for i in np.nonzero(over)[0][:8])
    bad_env = discrete & ~env_ok
    assert not bad_env.any(), f"{what}: discrete columns {list(np.nonzero(bad_env)[0][:8])} " \
        "outside the loop-exit envelope"
    assert discrete.sum() <= FP64_DISCRETE_FRAC * n, (what, rec["discrete"])
    return rec


def check_fp64_pooled(records):
    """The pooled cap on discrete columns over records of check_fp64_rule, one
    per column set (not one per kernel variant)."""
    tot_n = sum(r["n"] for r in records)
    tot_d = sum(len(r["discrete"]) for r in records)
    print(f"fp64 discrete columns pooled: {tot_d} of {tot_n}")
    assert tot_d <= FP64_DISCRETE_POOLED * tot_n, \
        f"{tot_d} discrete columns of {tot_n} pooled: " + str(
            [(r["what"], r["discrete"]) for r in records if r["discrete"]])


def fixture_step_args(g: dict):
    """port.step's positional arguments for a single-call fixture, with the
    table values the fixture was generated with."""
    return (fixture_params(g), tuple(g["options"]), g["zsoil"], float(g["dt"]), int(g["yearlen"]),
            float(g["julian"]), g["state0"], g["isnow0"], g["static_f"], g["static_i"],
            g["forcing"])


_ENSEMBLES = {}


def fixture_ensemble(port, fname: str, group: int | None = None):
    """port.step_ensemble of the fixture file `fname` (of its group `group`,
    for a grouped fixture) at amplitude 1, computed once per session and
    shared (read-only) by every test that needs it."""
    key = fname if group is None else (fname, group)
    if key not in _ENSEMBLES:
        g = load(fname) if group is None else layer_group(load(fname), group)
        base, discrete, q = port.step_ensemble(*fixture_step_args(g), perturb_bounds())
        for a in (*base, discrete, q):
            a.setflags(write=False)
        _ENSEMBLES[key] = (base, discrete, q)
    return _ENSEMBLES[key]
