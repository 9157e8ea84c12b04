"""The perturbed fp64 restatement (oracle/noahmp_oracle.c ORACLE_PERTURB,
port.step_ensemble): the conditions the fp64 engine's GPU rule rests on
(golden_io.check_fp64_rule), checked on the CPU, and the restatement's T2M.

 * mode 0 is the plain fp64 build bit for bit, and its trip counts are the
   trip-count build's;
 * a member is a function of (mode, seed) alone;
 * over every single-call and branch fixture, moving every libm result, power
   and Newton-loop division within its device bound changes no ISNOW, status
   or loop trip count and moves no value by more than the bar: the engine's
   1e-9 misses could not be explained by those bounds;
 * the trip-count recorder is live: at 1e10 times the bounds it fires.
"""
import numpy as np
import pytest

from golden_io import (bit_equal, fixture_ensemble, fixture_step_args, load, perturb_bounds,
                       single_names)
from noahmp_amd import layout as L
from test_branch_golden import SINGLES as BRANCH_SINGLES

FIXTURES = ["single_" + n for n in single_names()] + ["branch_" + n for n in BRANCH_SINGLES]


def _same(a, b):
    return all(bit_equal(x, y).all() for x, y in zip(a, b))


@pytest.mark.parametrize("fname", ["single_casenml_mixed", "single_veg2", "branch_combo"])
def test_mode0_is_the_plain_fp64_build(oracle_port, fname):
    args = fixture_step_args(load(fname + ".npz"))
    plain = oracle_port.step(*args, precision=8)
    stats = oracle_port.step_stats(*args, precision=8)
    base, _, _ = oracle_port.step_ensemble(*args, perturb_bounds(), members=())
    assert _same(plain, base[:4])
    assert _same(stats[:4], base[:4]) and np.array_equal(stats[4], base[4])
    assert base[4].sum() > 0   # the recorder ran


def test_bounds_come_from_the_device_record():
    """Every site kind port names has a bound or is formed per call; the ocml
    kinds are the recorded maxima plus the margin."""
    import port
    b = perturb_bounds()
    assert set(b) == set(port.PERTURB_SITES) - {"pow", "tdf"}
    assert all(0.5 <= v <= 4.0 for v in b.values()), b


def test_members_are_reproducible(oracle_port):
    import port
    args = fixture_step_args(load("single_casenml_mixed.npz"))
    members = port.FIXED_MEMBERS + ((5, 1), (5, 2))
    runs = [[oracle_port._member_step(perturb_bounds(), mode, seed, 1.0, args)
             for mode, seed in members] for _ in range(2)]
    for (mode, seed), a, b in zip(members, *runs):
        assert _same(a, b), (mode, seed)
    # and the members differ from the base and from each other
    base = oracle_port._member_step(perturb_bounds(), 0, 0, 1.0, args)
    outs = [base] + runs[0]
    for i in range(len(outs)):
        for j in range(i):
            assert not bit_equal(outs[i][0], outs[j][0]).all(), (i, j)


@pytest.mark.parametrize("fname", FIXTURES)
def test_no_discrete_columns_and_q_within_the_bar(oracle_port, fname):
    """Amplitude 1: no member changes ISNOW, status or a trip count on any
    column, and q <= 1 everywhere (DESIGN.md "fp64" records the worst q)."""
    base, discrete, q = fixture_ensemble(oracle_port, fname + ".npz")
    print(f"{fname}: n {q.size} worst q {q.max():.4f} at column {int(q.argmax())}")
    assert not discrete.any(), list(np.nonzero(discrete)[0][:8])
    assert (q <= 1.0).all(), (float(q.max()), int(q.argmax()))


def test_recorder_is_live(oracle_port):
    """At 1e10 times the bounds the perturbation reaches the loop exits."""
    args = fixture_step_args(load("single_casenml_mixed.npz"))
    _, discrete, q = oracle_port.step_ensemble(*args, perturb_bounds(),
                                               members=tuple((5, s) for s in range(1, 9)),
                                               amplitude=1e10)
    print("discrete at 1e10:", int(discrete.sum()), "of", discrete.size)
    assert discrete.any()


@pytest.mark.parametrize("name", single_names())
def test_restatement_t2m_is_the_fveg_blend(oracle_port, name):
    """The fp32 restatement's T2M (port.step_t2m) against a float32 formula on
    the reference fixture's own FVEG / T2MV / T2MB: the blend bit for bit
    wherever FCTR or FCEV is nonzero (only the vegetated branch sets them, to
    TR and EVC), T2MB wherever FVEG is 0."""
    g = load(f"single_{name}.npz")
    *out, t2m = oracle_port.step_t2m(*fixture_step_args(g), precision=4)
    assert bit_equal(out[2], g["diag"]).all()   # the hook leaves the outputs alone
    d = lambda n: g["diag"][L.DIAG_FULL.index(n)].astype(np.float32)  # noqa: E731
    fveg, t2mv, t2mb = d("FVEG"), d("T2MV"), d("T2MB")
    one = np.float32(1.0)
    blend = fveg * t2mv + (one - fveg) * t2mb
    assert blend.dtype == np.float32
    veg = (d("FCTR") != 0) | (d("FCEV") != 0)
    assert bit_equal(t2m[veg], blend[veg]).all(), int((~bit_equal(t2m[veg], blend[veg])).sum())
    bare = fveg == 0
    assert bit_equal(t2m[bare], t2mb[bare]).all()
    if name == "casenml_mixed":
        assert veg.any() and bare.any()


def _rule(oracle_port, mutate=None, member=None, discrete_override=None):
    """check_fp64_rule on single_casenml_mixed with the base itself (or a
    perturbed member) standing in for the engine."""
    from golden_io import FP64_DIAG_ENV, FP64_STATE_ENV, check_fp64_rule
    (st, isn, dg, status, _, _), discrete, q = fixture_ensemble(oracle_port,
                                                                "single_casenml_mixed.npz")
    got = [st.copy(), isn.copy(), dg.copy(), status.copy()]
    if member is not None:
        args = fixture_step_args(load("single_casenml_mixed.npz"))
        got = [np.array(a) for a in oracle_port._member_step(perturb_bounds(), *member, args)[:4]]
    if mutate is not None:
        mutate(*got)
    d = discrete if discrete_override is None else discrete_override
    names = [f"s{k}" for k in range(st.shape[0])]
    return check_fp64_rule("self-test", [(got[0], st, names, FP64_STATE_ENV),
                                         (got[2], dg, L.DIAG_FULL, FP64_DIAG_ENV)],
                           got[1], got[3], isn, status, d, q)


def test_rule_holds_every_column(oracle_port):
    """The rule itself: the base and a member outside the ensemble pass; one
    value of one column 3e-9 (1 + |x|) off, one ISNOW, one status bit, or an
    engine with 1000 times the device bounds do not; a discrete column is
    excused from the bar but not from the envelope, and not beyond 1 %."""
    col = 1234
    rec = _rule(oracle_port)
    assert rec["worst"] == 0.0 and rec["discrete"] == []
    rec = _rule(oracle_port, member=(5, 99, 1.0))
    assert 0.0 < rec["worst"] <= 1.0

    def nudge(rel):
        def f(st, isn, dg, status):
            k = L.DIAG_FULL.index("FSH")
            dg[k, col] += rel * (1.0 + abs(dg[k, col]))
        return f
    assert _rule(oracle_port, nudge(0.9e-9))["column"] == col
    with pytest.raises(AssertionError, match=f"col {col} FSH"):
        _rule(oracle_port, nudge(3e-9))

    def snow(st, isn, dg, status):
        isn[col] -= 1
    with pytest.raises(AssertionError, match="ISNOW or status"):
        _rule(oracle_port, snow)

    def stat(st, isn, dg, status):
        status[col] ^= 2
    with pytest.raises(AssertionError, match="ISNOW or status"):
        _rule(oracle_port, stat)
    with pytest.raises(AssertionError, match="outside 1e-9"):
        _rule(oracle_port, member=(1, 0, 1000.0))
    # a discrete column: excused from the bar, not from the envelope or the cap
    n = 2048
    one = np.zeros(n, bool)
    one[col] = True
    assert _rule(oracle_port, nudge(3e-9), discrete_override=one)["discrete"] == [col]
    with pytest.raises(AssertionError, match="loop-exit envelope"):
        _rule(oracle_port, nudge(10.0), discrete_override=one)
    many = np.zeros(n, bool)
    many[:21] = True   # 21 of 2,048 > 1 %
    with pytest.raises(AssertionError):
        _rule(oracle_port, discrete_override=many)


def test_run_ensemble_base_is_repeated_plain_steps(oracle_port):
    """The multi-step form: its base is the plain fp64 build stepped three
    times (status OR-ed over the steps, as the engine keeps it), and at
    amplitude 1 a 256-column sample has no discrete column."""
    from golden_io import load_params
    from noahmp_amd import cases
    from noahmp_amd.params import Params
    n, dt, yl = 256, 3600.0, 366
    opts = tuple(dict(L.CASE_NML_OPTIONS, opt_veg=2)[k] for k in L.OPTION_NAMES)
    cols = cases.make_columns(n, "global", Params.builtin().as_dict(), seed=4, julian=180.0)
    jul = [float(np.float32(180.0 + k * dt / 86400.0)) for k in range(3)]
    F = [cases.forcing_step(cols, j, yl, k, seed=4).astype(np.float64) for k, j in enumerate(jul)]
    base, discrete, q = oracle_port.run_ensemble(
        load_params(), opts, cases.CASE_NML_ZSOIL, dt, yl, jul, cols.state, cols.isnow,
        cols.static_f, cols.static_i, F, perturb_bounds())
    st, isn, status = cols.state, cols.isnow, 0
    for k in range(3):
        st, isn, dg, s_k = oracle_port.step(load_params(), opts, cases.CASE_NML_ZSOIL, dt, yl, jul[k],
                                            st, isn, cols.static_f, cols.static_i, F[k], precision=8)
        status = status | s_k
    assert _same((st, isn, dg, status), base[:4])
    assert base[4].shape == (n, 15)   # five loops, three steps
    assert not discrete.any() and (q <= 1.0).all(), (int(discrete.sum()), float(q.max()))
