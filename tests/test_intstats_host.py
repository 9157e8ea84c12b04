"""Interval statistics, host side (no GPU): the spec parser, the canonical spec
and the row names, the numpy restatement (intstats.update_host / output_host)
on hand-written sequences for every clause of the rule the header states, the
new enums against the header, the two C entries' declaration, export, binding
and argument rules, the restart variables of ncio, the driver's refusals and the
CLI option.

Every comparison of values is on bits; the expectations are literals."""
import datetime
import importlib.util
import os
import re
import subprocess

import numpy as np
import pytest

from noahmp_amd import build as _build, extremes as X, intstats as IS, layout as L, lib as _lib, \
    ncio
from test_abi_host import _enum_values, _header

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")
INF = float("inf")
DIAG, FORC, STATE = L.EXT_SRC_DIAG, L.EXT_SRC_FORCING, L.EXT_SRC_STATE


def ibits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(ibits(a), ibits(b))


# ---- parse / spec_string / row_names ---------------------------------------------------------
def test_parse_the_issue_examples():
    t2m, sfctmp = L.DIAG_OUT.index("T2M"), L.FORCING.index("SFCTMP")
    prcp, sneqv = L.FORCING.index("PRCP"), L.STATE_OFF["SNEQV"][0]
    assert IS.parse("T2M") == IS.parse("T2M:mean") == \
        [IS.Item("T2M", "T2M", DIAG, t2m, L.IST_NONE, 0.0, L.IST_MEAN)]
    assert IS.row_names(IS.parse("T2M")) == ["T2M_MEAN"]
    items = IS.parse("FROST=T2M@lt273.15:dur+spell,GDD=SFCTMP@gt278.15:deg,"
                     "WET=PRCP@gt0:dur+spell,SNOWCOV=SNEQV@gt1")
    assert items == [
        IS.Item("FROST", "T2M", DIAG, t2m, L.IST_LT, 273.15, L.IST_DUR | L.IST_SPELL),
        IS.Item("GDD", "SFCTMP", FORC, sfctmp, L.IST_GT, 278.15, L.IST_DEG),
        IS.Item("WET", "PRCP", FORC, prcp, L.IST_GT, 0.0, L.IST_DUR | L.IST_SPELL),
        IS.Item("SNOWCOV", "SNEQV", STATE, sneqv, L.IST_GT, 1.0, L.IST_DUR)]
    assert IS.row_names(items) == ["FROST_DUR", "FROST_SPELL", "GDD_DEG", "WET_DUR", "WET_SPELL",
                                   "SNOWCOV_DUR"]
    assert IS.spec_string(items) == ("FROST=T2M@lt273.15:dur+spell,GDD=SFCTMP@gt278.15:deg,"
                                     "WET=PRCP@gt0.0:dur+spell,SNOWCOV=SNEQV@gt1.0:dur")
    assert IS.table(items).tolist() == [[0, t2m, 3, 10], [1, sfctmp, 1, 4], [1, prcp, 1, 10],
                                        [2, sneqv, 1, 2]]
    assert IS.table(items).dtype == np.int32 and IS.thresholds(items).dtype == np.float64
    assert IS.thresholds(items).tolist() == [273.15, 278.15, 0.0, 1.0]
    assert IS.has_diag(items) and not IS.has_diag(items[1:])
    # rows come in bit order MEAN, DUR, DEG, SPELL, whatever the spec's order
    assert IS.row_names(IS.parse("F=TG@le-1.5e-3:spell+deg+dur")) == ["F_DUR", "F_DEG", "F_SPELL"]
    assert IS.parse("F=TG@le-1.5e-3:spell+deg+dur")[0].c == -0.0015


def test_round_trips_and_every_offered_name():
    assert set(IS.SOURCES) == set(X.SOURCES) and len(IS.SOURCES) == 68
    for n, (kind, row) in X.SOURCES.items():
        (it,) = IS.parse(n)
        assert it == IS.Item(n, n, kind, row, 0, 0.0, 1)
        (it,) = IS.parse(f"A_1={n}@ge0.1:deg")
        assert it == IS.Item("A_1", n, kind, row, L.IST_GE, 0.1, L.IST_DEG)
    for spec in ("T2M", "TAVG=T2M", "T2M,SMC1,TG,SNEQV", " T2M : MEAN , F = TG @ LT 273.15 : Dur ",
                 "A=PRCP@gt0,B=PRCP@ge0:spell,C=PRCP@lt1e-07:deg,D=PRCP@le-3.5:dur+deg+spell",
                 "X=FSH@gt0.1:deg", "X=FSH@gt1e+22:deg", "X=FSH@gt5e-324"):
        items = IS.parse(spec)
        canon = IS.spec_string(items)
        assert IS.parse(canon) == items and IS.spec_string(IS.parse(canon)) == canon
        assert IS.parse(items) == items and IS.parse(canon.split(",")) == items
    assert IS.spec_string(IS.parse("TAVG=T2M,T2M")) == "TAVG=T2M:mean,T2M:mean"
    assert IS.spec_string(IS.parse("X=FSH@gt0.1:deg")) == "X=FSH@gt0.1:deg"   # repr(float)
    names = sorted(X.SOURCES)
    assert len(IS.parse(names[:32])) == 32
    with pytest.raises(ValueError, match="at most 32"):
        IS.parse(names[:33])
    # no default row name collides with a flux or a state-output row; the means of the
    # energy fluxes are also accumulation's rows (OutputBlock refuses the two together)
    from noahmp_amd import stateout
    every = [r for i in range(0, 68, 32) for r in IS.row_names(IS.parse(names[i:i + 32]))]
    assert len(set(every)) == 68
    assert not set(every) & (set(L.DIAG_OUT) | set(stateout.row_names(stateout.ALL)))
    assert set(every) & set(L.BUDGET) == {n for n in L.BUDGET if n.endswith("_MEAN")}
    assert "FSH_MEAN" in L.BUDGET and "T2M_MEAN" in L.BUDGET and "TG_MEAN" not in L.BUDGET


@pytest.mark.parametrize("bad", [
    "NOPE", "t2m", "STC", "SNICE", "SNLIQ1", "STC0", "SMC5", "ISNOW", "X=NOPE@gt1",   # names
    "X=T2M@eq1", "X=T2M@g1", "X=T2M@>1", "X=T2M@", "X=T2M@gt", "X=T2M@gtabc",         # operators
    "T2M:avg", "T2M:", "T2M:mean+", "X=T2M@gt1:max", "X=T2M@gt1:",                    # stats
    "T2M:dur", "T2M:mean+dur", "X=T2M:spell", "X=T2M@gt1:mean", "X=T2M@gt1:dur+mean",  # wrong type
    "T2M@lt273.15", "T2M@lt273.15:dur", "=T2M@gt1", "x=T2M@gt1", "1X=T2M@gt1", "X-Y=T2M@gt1",
    "X Y=T2M", "ABCDEFGHIJKLMNOPQRSTUVWXY=T2M@gt1",                                    # labels
    "T2M,T2M", "T2M,T2M=TG@gt1", "X=T2M@gt1,X=TG@gt1", "X=T2M,X=TG",                   # duplicates
    "X=T2M@gtinf", "X=T2M@lt-inf", "X=T2M@genan",                                      # thresholds
    "", " , ", [], [("T2M", 1)], [5],                                                  # nothing
])
def test_parse_refusals(bad):
    with pytest.raises(ValueError, match="interval_stats"):
        IS.parse(bad)


def test_parse_refuses_bad_items():
    ok = IS.parse("X=TG@gt1")[0]
    assert len("ABCDEFGHIJKLMNOPQRSTUVWX") == 24 and IS.parse("ABCDEFGHIJKLMNOPQRSTUVWX=TG")
    for kw in (dict(row=ok.row + 1), dict(kind=0), dict(op=5), dict(op=-1), dict(stats=0),
               dict(stats=1), dict(stats=16), dict(c=INF), dict(c=NAN), dict(label="x"),
               dict(name="NOPE"), dict(op=0), dict(op=0, stats=3)):
        with pytest.raises(ValueError):
            IS.parse([ok._replace(**kw)])
    assert IS.parse([ok._replace(op=0, stats=1)])[0].op == 0


# ---- the rule ----------------------------------------------------------------------------
def run_item(values, op, c, dtype=np.float32, kind=FORC, row=8):
    """One item over len(values[0]) steps, one column per list in `values`
    (columns x steps), from prefilled garbage: (acc, cnt) after the last step."""
    v = np.array(values, dtype).T                      # (steps, columns)
    n = v.shape[1]
    acc, cnt = np.full((1, n), NAN), np.full((3, n), -7, np.int32)
    nrows = {DIAG: 16, FORC: 12, STATE: 56}[kind]
    for k in range(1, v.shape[0] + 1):
        block = np.full((nrows, n), 123, dtype)
        block[row] = v[k - 1]
        kw = {DIAG: dict(diag=block), FORC: dict(forcing=block), STATE: dict(state=block)}[kind]
        IS.update_host(acc, cnt, k, [(kind, row, op, 1 if op == 0 else 14)], [c], **kw)
    return acc[0], cnt


THR2 = [
    [3, 3, 1, 3, 3, 3, 1, 3],            # 0: spells of 2, 3 and 1
    [2, 2, 2, 2, 2, 2, 2, 2],            # 1: equal to the threshold throughout
    [3, 3, NAN, 3, 3, 1, 1, 1],          # 2: NaN breaks a spell: two spells of equal length
    [INF, -INF, INF, INF, 1, 1, 1, 1],   # 3: infinities
    [3, 1, 3, 1, 3, 1, 3, 1],            # 4: alternating
    [1, 1, 1, 1, 1, 1, 1, 1],            # 5: below throughout
    [5, 5, 5, 5, 5, 5, 5, 5],            # 6: above throughout
    [NAN] * 8,                           # 7: NaN throughout
]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_update_host_conditions_against_2(dtype):
    # (acc, count, run, longest) per column
    want = {
        L.IST_GT: [(6.0, 6, 1, 3), (0.0, 0, 0, 0), (4.0, 4, 0, 2), (INF, 3, 0, 2), (4.0, 4, 0, 1),
                   (0.0, 0, 0, 0), (24.0, 8, 8, 8), (0.0, 0, 0, 0)],
        L.IST_GE: [(6.0, 6, 1, 3), (0.0, 8, 8, 8), (4.0, 4, 0, 2), (INF, 3, 0, 2), (4.0, 4, 0, 1),
                   (0.0, 0, 0, 0), (24.0, 8, 8, 8), (0.0, 0, 0, 0)],
        L.IST_LT: [(2.0, 2, 0, 1), (0.0, 0, 0, 0), (3.0, 3, 3, 3), (INF, 5, 4, 4), (4.0, 4, 1, 1),
                   (8.0, 8, 8, 8), (0.0, 0, 0, 0), (0.0, 0, 0, 0)],
        L.IST_LE: [(2.0, 2, 0, 1), (0.0, 8, 8, 8), (3.0, 3, 3, 3), (INF, 5, 4, 4), (4.0, 4, 1, 1),
                   (8.0, 8, 8, 8), (0.0, 0, 0, 0), (0.0, 0, 0, 0)],
    }
    for op, rows in want.items():
        acc, cnt = run_item(THR2, op, 2.0, dtype)
        assert acc.dtype == np.float64 and cnt.dtype == np.int32
        for c, (a, n, run, lng) in enumerate(rows):
            assert ibits(acc)[c] == ibits(np.array([a]))[0], (op, c, acc[c])
            assert cnt[:, c].tolist() == [n, run, lng], (op, c)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_update_host_zeros_against_0(dtype):
    cols = [[-0.0, 0.0, -0.0, 0.0], [0.0, -0.0, 0.0, -0.0], [-1, 0.0, 1, -0.0]]
    for c in (0.0, -0.0):
        for op, counts in ((L.IST_GT, [0, 0, 1]), (L.IST_GE, [4, 4, 3]), (L.IST_LT, [0, 0, 1]),
                           (L.IST_LE, [4, 4, 3])):
            acc, cnt = run_item(cols, op, c, dtype)
            assert cnt[0].tolist() == counts, (op, c)
            assert ibits(acc).tolist() == ibits(np.array([0.0, 0.0, 1.0])).tolist(), (op, c)


def test_update_host_compares_in_the_engine_type():
    # float32(0.1) > 0.1 in double, but the threshold is rounded to T first: equal in fp32
    v = [[float(np.float32(0.1))] * 3]
    acc, cnt = run_item(v, L.IST_GT, 0.1, np.float32)
    assert cnt[:, 0].tolist() == [0, 0, 0] and ibits(acc)[0] == 0
    acc, cnt = run_item(v, L.IST_GE, 0.1, np.float32)
    assert cnt[:, 0].tolist() == [3, 3, 3] and ibits(acc)[0] == 0      # d = 0 exactly
    acc, cnt = run_item(v, L.IST_GT, 0.1, np.float64)
    assert cnt[:, 0].tolist() == [3, 3, 3]
    assert acc[0] == 4.4703483415009515e-09               # three adds of 1.4901161138336505e-09
    # d is formed in double from the rounded threshold: 273.15f = 273.149993896484375
    acc, cnt = run_item([[273.0, 273.15, 273.2]], L.IST_LT, 273.15, np.float32)
    assert cnt[:, 0].tolist() == [1, 0, 1] and acc[0] == 0.149993896484375
    acc, cnt = run_item([[273.0, 273.15, 273.2]], L.IST_LE, 273.15, np.float32)
    assert cnt[:, 0].tolist() == [2, 0, 2] and acc[0] == 0.149993896484375


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_update_host_mean_is_a_step_ordered_double_sum(dtype):
    cols = [
        [1, 2, 3, 4],
        [0.1, 0.1, 0.1, 0.1],
        [1, NAN, 3, 4],
        [-0.0, -0.0, -0.0, -0.0],
        [INF, 1, -INF, 1],
        [1e30, 1.0, -1e30, 1.0],          # the order of the adds shows: 1 is lost, then 1 stays
        [INF, INF, 1, 2],
    ]
    acc, cnt = run_item(cols, L.IST_NONE, 0.0, dtype, kind=STATE, row=29)
    assert (cnt == -7).all()               # a mean item never touches its cnt rows
    tenth = 0.4000000059604645 if dtype == np.float32 else 0.4
    assert acc[0] == 10.0 and acc[1] == tenth and acc[5] == 1.0 and acc[6] == INF
    assert ibits(acc)[2] == 0x7ff8000000000000     # a NaN operand travels
    assert ibits(acc)[3] == 0                      # +0.0 + -0.0 = +0.0 at k == 1
    assert ibits(acc)[4] == 0xfff8000000000000     # inf + -inf: the adder's own NaN, sign set
    out = IS.output_host(acc[None], cnt, [(STATE, 29, 0, 1)], 4, 900.0, dtype)
    assert out.dtype == dtype and out.shape == (1, 7)
    assert out[0, 0] == 2.5 and out[0, 1] == dtype(0.1) and out[0, 5] == 0.25
    assert np.isnan(out[0, 2]) and ibits(out[0])[3] == 0 and out[0, 6] == INF
    # k == 1 starts over whatever is stored
    acc2, cnt2 = np.full((1, 2), NAN), np.full((3, 2), 9, np.int32)
    st = np.zeros((56, 2), dtype)
    st[29] = [7, -2]
    IS.update_host(acc2, cnt2, 1, [(STATE, 29, L.IST_GT, 2)], [0.0], state=st)
    assert acc2.tolist() == [[7.0, 0.0]] and cnt2.tolist() == [[1, 0], [1, 0], [1, 0]]


def test_update_host_blocks_rows_and_refusals():
    rng = np.random.default_rng(0)
    d, f, s = (rng.normal(size=(r, 5)) for r in (16, 12, 56))
    tab = [(STATE, 55, 0, 1), (DIAG, 0, L.IST_GT, 2), (FORC, 11, L.IST_LE, 12)]
    thr = [0.0, 0.0, 0.0]
    acc, cnt = np.zeros((3, 5)), np.zeros((9, 5), np.int32)
    IS.update_host(acc, cnt, 1, tab, thr, d, f, s)
    IS.update_host(acc, cnt, 2, tab, thr, d, f, s)
    assert same_bits(acc[0], s[55] + s[55])
    assert same_bits(acc[1], np.where(d[0] > 0, d[0] + d[0], 0.0))
    assert same_bits(acc[2], np.where(f[11] <= 0, -f[11] - f[11], 0.0))
    assert (cnt[:3] == 0).all()
    assert cnt[3].tolist() == cnt[4].tolist() == cnt[5].tolist() == (2 * (d[0] > 0)).tolist()
    assert cnt[6].tolist() == (2 * (f[11] <= 0)).tolist()
    for kw in (dict(k=0), dict(k=-1), dict(tab=[(3, 0, 0, 1)]), dict(tab=[(-1, 0, 0, 1)]),
               dict(tab=[(0, 16, 0, 1)]), dict(tab=[(1, 12, 0, 1)]), dict(tab=[(2, 56, 0, 1)]),
               dict(tab=[(0, -1, 0, 1)]), dict(tab=[(0, 0, 5, 2)]), dict(tab=[(0, 0, -1, 2)]),
               dict(tab=[(0, 0, 0, 0)]), dict(tab=[(0, 0, 0, 2)]), dict(tab=[(0, 0, 0, 3)]),
               dict(tab=[(0, 0, 1, 1)]), dict(tab=[(0, 0, 1, 3)]), dict(tab=[(0, 0, 1, 16)]),
               dict(tab=[(0, 0, 1, 2)], thr=[NAN]), dict(tab=[(0, 0, 1, 2)], thr=[INF]),
               dict(tab=[]), dict(tab=[(2, 0, 0, 1)] * 33), dict(thr=[0.0, 0.0])):
        a = dict(k=1, tab=[(0, 0, 0, 1)])
        a.update(kw)
        n = max(len(a["tab"]), 1)
        a.setdefault("thr", [0.0] * len(a["tab"]))
        with pytest.raises(ValueError):
            IS.update_host(np.zeros((n, 5)), np.zeros((3 * n, 5), np.int32), a["k"], a["tab"],
                           a["thr"], d, f, s)
    # a mean item's threshold is not looked at
    IS.update_host(np.zeros((1, 5)), np.zeros((3, 5), np.int32), 1, [(0, 0, 0, 1)], [NAN], d)
    with pytest.raises(ValueError, match="missing"):
        IS.update_host(np.zeros((1, 5)), np.zeros((3, 5), np.int32), 1, [(1, 0, 0, 1)], [0.0],
                       diag=d, state=s)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_output_host_rows(dtype):
    acc = np.array([[10.0, 1.0, NAN, 1e300], [6.0, 0.1, INF, 0.0], [2.0, 3.0, 4.0, 5.0]])
    cnt = np.array([[9, 9, 9, 9], [9, 9, 9, 9], [9, 9, 9, 9],
                    [6, 1, 3, 0], [1, 0, 0, 0], [3, 1, 2, 0],
                    [2, 2 ** 31 - 1, 0, 7], [0, 0, 0, 0], [1, 5, 0, 7]], np.int32)
    tab = [(DIAG, 0, 0, 1), (FORC, 0, L.IST_GT, 2 | 4 | 8), (STATE, 0, L.IST_LE, 8 | 2)]
    a0, c0 = acc.copy(), cnt.copy()
    out = IS.output_host(acc, cnt, tab, 3, 900.0, dtype)
    assert same_bits(acc, a0) and np.array_equal(cnt, c0)
    assert out.dtype == dtype and out.shape == (6, 4)
    big = INF if dtype == np.float32 else 1e300 / 3.0
    want = np.array([[10.0 / 3.0, 1.0 / 3.0, NAN, big],          # MEAN: one double division
                     [5400.0, 900.0, 2700.0, 0.0],               # DUR
                     [5400.0, 0.1 * 900.0, INF, 0.0],            # DEG: one double product
                     [2700.0, 900.0, 1800.0, 0.0],               # SPELL
                     [1800.0, (2.0 ** 31 - 1) * 900.0, 0.0, 6300.0],   # DUR of item 2
                     [900.0, 4500.0, 0.0, 6300.0]]).astype(dtype)      # SPELL of item 2
    assert same_bits(out, want)
    assert ibits(np.array([10.0 / 3.0]))[0] == 0x400aaaaaaaaaaaab
    # dt that is not exact: one rounded double product, then one conversion
    out = IS.output_host(acc, cnt, tab, 7, 0.1, dtype)
    assert same_bits(out[1], np.array([dtype(6 * 0.1), dtype(0.1), dtype(3 * 0.1), 0], dtype))
    assert same_bits(out[0, :2], np.array([dtype(10.0 / 7.0), dtype(1.0 / 7.0)], dtype))
    for kw in (dict(k=0), dict(k=-3), dict(dt=0.0), dict(dt=-900.0), dict(dt=NAN), dict(dt=INF),
               dict(tab=[(0, 0, 0, 1), (1, 0, 1, 1), (2, 0, 4, 10)]),
               dict(tab=[(0, 0, 0, 2), (1, 0, 1, 2), (2, 0, 4, 10)]),
               dict(tab=[(0, 0, 0, 1), (1, 0, 1, 0), (2, 0, 4, 10)]),
               dict(tab=[(0, 0, 0, 1), (1, 0, 1, 16), (2, 0, 4, 10)])):
        a = dict(k=3, dt=900.0, tab=tab)
        a.update(kw)
        with pytest.raises(ValueError):
            IS.output_host(acc, cnt, a["tab"], a["k"], a["dt"], dtype)


# ---- header, enums, ABI -------------------------------------------------------------------
def test_layout_mirrors_the_header_enums():
    text = _header()
    e = _enum_values(text)
    assert (e["NMP_IST_NONE"], e["NMP_IST_GT"], e["NMP_IST_GE"], e["NMP_IST_LT"],
            e["NMP_IST_LE"]) == (L.IST_NONE, L.IST_GT, L.IST_GE, L.IST_LT, L.IST_LE) == \
        (0, 1, 2, 3, 4)
    assert (e["NMP_IST_MEAN"], e["NMP_IST_DUR"], e["NMP_IST_DEG"], e["NMP_IST_SPELL"]) == \
        (L.IST_MEAN, L.IST_DUR, L.IST_DEG, L.IST_SPELL) == (1, 2, 4, 8)
    assert L.IST_OPS == {"gt": 1, "ge": 2, "lt": 3, "le": 4}
    assert L.IST_STATS == {"MEAN": 1, "DUR": 2, "DEG": 4, "SPELL": 8}
    assert [b for _, b in IS.STAT_ORDER] == [1, 2, 4, 8]
    assert int(re.search(r"#define NMP_IST_MAXITEMS (\d+)", text).group(1)) == \
        L.IST_MAXITEMS == 32
    assert not [n for n in e if n.startswith("NMP_E_") and "IST" in n]
    i = text.index("Interval statistics (no counterpart")
    words = re.sub(r"\s*\n \*\s*", " ", text[i:text.index("int nmp_intstats_update", i)])
    for w in ("the old acc and cnt are not read: they count as +0.0 and 0",
              "acc = acc + (double)v, one double add per step",
              "h = v OP cT, compared in T: a NaN never holds, -0 and +0 compare equal",
              "d = (double)v - (double)cT for GT and GE, d = (double)cT - (double)v for LT and LE",
              "count += 1; run += 1; longest = max(longest, run)",
              "Otherwise run = 0 and nothing else changes",
              "A store that would write the value already there may be skipped",
              "A mean item never touches its cnt rows",
              "(T)(acc / (double)k)", "(T)((double)count * dt)", "(T)(acc * dt)",
              "(T)((double)longest * dt)", "It changes neither acc nor cnt",
              "neither synchronise nor allocate", "then ncol == 0 is NMP_OK"):
        assert w in words, w


def test_entries_declared_exported_and_bound(engine_lib):
    decl = set(re.findall(r"^\s*(?:int|int64_t|void\*?|const char\*)\s*(nmp_\w+)\s*\(", _header(),
                          re.M))
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.library_path()], capture_output=True,
                        text=True, check=True).stdout
    exported = set(re.findall(r"\bT (nmp_\w+)$", nm, re.M))
    for name in ("nmp_intstats_update", "nmp_intstats_output"):
        assert name in decl, f"{name} not declared in the header"
        assert name in _lib.EXPORTED_SYMBOLS and name in exported
        assert getattr(engine_lib, name).argtypes is not None, f"{name} not bound in lib.py"
    assert "intstats.hip" in _build.SOURCES
    assert os.path.exists(os.path.join(_build.CSRC, "intstats.hip"))
    assert re.search(r"#define NMP_ABI_VERSION 8\b", _header())
    assert engine_lib.nmp_abi_version() == 8   # additive: the version stays
    # no new -DNMP_* switch
    src = open(os.path.join(_build.CSRC, "intstats.hip")).read()
    assert not re.search(r"#\s*if(n?def)?\b", src)


def test_entries_refuse_bad_arguments_without_an_engine(engine_lib):
    """Every refused case, with NULL handles (no device is touched)."""
    import ctypes as C
    i32 = lambda *v: (C.c_int32 * len(v))(*v)  # noqa: E731
    f64 = lambda *v: (C.c_double * len(v))(*v)  # noqa: E731

    def upd(ncol=1, ld=1, ni=1, items=(0, 0, 0, 1), thr=(0.0,), k=1, ld_st=1):
        return engine_lib.nmp_intstats_update(None, ncol, ld, ni, i32(*items), f64(*thr), None,
                                              None, None, k, None, None, ld_st, None)

    def out(ncol=1, ni=1, items=(0, 0, 0, 1), k=1, dt=900.0, ld_st=1, ld_out=1):
        return engine_lib.nmp_intstats_output(None, ncol, ni, i32(*items), k, dt, None, None,
                                              ld_st, None, ld_out, None)
    big = 1 << 29
    assert upd() == -1 and out() == -1
    assert upd(ncol=0, ld=0, ld_st=0) == -1 and out(ncol=0, ld_st=0, ld_out=0) == -1  # no engine
    assert upd(ncol=-1) == -1 and out(ncol=-1) == -1
    assert upd(ncol=2) == -1 and upd(ncol=2, ld=2) == -1 and upd(ncol=2, ld_st=2) == -1
    assert out(ncol=2) == -1 and out(ncol=2, ld_st=2) == -1 and out(ncol=2, ld_out=2) == -1
    assert upd(ld=big) == -1 and upd(ld_st=big) == -1
    assert out(ld_st=big) == -1 and out(ld_out=big) == -1
    for ni in (0, -1, 33):
        assert upd(ni=ni, items=(0, 0, 0, 1) * 33, thr=(0.0,) * 33) == -1
        assert out(ni=ni, items=(0, 0, 0, 1) * 33) == -1
    for items in ((3, 0, 0, 1), (-1, 0, 0, 1), (0, 16, 0, 1), (1, 12, 0, 1), (2, 56, 0, 1),
                  (0, -1, 0, 1), (0, 0, 5, 2), (0, 0, -1, 2), (0, 0, 0, 0), (0, 0, 0, 2),
                  (0, 0, 0, 3), (0, 0, 1, 1), (0, 0, 1, 3), (0, 0, 1, 16), (0, 0, 1, 0)):
        assert upd(items=items) == -1 and out(items=items) == -1
    for thr in (NAN, INF, -INF):
        assert upd(items=(0, 0, 1, 2), thr=(thr,)) == -1
    for k in (0, -1):
        assert upd(k=k) == -1 and out(k=k) == -1
    for dt in (0.0, -900.0, NAN, INF, -INF):
        assert out(dt=dt) == -1
    assert engine_lib.nmp_intstats_update(None, 1, 1, 1, None, f64(0.0), None, None, None, 1,
                                          None, None, 1, None) == -1
    assert engine_lib.nmp_intstats_update(None, 1, 1, 1, i32(0, 0, 0, 1), None, None, None, None,
                                          1, None, None, 1, None) == -1
    assert engine_lib.nmp_intstats_output(None, 1, 1, None, 1, 900.0, None, None, 1, None, 1,
                                          None) == -1


def test_refusals_come_in_the_documented_order():
    """The entries' source: engine and strides, the items, the empty call's
    NMP_OK, NULL pointers, the device last (engine_impl.h)."""
    src = open(os.path.join(_build.CSRC, "intstats.hip")).read()
    for name in ("nmp_intstats_update", "nmp_intstats_output"):
        body = src[src.index(f"int {name}("):]
        body = body[:body.index("\n}\n")]
        marks = ["if (!eng || ncol < 0", "nitems < 1 || nitems > NMP_IST_MAXITEMS",
                 "nmp::ist_table(", "if (ncol == 0) return NMP_OK;", "if (!acc ||",
                 "nmp::ensure_device(", "nmp::launch_cols("]
        at = [body.index(m) for m in marks]
        assert at == sorted(at), name


# ---- restart variables -------------------------------------------------------------------
def test_netcdf_restart_carries_the_interval(tmp_path, ref_params):
    from noahmp_amd import cases
    from test_ncio import grid_for
    cols = cases.make_columns(32, "mixed", ref_params, seed=8)
    grid = grid_for(cols)
    items = IS.parse("T2M,FROST=SFCTMP@lt273.15:dur+spell+deg,SMC1")
    spec = IS.spec_string(items)
    rng = np.random.default_rng(3)
    acc = rng.normal(size=(3, 32))
    acc[0, 0], acc[1, 1], acc[2, 31] = -0.0, NAN, INF
    cnt = rng.integers(0, 13, size=(9, 32)).astype(np.int32)
    state = np.asarray(cols.state, np.float32)
    t = datetime.datetime(2000, 1, 1, 10)
    path = str(tmp_path / "r.nc")
    ncio.write_state(path, grid, state, cols.isnow, t, 40, intstats=(acc, cnt, 4, spec))
    got = ncio.read_intstats(path, grid)
    assert got[2:] == (4, spec)
    assert same_bits(got[0], acc) and got[1].dtype == np.int32 and np.array_equal(got[1], cnt)
    f = ncio._read(path)
    try:
        assert f.variables["IST_FROST_SUM"].data.dtype.str[1:] == "f8"
        assert f.variables["IST_FROST_LONGEST"].data.dtype.str[1:] == "i4"
        assert {"IST_T2M_SUM", "IST_SMC1_SUM", "IST_T2M_COUNT", "IST_FROST_COUNT",
                "IST_FROST_RUN"} <= set(f.variables)
    finally:
        f.close()
    # read_state ignores them; a file without them has none
    st, isn, tt, step = ncio.read_state(path, grid, np.float32)
    assert same_bits(st, state) and (tt, step) == (t, 40)
    assert ncio.read_accum(path, grid) is None and ncio.read_extremes(path, grid) is None
    ncio.write_state(path, grid, state, cols.isnow, t, 40)
    assert ncio.read_intstats(path, grid) is None
    # beside an accumulating run's and the extremes' variables
    accum = (rng.normal(size=(L.NACC, 32)), rng.normal(size=32), 4)
    xs = X.parse("TG")
    ext = (rng.normal(size=(2, 32)).astype(np.float32),
           rng.integers(1, 5, size=(2, 32)).astype(np.int32), 4, X.spec_string(xs))
    ncio.write_state(path, grid, state, cols.isnow, t, 40, accum=accum, extremes=ext,
                     intstats=(acc, cnt, 4, spec))
    assert same_bits(ncio.read_intstats(path, grid)[0], acc)
    assert same_bits(ncio.read_accum(path, grid)[0], accum[0])
    assert same_bits(ncio.read_extremes(path, grid)[0], ext[0])


# ---- the driver's refusals and the CLI ----------------------------------------------------
def test_driver_refuses_before_any_device_work(tmp_path):
    from noahmp_amd import cases, config, driver
    from noahmp_amd.params import Params
    from test_config import write_case
    cfg = config.Config(write_case(tmp_path))
    cols = cases.make_columns(8, "mixed", Params.builtin().as_dict(), seed=2, julian=0.0)
    with pytest.raises(ValueError, match="writes output"):
        driver.OfflineDriver(cfg, cols, write=False, interval_stats="T2M")
    for bad in ("NOPE", "T2M:avg", "T2M,T2M", "", "T2M@gt1", "X=T2M@gtinf"):
        with pytest.raises(ValueError, match="interval_stats"):
            driver.OfflineDriver(cfg, cols, interval_stats=bad)


def _load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_cli_parses_interval_stats(capsys):
    cli = _load(os.path.join(ROOT, "noahmp_offline.py"), "noahmp_offline")
    ap = cli.build_parser()
    assert ap.parse_args(["case.nml"]).interval_stats is None
    a = ap.parse_args(["case.nml", "--interval-stats", "T2M,FROST=T2M@lt273.15:dur+spell"])
    assert a.interval_stats == "T2M,FROST=T2M@lt273.15:dur+spell" and a.nmlfile == "case.nml"
    assert IS.row_names(IS.parse(a.interval_stats)) == ["T2M_MEAN", "FROST_DUR", "FROST_SPELL"]
    with pytest.raises(SystemExit):
        ap.parse_args(["case.nml", "--interval-stats"])
    with pytest.raises(SystemExit):                       # a bad spec ends the run in main()
        cli.main([os.path.join(ROOT, "examples", "offline_case.nml"), "--interval-stats",
                  "T2M@lt273.15"])
    capsys.readouterr()
    assert "FROST_SPELL" in ap.format_help()
