"""Interval extremes, host side (no GPU): the spec parser and the row names,
the numpy restatement (extremes.update_host / output_host) on hand-written
cases for every clause of the rule the header states, the new enums against the
header, the two C entries' declaration, export, binding and argument rules,
the restart variables of ncio, and the CLI option.

Every comparison of values is on bits."""
import datetime
import importlib.util
import os
import re
import subprocess

import numpy as np
import pytest

from noahmp_amd import build as _build, extremes as X, layout as L, lib as _lib, ncio
from test_abi_host import _enum_values, _header

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")
INF = float("inf")


def ibits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(ibits(a), ibits(b))


# ---- parse / row_names ------------------------------------------------------------------
def test_parse_accepts_every_offered_name():
    single = [n for n, w in L.STATE_FIELDS if w == 1]
    soil = [f"{f}{i}" for f in ("SMC", "SH2O", "STC") for i in range(1, 5)]
    assert len(single) == 28
    assert sorted(X.SOURCES) == sorted(L.DIAG_OUT + L.FORCING + single + soil)
    for i, n in enumerate(L.DIAG_OUT):
        assert X.parse(n) == [X.Series(n, L.EXT_SRC_DIAG, i, 3)]
    for i, n in enumerate(L.FORCING):
        assert X.parse([n]) == [X.Series(n, L.EXT_SRC_FORCING, i, 3)]
    for n in single:
        assert X.parse(n)[0][1:3] == (L.EXT_SRC_STATE, L.STATE_OFF[n][0])
    for i in range(1, 5):
        assert X.parse(f"SMC{i}")[0].row == L.si("SMC") + i - 1
        assert X.parse(f"SH2O{i}")[0].row == L.si("SH2O") + i - 1
        assert X.parse(f"STC{i}")[0].row == L.si("STC") + 2 + i
    assert X.parse("STC1")[0].row == 3 and X.parse("STC4")[0].row == 6


def test_parse_specs_and_refusals():
    s = X.parse("T2M,TRAD:max,PRCP:max+tmax")
    assert s == [X.Series("T2M", 0, L.DIAG_OUT.index("T2M"), 3),
                 X.Series("TRAD", 0, L.DIAG_OUT.index("TRAD"), 1),
                 X.Series("PRCP", 1, L.FORCING.index("PRCP"), 1 | 4)]
    assert X.parse(" T2M , TRAD : max ,PRCP:MAX+TMax ") == s
    assert X.parse(["T2M", ("TRAD", "max"), ("PRCP", ["max", "tmax"])]) == s
    assert X.parse(["T2M", "TRAD:max", ("PRCP", 5)]) == s
    assert X.parse(s) == s and X.parse(X.spec_string(s)) == s
    assert X.spec_string(s) == "T2M:max+min,TRAD:max,PRCP:max+tmax"
    assert X.parse("TG:tmin+min+tmax+max")[0].stats == 15
    assert X.row_names(s) == ["T2M_MAX", "T2M_MIN", "TRAD_MAX", "PRCP_MAX", "PRCP_TMAX"]
    assert X.row_names(X.parse("TG:tmin+min+tmax+max,SMC1:tmin")) == \
        ["TG_MAX", "TG_MIN", "TG_TMAX", "TG_TMIN", "SMC1_TMIN"]
    assert X.pairs(s).tolist() == [[0, 14], [0, 11], [1, 8]] and X.pairs(s).dtype == np.int32
    assert X.masks(s).tolist() == [3, 1, 5] and X.has_diag(s)
    assert not X.has_diag(X.parse("PRCP,TG"))
    # unknown names (snow-layer rows among them), stats, duplicates, nothing, too many
    for bad in ("NOPE", "t2m", "STC", "SMC", "SNICE", "SNLIQ1", "STC0", "STC5", "SMC5", "ZSNSO",
                "ISNOW", "T2M:avg", "T2M:", "T2M:max+", "T2M:max-min", "T2M,T2M", "T2M,TG,T2M:max",
                "", " , ", [], [("T2M", 0)], [("T2M", 16)], [("T2M", [])]):
        with pytest.raises(ValueError):
            X.parse(bad)
    names = sorted(X.SOURCES)
    assert len(X.parse(names[:32])) == 32
    with pytest.raises(ValueError, match="at most 32"):
        X.parse(names[:33])
    # no row name collides with a flux, a budget row or a state-output row
    from noahmp_amd import stateout
    every = X.row_names(X.parse([(n, 15) for n in names[:32]]) + X.parse(
        [(n, 15) for n in names[32:64]]) + X.parse([(n, 15) for n in names[64:]]))
    assert len(set(every)) == 4 * len(names)
    assert not set(every) & (set(L.DIAG_OUT_ACC) | set(stateout.row_names(stateout.ALL)))


# ---- the rule ----------------------------------------------------------------------------
def run_series(values, dtype=np.float32):
    """One DIAG series (row 3) over len(values) steps, one column per list in
    `values` (columns x steps): (val, when) after every step."""
    v = np.array(values, dtype).T                      # (steps, columns)
    n = v.shape[1]
    val, when = np.full((2, n), 77, dtype), np.full((2, n), -5, np.int32)
    out = []
    for k in range(1, v.shape[0] + 1):
        diag = np.full((16, n), 123, dtype)
        diag[3] = v[k - 1]
        X.update_host(val, when, k, [(L.EXT_SRC_DIAG, 3)], diag=diag)
        out.append((val.copy(), when.copy()))
    return out


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_update_host_every_clause(dtype):
    cols = [
        [1, 5, 3, 5, 2, 0],          # 0: equal maxima at steps 2 and 4: the first wins
        [4, 1, 7, 1, 9, 1],          # 1: equal minima at 2, 4, 6
        [NAN, 2, 1, 3, NAN, 2],      # 2: NaN first, then numbers
        [2, 3, NAN, NAN, 1, NAN],    # 3: numbers, then NaN
        [NAN] * 6,                   # 4: all NaN
        [0.0, -0.0, 0.0, -0.0, 0.0, -0.0],   # 5: +0 then -0
        [-0.0, 0.0, -0.0, 0.0, -0.0, 0.0],   # 6: -0 then +0
        [1, INF, 2, INF, -INF, -INF],        # 7: infinities
        [1, 2, 3, 4, 5, 6],          # 8: strictly rising
        [6, 5, 4, 3, 2, 1],          # 9: strictly falling
        [NAN, NAN, -INF, 1, 1, 1],   # 10: NaN replaced by -inf, which then stays the min
    ]
    steps = run_series(cols, dtype)
    val, when = steps[-1]
    mx, mn, wmx, wmn = val[0], val[1], when[0], when[1]
    assert val.dtype == dtype and when.dtype == np.int32
    assert (mx[0], wmx[0], mn[0], wmn[0]) == (5, 2, 0, 6)
    assert (mx[1], wmx[1], mn[1], wmn[1]) == (9, 5, 1, 2)
    assert (mx[2], wmx[2], mn[2], wmn[2]) == (3, 4, 1, 3)
    assert (mx[3], wmx[3], mn[3], wmn[3]) == (3, 2, 1, 5)
    assert np.isnan(mx[4]) and np.isnan(mn[4]) and wmx[4] == wmn[4] == 1
    pz, nz = ibits(np.array([0.0], dtype))[0], ibits(np.array([-0.0], dtype))[0]
    assert ibits(mx)[5] == pz and ibits(mn)[5] == pz and wmx[5] == wmn[5] == 1
    assert ibits(mx)[6] == nz and ibits(mn)[6] == nz and wmx[6] == wmn[6] == 1
    assert (mx[7], wmx[7], mn[7], wmn[7]) == (INF, 2, -INF, 5)
    assert (mx[8], wmx[8], mn[8], wmn[8]) == (6, 6, 1, 1)
    assert (mx[9], wmx[9], mn[9], wmn[9]) == (6, 1, 1, 6)
    assert (mx[10], wmx[10], mn[10], wmn[10]) == (1, 4, -INF, 3)
    # after the first step: everything is the value, NaN included, when = 1
    v1, w1 = steps[0]
    first = np.array([c[0] for c in cols], dtype)
    assert same_bits(v1[0], first) and same_bits(v1[1], first) and (w1 == 1).all()
    # while NaN holds, when stays 1; the first number takes it with its own step
    assert np.isnan(steps[1][0][0, 10]) and steps[1][1][0, 10] == 1
    assert steps[2][0][0, 10] == -INF and steps[2][1][:, 10].tolist() == [3, 3]
    # k = 1 again starts a new interval whatever is stored
    X.update_host(val, when, 1, [(0, 3)], diag=np.full((16, len(cols)), 8, dtype))
    assert (val == 8).all() and (when == 1).all()


def test_update_host_payloads_blocks_and_refusals():
    # a NaN's payload and sign travel as stored
    odd = np.array([0x7fc01234, 0xffc00001, 0x7f800001], np.uint32).view(np.float32)
    val, when = np.zeros((2, 3), np.float32), np.zeros((2, 3), np.int32)
    st = np.zeros((56, 3), np.float32)
    st[29] = odd
    X.update_host(val, when, 1, [(L.EXT_SRC_STATE, 29)], state=st)
    assert same_bits(val[0], odd) and same_bits(val[1], odd)
    st[29] = odd[::-1]
    X.update_host(val, when, 2, [(L.EXT_SRC_STATE, 29)], state=st)
    assert same_bits(val[0], odd) and (when == 1).all()
    # three kinds at once; rows 2s, 2s + 1 belong to series s
    rng = np.random.default_rng(0)
    d, f, s = (rng.normal(size=(r, 5)) for r in (16, 12, 56))
    val, when = np.zeros((6, 5)), np.zeros((6, 5), np.int32)
    kr = [(L.EXT_SRC_STATE, 55), (L.EXT_SRC_DIAG, 0), (L.EXT_SRC_FORCING, 11)]
    X.update_host(val, when, 1, kr, d, f, s)
    assert same_bits(val, np.stack([s[55], s[55], d[0], d[0], f[11], f[11]]))
    d2, f2, s2 = d + 1, f - 1, s.copy()
    X.update_host(val, when, 2, kr, d2, f2, s2)
    assert same_bits(val, np.stack([s[55], s[55], d2[0], d[0], f[11], f2[11]]))
    assert when.tolist() == [[1] * 5, [1] * 5, [2] * 5, [1] * 5, [1] * 5, [2] * 5]
    for kw in (dict(k=0), dict(k=-1), dict(kr=[(3, 0)]), dict(kr=[(-1, 0)]), dict(kr=[(0, 16)]),
               dict(kr=[(1, 12)]), dict(kr=[(2, 56)]), dict(kr=[(0, -1)]), dict(kr=[]),
               dict(kr=[(2, 0)] * 33)):
        a = dict(k=1, kr=[(0, 0)])
        a.update(kw)
        n = max(len(a["kr"]), 1)
        with pytest.raises(ValueError):
            X.update_host(np.zeros((2 * n, 5)), np.zeros((2 * n, 5), np.int32), a["k"], a["kr"],
                          d, f, s)
    with pytest.raises(ValueError, match="missing"):
        X.update_host(np.zeros((2, 5)), np.zeros((2, 5), np.int32), 1, [(1, 0)], diag=d, state=s)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_output_host_rows_and_times(dtype):
    rng = np.random.default_rng(1)
    val = rng.normal(size=(6, 7)).astype(dtype)
    val[0, 0], val[3, 1] = NAN, -0.0
    when = rng.integers(1, 97, size=(6, 7)).astype(np.int32)
    when[4, 0], when[5, 1] = 2 ** 31 - 1, 1
    out = X.output_host(val, when, [1 | 4, 2 | 8 | 4, 15], 900.0)
    assert out.dtype == dtype and out.shape == (2 + 3 + 4, 7)
    t = lambda r, dt=900.0: np.array([dtype(float(w) * dt) for w in when[r]], dtype)  # noqa: E731
    want = [val[0], t(0), val[3], t(2), t(3), val[4], val[5], t(4), t(5)]
    for got, w in zip(out, want):
        assert same_bits(got, w)
    # one rounded double product, then one conversion (0.1 is not exact)
    out = X.output_host(val[:2], when[:2], [8], 0.1)
    assert same_bits(out[0], np.array([dtype(float(w) * 0.1) for w in when[1]], dtype))
    assert same_bits(X.output_host(val, when, [4, 4, 4], 900.0)[2], t(4))
    v0, w0 = val.copy(), when.copy()
    X.output_host(val, when, [3, 3, 3], 1800.0)
    assert same_bits(val, v0) and np.array_equal(when, w0)
    for stats, dt in (([0, 1, 1], 900.0), ([16, 1, 1], 900.0), ([1, 1, 17], 900.0),
                      ([-1, 1, 1], 900.0), ([1, 1, 1], 0.0), ([1, 1, 1], -900.0),
                      ([1, 1, 1], NAN), ([1, 1, 1], INF)):
        with pytest.raises(ValueError):
            X.output_host(val, when, stats, dt)


# ---- header, enums, ABI -------------------------------------------------------------------
def test_layout_mirrors_the_header_enums():
    text = _header()
    e = _enum_values(text)
    assert (e["NMP_EXT_SRC_DIAG"], e["NMP_EXT_SRC_FORCING"], e["NMP_EXT_SRC_STATE"]) == \
        (L.EXT_SRC_DIAG, L.EXT_SRC_FORCING, L.EXT_SRC_STATE) == (0, 1, 2)
    assert (e["NMP_EXT_MAX"], e["NMP_EXT_MIN"], e["NMP_EXT_TMAX"], e["NMP_EXT_TMIN"]) == \
        (L.EXT_MAX, L.EXT_MIN, L.EXT_TMAX, L.EXT_TMIN) == (1, 2, 4, 8)
    assert L.EXT_STATS == {"MAX": 1, "MIN": 2, "TMAX": 4, "TMIN": 8}
    assert [b for _, b in X.STAT_ORDER] == [1, 2, 4, 8]
    assert int(re.search(r"#define NMP_EXT_MAXSERIES (\d+)", text).group(1)) == \
        L.EXT_MAXSERIES == 32
    # the error codes' prefix is not reused
    assert not [n for n in e if n.startswith("NMP_E_") and "EXT" in n]
    i = text.index("Interval extremes (no counterpart")
    words = re.sub(r"\s*\n \*\s*", " ", text[i:text.index("int nmp_extremes_update", i)])
    for w in ("(v > max) || (max != max && v == v)", "(v < min) || (min != min && v == v)",
              "max = min = v, both when = 1", "(T)((double)when * dt)",
              "the first occurrence wins a tie", "no arithmetic, no rounding",
              "It changes neither val nor when", "neither synchronise nor allocate",
              "ncol == 0 with otherwise valid arguments is NMP_OK"):
        assert w in words, w


def test_entries_declared_exported_and_bound(engine_lib):
    decl = set(re.findall(r"^\s*(?:int|int64_t|void\*?|const char\*)\s*(nmp_\w+)\s*\(", _header(),
                          re.M))
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.library_path()], capture_output=True,
                        text=True, check=True).stdout
    exported = set(re.findall(r"\bT (nmp_\w+)$", nm, re.M))
    for name in ("nmp_extremes_update", "nmp_extremes_output"):
        assert name in decl, f"{name} not declared in the header"
        assert name in _lib.EXPORTED_SYMBOLS and name in exported
        assert getattr(engine_lib, name).argtypes is not None, f"{name} not bound in lib.py"
    assert "extremes.hip" in _build.SOURCES
    assert os.path.exists(os.path.join(_build.CSRC, "extremes.hip"))
    assert re.search(r"#define NMP_ABI_VERSION 8\b", _header())
    assert engine_lib.nmp_abi_version() == 8   # additive: the version stays
    # no new -DNMP_* switch
    src = open(os.path.join(_build.CSRC, "extremes.hip")).read()
    assert not re.search(r"#\s*if(n?def)?\b", src)


def test_entries_refuse_bad_arguments_without_an_engine(engine_lib):
    """Every refused case, with NULL handles (no device is touched)."""
    import ctypes as C
    i32 = lambda *v: (C.c_int32 * len(v))(*v)  # noqa: E731

    def upd(ncol=1, ld=1, ns=1, series=(0, 0), k=1, ld_ext=1):
        return engine_lib.nmp_extremes_update(None, ncol, ld, ns, i32(*series), None, None, None,
                                              k, None, None, ld_ext, None)

    def out(ncol=1, ns=1, stats=(1,), dt=900.0, ld_ext=1, ld_out=1):
        return engine_lib.nmp_extremes_output(None, ncol, ns, i32(*stats), dt, None, None,
                                              ld_ext, None, ld_out, None)
    big = 1 << 29
    assert upd() == -1 and out() == -1
    assert upd(ncol=0, ld=0, ld_ext=0) == -1 and out(ncol=0, ld_ext=0, ld_out=0) == -1  # no engine
    assert upd(ncol=-1) == -1 and out(ncol=-1) == -1
    assert upd(ncol=2) == -1 and upd(ncol=2, ld=2) == -1 and upd(ncol=2, ld_ext=2) == -1
    assert out(ncol=2) == -1 and out(ncol=2, ld_ext=2) == -1 and out(ncol=2, ld_out=2) == -1
    assert upd(ld=big) == -1 and upd(ld_ext=big) == -1
    assert out(ld_ext=big) == -1 and out(ld_out=big) == -1
    for ns in (0, -1, 33):
        assert upd(ns=ns, series=(0, 0) * 33) == -1 and out(ns=ns, stats=(1,) * 33) == -1
    for series in ((3, 0), (-1, 0), (0, 16), (1, 12), (2, 56), (0, -1)):
        assert upd(series=series) == -1
    for k in (0, -1):
        assert upd(k=k) == -1
    for stats in ((0,), (16,), (17,), (-1,)):
        assert out(stats=stats) == -1
    for dt in (0.0, -900.0, NAN, INF, -INF):
        assert out(dt=dt) == -1
    assert engine_lib.nmp_extremes_update(None, 1, 1, 1, None, None, None, None, 1, None, None, 1,
                                          None) == -1
    assert engine_lib.nmp_extremes_output(None, 1, 1, None, 900.0, None, None, 1, None, 1,
                                          None) == -1


# ---- restart variables -------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_netcdf_restart_carries_the_interval(tmp_path, ref_params, dtype):
    from noahmp_amd import cases
    from test_ncio import grid_for
    cols = cases.make_columns(32, "mixed", ref_params, seed=8)
    grid = grid_for(cols)
    series = X.parse("T2M,PRCP:max+tmax,STC1:tmin")
    spec = X.spec_string(series)
    rng = np.random.default_rng(3)
    val = rng.normal(size=(6, 32)).astype(dtype)
    val[0, 0], val[5, 31] = -0.0, INF
    when = rng.integers(1, 13, size=(6, 32)).astype(np.int32)
    state = np.asarray(cols.state, dtype)
    t = datetime.datetime(2000, 1, 1, 10)
    path = str(tmp_path / "r.nc")
    ncio.write_state(path, grid, state, cols.isnow, t, 40, extremes=(val, when, 4, spec))
    got = ncio.read_extremes(path, grid)
    assert got[2:] == (4, spec)
    assert same_bits(got[0], val) and got[1].dtype == np.int32 and np.array_equal(got[1], when)
    # read_state ignores them; a file without them has none
    st, isn, tt, step = ncio.read_state(path, grid, dtype)
    assert same_bits(st, state) and (tt, step) == (t, 40)
    assert ncio.read_accum(path, grid) is None
    ncio.write_state(path, grid, state, cols.isnow, t, 40)
    assert ncio.read_extremes(path, grid) is None
    # beside an accumulating run's variables
    acc = (rng.normal(size=(L.NACC, 32)), rng.normal(size=32), 4)
    ncio.write_state(path, grid, state, cols.isnow, t, 40, accum=acc,
                     extremes=(val, when, 4, spec))
    assert same_bits(ncio.read_extremes(path, grid)[0], val)
    assert same_bits(ncio.read_accum(path, grid)[0], acc[0])


# ---- the driver's refusals and the CLI ----------------------------------------------------
def test_driver_refuses_before_any_device_work(tmp_path):
    from noahmp_amd import cases, config, driver
    from noahmp_amd.params import Params
    from test_config import write_case
    cfg = config.Config(write_case(tmp_path))
    cols = cases.make_columns(8, "mixed", Params.builtin().as_dict(), seed=2, julian=0.0)
    with pytest.raises(ValueError, match="writes output"):
        driver.OfflineDriver(cfg, cols, write=False, extremes="T2M")
    for bad in ("NOPE", "T2M:avg", "T2M,T2M", ""):
        with pytest.raises(ValueError, match="extremes"):
            driver.OfflineDriver(cfg, cols, extremes=bad)


def _load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_cli_parses_extremes(capsys):
    cli = _load(os.path.join(ROOT, "noahmp_offline.py"), "noahmp_offline")
    ap = cli.build_parser()
    assert ap.parse_args(["case.nml"]).extremes is None
    a = ap.parse_args(["case.nml", "--extremes", "T2M,TRAD:max,PRCP:max+tmax"])
    assert a.extremes == "T2M,TRAD:max,PRCP:max+tmax" and a.nmlfile == "case.nml"
    assert X.row_names(X.parse(a.extremes)) == ["T2M_MAX", "T2M_MIN", "TRAD_MAX", "PRCP_MAX",
                                                "PRCP_TMAX"]
    with pytest.raises(SystemExit):
        ap.parse_args(["case.nml", "--extremes"])
    with pytest.raises(SystemExit):                       # a bad spec ends the run in main()
        cli.main([os.path.join(ROOT, "examples", "offline_case.nml"), "--extremes", "T2M:avg"])
    capsys.readouterr()
    assert "_TMAX" in ap.format_help()
