"""Vegetation fraction through the year, host side (no GPU): the numpy twin
(vegclim.shdfac_host) against ncio._month_weighted -- what read_static forms
at a run's first instant -- and against the operation order restated here from
include/noahmp_engine.h alone, the date arithmetic (month_weights, quantise),
the C entry's declaration, export, binding and argument rules, the CLI option,
the case writer's seasonal table and ncio.read_greenfrac.

Every comparison is on bits."""
import datetime
import importlib.util
import os
import re
import subprocess

import numpy as np
import pytest

from noahmp_amd import build as _build, cases, layout as L, lib as _lib, ncio, timeman, vegclim
from noahmp_amd.params import Params
from test_abi_host import _header

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 97
# 16 January 06:00 of a leap year: 12 * 15.25 / 366 = 0.5 exactly, so t = 0 and w == 0.0
W0_INSTANT = datetime.datetime(2004, 1, 16, 6)


def ibits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def same(a, b):
    """Bit for bit, a NaN equal to any NaN of the same place."""
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and bool(
        ((ibits(a) == ibits(b)) | (np.isnan(a) & np.isnan(b))).all())


def table(n=N, seed=0, special=False):
    """(12, n) float32 months in [0, 1]; special: a handful of NaN, -0.0, a
    subnormal and 1.0 among them."""
    rng = np.random.default_rng(seed)
    g = rng.random((12, n)).astype(np.float32)
    if special:
        g[0, 3], g[5, 4], g[11, 5] = np.nan, np.nan, np.nan
        g[1, 6], g[6, 6], g[7, 6] = -0.0, -0.0, -0.0
        g[2, 7], g[8, 8] = np.float32(1e-42), np.float32(1e-42)
        g[3, 9], g[4, 9], g[9, 10] = 1.0, 1.0, 1.0
    return g


def instants():
    """Every day's 00:00 and 13:30 of 2003 (365 days) and 2004 (366), the wrap
    of 1 to 16 January and the w == 0 instant."""
    out = []
    for year in (2003, 2004):
        d = datetime.datetime(year, 1, 1)
        while d.year == year:
            out += [d, d + datetime.timedelta(hours=13, minutes=30)]
            d += datetime.timedelta(days=1)
    for year in (2003, 2004):
        for day in range(1, 17):
            out += [datetime.datetime(year, 1, day, h) for h in (0, 5, 6, 23)]
    return out + [W0_INSTANT]


# ---- the twin ---------------------------------------------------------------------------
def test_shdfac_host_equals_read_statics_interpolation():
    g = table(special=True)
    ts = instants()
    assert len(ts) == 2 * 731 + 2 * 16 * 4 + 1
    for when in ts:
        want = ncio._month_weighted(g, when)
        got = vegclim.shdfac_host(g, when)
        assert got.dtype == np.float32 and np.array_equal(ibits(got), ibits(want)), when
        # an fp64 engine sees the fp32 value widened
        assert np.array_equal(ibits(vegclim.shdfac_host(g, when, np.float64)),
                              ibits(want.astype(np.float64))), when


def test_month_weights():
    for when in instants():
        m0, m1, w = vegclim.month_weights(when)
        t = 12.0 * timeman.julian(when) / timeman.yearlen(when.year) - 0.5
        assert (m0, m1) == (int(np.floor(t)) % 12, (int(np.floor(t)) + 1) % 12)
        assert w == t - np.floor(t) and 0.0 <= w < 1.0 and isinstance(w, float)
    # early January lies between December and January
    for year, last in ((2003, datetime.datetime(2003, 1, 16, 4)),
                       (2004, datetime.datetime(2004, 1, 16, 5))):
        d = datetime.datetime(year, 1, 1)
        while d <= last:
            assert vegclim.month_weights(d)[:2] == (11, 0), d
            d += datetime.timedelta(hours=1)
        assert vegclim.month_weights(last + datetime.timedelta(hours=2))[:2] == (0, 1)
    # mid-month of an equal-month year: t is an integer, the month's own row
    assert vegclim.month_weights(W0_INSTANT) == (0, 1, 0.0)
    g = table()
    assert np.array_equal(ibits(vegclim.shdfac_host(g, W0_INSTANT)), ibits(g[0]))
    assert np.array_equal(ibits(ncio._month_weighted(g, W0_INSTANT)), ibits(g[0]))
    assert vegclim.month_weights(datetime.datetime(2004, 7, 1, 0))[:2] == (5, 6)


def test_twelve_equal_rows_return_the_row():
    row = table(special=False)[0]
    row[:4] = (0.0, 1.0, np.float32(1e-42), np.float32(0.7))
    g = np.repeat(row[None, :], 12, 0)
    for when in instants():
        assert np.array_equal(ibits(vegclim.shdfac_host(g, when)), ibits(row)), when


def restated(g, m0, m1, w, dtype):
    """nmp_static_monthly as the header words it, column by column in Python
    floats (IEEE double), fp32 through numpy scalars."""
    out = np.empty(g.shape[1], dtype)
    u = 1.0 - w
    with np.errstate(all="ignore"):
        for c in range(g.shape[1]):
            a, b = float(g[m0, c]), float(g[m1, c])
            p, q = u * a, w * b
            out[c] = dtype(np.float32(p + q))
    return out


def test_static_monthly_host_is_the_documented_operation_order():
    h = _header()
    i = h.index("Vegetation fraction through the year")
    text = h[i:h.index("int nmp_static_monthly", i)]
    for words in ("a = (double)table12[m0*ld_tab + c]", "b = (double)table12[m1*ld_tab + c]",
                  "u = 1.0 - w", "r = (float)(u*a + w*b)", "out_row[c] = (T)r",
                  "two rounded products, then one add", "no fused multiply-add"):
        assert words in text, words
    g = table(special=True)
    for m0, m1, w in ((11, 0, 0.0), (0, 1, 2.0 ** -30), (5, 6, 1 / 3), (6, 6, 0.5),
                      (3, 4, 1 - 2.0 ** -53), (7, 2, 0.9)):
        for dtype in (np.float32, np.float64):
            got = vegclim.static_monthly_host(g, m0, m1, w, dtype)
            assert got.dtype == dtype and same(got, restated(g, m0, m1, w, dtype)), (m0, m1, w)
    # no special case at w == 0: -0.0 and NaN go through the formula
    got = vegclim.static_monthly_host(g, 1, 0, 0.0)
    assert ibits(got)[6] == 0 and np.isnan(got[3])          # -0*1 + 0*b = +0; 0 * NaN = NaN
    for kw in (dict(m0=-1), dict(m0=12), dict(m1=-1), dict(m1=12), dict(w=1.0), dict(w=-0.25),
               dict(w=float("nan")), dict(w=float("inf"))):
        args = dict(m0=0, m1=1, w=0.5)
        args.update(kw)
        with pytest.raises(ValueError):
            vegclim.static_monthly_host(g, **args)


def test_quantise():
    t = datetime.datetime(2004, 2, 29, 13, 30, 15)
    assert vegclim.quantise(t, "step") == t
    assert vegclim.quantise(t, "daily") == datetime.datetime(2004, 2, 29)
    midnight = datetime.datetime(2003, 12, 31)
    assert vegclim.quantise(midnight, "daily") == midnight == vegclim.quantise(midnight, "step")
    last = datetime.datetime(2003, 12, 31, 23, 59, 59)
    assert vegclim.quantise(last, "daily") == midnight
    assert vegclim.quantise(last + datetime.timedelta(seconds=1), "daily") == \
        datetime.datetime(2004, 1, 1)
    for bad in ("monthly", "", "Daily", True):
        with pytest.raises(ValueError):
            vegclim.quantise(t, bad)
    assert vegclim.CADENCES == ("daily", "step")
    g = table()
    assert vegclim.check_table(g, N) is not None and vegclim.check_table(g.astype(np.float64), N) \
        .dtype == np.float32
    for bad in (g[:11], g[:, :-1], g[0], g[None]):
        with pytest.raises(ValueError):
            vegclim.check_table(bad, N)


# ---- ABI --------------------------------------------------------------------------------
def test_static_monthly_exported(engine_lib):
    decl = set(re.findall(r"^\s*(?:int|int64_t|void\*?|const char\*)\s*(nmp_\w+)\s*\(", _header(),
                          re.M))
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.library_path()], capture_output=True,
                        text=True, check=True).stdout
    exported = set(re.findall(r"\bT (nmp_\w+)$", nm, re.M))
    name = "nmp_static_monthly"
    assert name in decl, f"{name} not declared in the header"
    assert name in _lib.EXPORTED_SYMBOLS and name in exported
    assert getattr(engine_lib, name).argtypes is not None, f"{name} not bound in lib.py"
    assert "vegclim.hip" in _build.SOURCES
    assert os.path.exists(os.path.join(_build.CSRC, "vegclim.hip"))
    assert re.search(r"#define NMP_ABI_VERSION 8\b", _header())
    assert engine_lib.nmp_abi_version() == 8   # additive: the version stays


def test_static_monthly_refuses_bad_arguments_without_an_engine(engine_lib):
    """Every refused case, with NULL handles (no device is touched)."""
    def call(ncol=1, ld=1, m0=0, m1=1, w=0.5):
        return engine_lib.nmp_static_monthly(None, ncol, ld, None, m0, m1, w, None, None)
    assert call() == -1
    assert call(ncol=0, ld=0) == -1                               # no engine
    assert call(ncol=-1) == -1 and call(ld=0) == -1
    assert call(ncol=(1 << 29) + 1, ld=(1 << 29) + 1) == -1
    for m in (-1, 12):
        assert call(m0=m) == -1 and call(m1=m) == -1
    for w in (1.0, -0.25, 1.5, float("nan"), float("inf")):
        assert call(w=w) == -1


# ---- the CLI, the case writer and the reader ------------------------------------------------
def _load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_cli_parses_veg_clim(capsys):
    cli = _load(os.path.join(ROOT, "noahmp_offline.py"), "noahmp_offline")
    ap = cli.build_parser()
    assert ap.parse_args(["case.nml"]).veg_clim is None
    assert ap.parse_args(["case.nml", "--veg-clim"]).veg_clim == "daily"
    assert ap.parse_args(["case.nml", "--veg-clim", "daily"]).veg_clim == "daily"
    assert ap.parse_args(["case.nml", "--veg-clim", "step"]).veg_clim == "step"
    assert ap.parse_args(["--veg-clim", "step", "case.nml"]).nmlfile == "case.nml"
    with pytest.raises(SystemExit):
        ap.parse_args(["case.nml", "--veg-clim", "monthly"])
    capsys.readouterr()
    assert "opt_veg = 1" in re.sub(r"\s+", " ", ap.format_help())


def _case(n=40, seed=2):
    P = Params.builtin().as_dict()
    cols = cases.make_columns(n, "mixed", P, seed=seed, julian=0.0)
    rng = np.random.default_rng(seed)
    mask = np.zeros(6 * 9, bool)
    mask[rng.permutation(mask.size)[:n]] = True
    lat = 30.0 + 0.25 * np.arange(6)[:, None] + 0.0 * np.arange(9)[None, :]
    lon = -120.0 + 0.25 * np.arange(9)[None, :] + 0.0 * np.arange(6)[:, None]
    return P, cols, ncio.Grid(lat, lon, mask.reshape(6, 9))


def test_driver_refuses_before_any_device_work(tmp_path):
    """veg_clim without a table, with one of the wrong shape, or an unknown
    cadence: ValueError, here on a machine that has no device to work on."""
    from noahmp_amd import config, driver
    text = open(os.path.join(ROOT, "examples", "offline_case.nml")).read()
    for k in ("geo_em.d01.nc", "init.nc", "ldasin", "ldasout", "restart"):
        text = text.replace(f"'{k}'", f"'{tmp_path / k}'").replace(f'"{k}"', f'"{tmp_path / k}"')
    (tmp_path / "case.nml").write_text(text)
    cfg = config.Config(str(tmp_path / "case.nml"))
    P, cols, _ = _case(8)
    g = table(8)
    for kw in (dict(veg_clim="daily"), dict(veg_clim="step", greenfrac=None),
               dict(veg_clim="daily", greenfrac=g[:11]), dict(veg_clim="daily", greenfrac=g[:, :7]),
               dict(veg_clim="daily", greenfrac=g[0]), dict(veg_clim="monthly", greenfrac=g)):
        with pytest.raises(ValueError, match="veg_clim|greenfrac"):
            driver.OfflineDriver(cfg, cols, write=False, **kw)


def test_read_greenfrac_round_trip(tmp_path):
    P, cols, grid = _case()
    g = table(grid.n, seed=4)
    path = str(tmp_path / "static.nc")
    ncio.write_static(path, cols, grid, greenfrac=g)
    got = ncio.read_greenfrac(path, grid)
    assert got.dtype == np.float32 and got.flags.c_contiguous
    assert np.array_equal(ibits(got), ibits(g))
    # the row read_static forms at `when` is the twin's from this table
    for when in (datetime.datetime(2000, 1, 1), datetime.datetime(2000, 7, 4, 13, 30)):
        _, sf, _ = ncio.read_static(path, P, when)
        assert np.array_equal(ibits(sf[L.STATIC_F.index("SHDFAC")]),
                              ibits(vegclim.shdfac_host(got, when)))
    # without a table the file holds the columns' SHDFAC every month
    ncio.write_static(path, cols, grid)
    got = ncio.read_greenfrac(path, grid)
    shd = np.asarray(cols.static_f[L.STATIC_F.index("SHDFAC")], np.float32)
    assert np.array_equal(ibits(got), ibits(np.repeat(shd[None, :], 12, 0)))
    # a file without the variable
    from scipy.io import netcdf_file
    bare = str(tmp_path / "bare.nc")
    f = netcdf_file(bare, "w")
    f.createDimension("south_north", 6)
    f.createDimension("west_east", 9)
    for name, a in (("XLAT_M", grid.lat_deg), ("XLONG_M", grid.lon_deg)):
        v = f.createVariable(name, "f8", ("south_north", "west_east"))
        v[:] = a
    f.close()
    assert ncio.read_greenfrac(bare, grid) is None


def test_seasonal_greenfrac_of_the_case_writer():
    tool = _load(os.path.join(ROOT, "tools", "make_offline_case.py"), "make_offline_case")
    P, cols, _ = _case()
    lat = np.asarray(cols.static_f[L.STATIC_F.index("LAT")]).copy()
    lat[::2] = -np.abs(lat[::2]) - np.float32(0.1)               # half the columns south
    cols.static_f[L.STATIC_F.index("LAT")] = lat
    g = tool._seasonal_greenfrac(cols)
    assert g.shape == (12, cols.isnow.shape[0]) and g.dtype == np.float32
    assert (g >= 0).all() and (g <= 1).all()
    shd = np.asarray(cols.static_f[L.STATIC_F.index("SHDFAC")])
    veg = shd > 0
    assert veg.any()
    north = veg & (lat >= 0)
    south = veg & (lat < 0)
    assert north.any() and south.any()
    assert (g[:, north].argmax(0) == 6).all() and (g[:, south].argmax(0) == 0).all()
    assert (g[:, north].argmin(0) == 0).all() and (g[:, south].argmin(0) == 6).all()
    assert np.allclose(g.max(0), shd, rtol=1e-6)
    assert np.allclose(g.min(0)[veg], 0.2 * shd[veg], rtol=1e-5)
