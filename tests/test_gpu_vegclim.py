"""Vegetation fraction through the year on the GPU: nmp_static_monthly against
its numpy twin (vegclim.static_monthly_host / shdfac_host, themselves held to
ncio._month_weighted and to a restatement of the header in
tests/test_vegclim_host.py) bit for bit, its argument rules, and the offline
driver's veg_clim: every step against the reference itself stepped with the
row set on the host, a constant climatology against the run without the
option, one stream range against two, restarts of both file kinds, a jump back
in time, spin-up, and a run from files in the coherent order.

Every comparison is on bits."""
import ctypes as C
import datetime
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

from golden_io import bit_equal
from noahmp_amd import cases, config, driver, layout as L, ncio, timeman, vegclim
from noahmp_amd.engine import Engine
from noahmp_amd.params import Params
from test_vegclim_host import W0_INSTANT, ibits, same, table

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NCOL, LD_TAB, LD = 200, 256, 232       # three full waves plus 8 lanes; neither stride divides the other
SENTINEL = -31337.0
SHD = L.STATIC_F.index("SHDFAC")
START = datetime.datetime(2000, 1, 1, 20)
HOUR = datetime.timedelta(hours=1)


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda:0")


def _engine(precision):
    return Engine(Params.builtin(), L.CASE_NML_OPTIONS, device=0, precision=precision)


def _np(precision):
    return np.float32 if precision == 4 else np.float64


def _midnights():
    out = []
    for year in (2003, 2004):
        d = datetime.datetime(year, 1, 1)
        while d.year == year:
            out.append(d)
            d += datetime.timedelta(days=1)
    return out + [W0_INSTANT]


def _raw(eng, ncol, ld_tab, tab, m0, m1, w, out, tab_off=0, out_off=0):
    """nmp_static_monthly through the C ABI; offsets in elements."""
    s = C.c_void_p(torch.cuda.current_stream(0).cuda_stream)
    pt = None if tab is None else C.c_void_p(tab.data_ptr() + 4 * tab_off)
    po = None if out is None else C.c_void_p(out.data_ptr() + out.element_size() * out_off)
    return eng._lib.nmp_static_monthly(eng._h, ncol, ld_tab, pt, m0, m1, w, po, s)


# ---- 1. the kernel ------------------------------------------------------------------------
@pytest.mark.parametrize("precision", [4, 8])
def test_kernel_equals_the_twin(engine_lib, precision):
    eng = _engine(precision)
    dtype = _np(precision)
    g = table(NCOL, seed=precision, special=True)
    pad = np.full((12, LD_TAB), np.nan, np.float32)      # the table's padding is never stored
    pad[:, :NCOL] = g
    tab = _dev(pad)
    sf = torch.full((L.NSTATIC_F, LD), SENTINEL, device="cuda:0",
                    dtype=torch.float32 if precision == 4 else torch.float64)
    ts = _midnights()
    assert len(ts) == 732
    for when in ts:
        m0, m1, w = vegclim.month_weights(when)
        assert _raw(eng, NCOL, LD_TAB, tab, m0, m1, w, sf, out_off=SHD * LD) == 0
        got = sf.cpu().numpy()
        want = vegclim.shdfac_host(g, when, dtype)
        assert same(got[SHD, :NCOL], want), when
        # the other five rows and the padding columns keep the sentinel
        assert (np.delete(got, SHD, 0) == SENTINEL).all() and (got[SHD, NCOL:] == SENTINEL).all()
    # the w == 0 instant: month row 0, widened (special values through the formula)
    clean = np.isfinite(g[0]) & np.isfinite(g[1]) & (ibits(g[0]) != 0x80000000)
    assert clean.sum() > NCOL - 8
    assert np.array_equal(ibits(got[SHD, :NCOL][clean]), ibits(g[0].astype(dtype)[clean]))
    assert np.isnan(got[SHD, 3])
    # -0.0 in both months stays -0.0; a subnormal survives the fp32 rounding
    m0, m1, w = 6, 7, 0.25
    assert _raw(eng, NCOL, LD_TAB, tab, m0, m1, w, sf, out_off=SHD * LD) == 0
    got = sf.cpu().numpy()[SHD, :NCOL]
    assert same(got, vegclim.static_monthly_host(g, m0, m1, w, dtype))
    assert np.signbit(got[6]) and got[6] == 0
    # the binding: cols=(lo, hi) writes only those columns
    tn = _dev(g)
    row_block = torch.full((L.NSTATIC_F, NCOL), SENTINEL, dtype=sf.dtype, device="cuda:0")
    eng.static_monthly(tn, 11, 0, 0.75, row_block[SHD], cols=(37, 165))
    torch.cuda.synchronize()
    got = row_block.cpu().numpy()
    want = vegclim.static_monthly_host(g, 11, 0, 0.75, dtype)
    assert same(got[SHD, 37:165], want[37:165])
    assert (got[SHD, :37] == SENTINEL).all() and (got[SHD, 165:] == SENTINEL).all()
    assert (np.delete(got, SHD, 0) == SENTINEL).all()
    # two ranges on their own streams give the whole row
    streams = [torch.cuda.Stream(0), torch.cuda.Stream(0)]
    for st, rng in zip(streams, ((0, 93), (93, NCOL))):
        st.wait_stream(torch.cuda.current_stream(0))
        eng.static_monthly(tn, 11, 0, 0.75, row_block[SHD], stream=st, cols=rng)
        torch.cuda.current_stream(0).wait_stream(st)
    torch.cuda.synchronize()
    assert same(row_block.cpu().numpy()[SHD], want)
    for bad_tab, bad_row in ((tn[:11], row_block[SHD]), (tn.cpu(), row_block[SHD]),
                             (tn.double(), row_block[SHD]), (tn, row_block[SHD, :-1]),
                             (tn, row_block[SHD].to(torch.float16)), (tn, row_block[SHD].cpu())):
        with pytest.raises(AssertionError):
            eng.static_monthly(bad_tab, 0, 1, 0.5, bad_row)
    eng.close()


@pytest.mark.parametrize("precision", [4, 8])
def test_argument_errors(engine_lib, precision):
    eng = _engine(precision)
    tab = _dev(table(LD_TAB, seed=1))
    row = torch.full((LD,), SENTINEL, device="cuda:0",
                     dtype=torch.float32 if precision == 4 else torch.float64)
    ok = dict(ncol=NCOL, ld_tab=LD_TAB, tab=tab, m0=3, m1=4, w=0.5, out=row)

    def call(**kw):
        a = dict(ok, **kw)
        return _raw(eng, a["ncol"], a["ld_tab"], a["tab"], a["m0"], a["m1"], a["w"], a["out"])
    big = (1 << 29) + 1
    refused = [dict(tab=None), dict(out=None), dict(ncol=-1), dict(ld_tab=NCOL - 1),
               dict(ncol=big, ld_tab=big), dict(m0=-1), dict(m0=12), dict(m1=-1), dict(m1=12),
               dict(w=1.0), dict(w=-0.25), dict(w=1.5), dict(w=float("nan")),
               dict(w=float("inf"))]
    for kw in refused:
        assert call(**kw) == -1, kw
    s = C.c_void_p(torch.cuda.current_stream(0).cuda_stream)
    assert eng._lib.nmp_static_monthly(None, NCOL, LD_TAB, C.c_void_p(tab.data_ptr()), 3, 4, 0.5,
                                       C.c_void_p(row.data_ptr()), s) == -1
    assert call(ncol=0) == 0 and call(ncol=0, tab=None, out=None) == 0
    torch.cuda.synchronize()
    assert (row.cpu().numpy() == SENTINEL).all()       # nothing was enqueued
    assert call() == 0
    torch.cuda.synchronize()
    got = row.cpu().numpy()
    assert (got[:NCOL] != SENTINEL).all() and (got[NCOL:] == SENTINEL).all()
    eng.close()


# ---- 2. the driver, synthetic columns -----------------------------------------------------
def _nml(tmp, start=START, end=START + 36 * HOUR, dt=3600):
    tmp.mkdir(parents=True, exist_ok=True)
    text = open(os.path.join(ROOT, "examples", "offline_case.nml")).read()
    for k in ("geo_em.d01.nc", "init.nc", "ldasin", "ldasout", "restart"):
        text = text.replace(f"'{k}'", f"'{tmp / k}'").replace(f'"{k}"', f'"{tmp / k}"')
    text = text.replace("interval_seconds = 900", f"interval_seconds = {dt}")
    for pre, t in (("start", start), ("end", end)):
        for fld in ("year", "month", "day", "hour"):
            text, k = re.subn(rf"{pre}_{fld} = \d+", f"{pre}_{fld} = {getattr(t, fld)}", text)
            assert k == 1, (pre, fld)
    nml = tmp / "case.nml"
    nml.write_text(text)
    return str(nml)


def seasonal_table(n, seed=0):
    """(12, n) float32 months between 0.1 and 0.9: a cosine of seeded phase
    and amplitude around 0.5 per column."""
    rng = np.random.default_rng(seed)
    amp, peak = rng.uniform(0.2, 0.4, n), rng.uniform(0.0, 12.0, n)
    m = np.arange(12.0)[:, None]
    g = (0.5 + amp[None, :] * np.cos(2.0 * np.pi * (m - peak[None, :]) / 12.0)).astype(np.float32)
    assert g.min() >= 0.1 and g.max() <= 0.9
    return g


def mixed_columns(n=96):
    """single_casenml_mixed's kind (tests/golden/make_golden.py): mixed columns, seed 11."""
    P = Params.builtin()
    return P, cases.make_columns(n, "mixed", P.as_dict(), seed=11, julian=timeman.julian(START))


def reference_trajectory(cfg, cols, g, nsteps, cadence):
    """The reference itself (oracle/ref.py step) from the columns' state over
    nsteps steps of the driver's synthetic forcing, static_f[SHDFAC] set from
    shdfac_host for each step's instant (cadence None: frozen at the run's
    first instant, as without veg_clim).  [(state, isnow)] after each step."""
    import ref
    opts = dict(L.CASE_NML_OPTIONS)
    opts.update(cfg.engine_options())
    ref.configure(tuple(opts[k] for k in L.OPTION_NAMES))
    forcing = driver.SyntheticForcing(cols)
    st, isn = cols.state.copy(), cols.isnow.copy()
    sf = np.array(cols.static_f, np.float32)
    out, t = [], cfg.begdatetime
    for k in range(nsteps):
        when = cfg.begdatetime if cadence is None else vegclim.quantise(t, cadence)
        sf[SHD] = vegclim.shdfac_host(g, when)
        st, isn, _, _ = ref.step(cases.CASE_NML_ZSOIL, cfg.timestep.total_seconds(),
                                 timeman.yearlen(t.year), timeman.julian(t), st, isn, sf,
                                 cols.static_i, forcing(k, t))
        out.append((st, isn))
        t = t + cfg.timestep
    return out


@pytest.mark.parametrize("cadence,nsteps", [("daily", 30), ("step", 8)])
def test_the_reference_follows_the_moving_row(engine_lib, tmp_path, cadence, nsteps):
    import ref
    if not ref.available():
        pytest.skip("reference oracle not built (oracle/_ref)")
    cfg = config.Config(_nml(tmp_path))
    P, cols = mixed_columns()
    g = seasonal_table(cols.n, seed=3)
    # on the reference side alone: the moving row changes the trajectory
    moving = reference_trajectory(cfg, cols, g, nsteps, cadence)
    frozen = reference_trajectory(cfg, cols, g, nsteps, None)
    differ = ~bit_equal(moving[-1][0], frozen[-1][0]).all(0)
    print(f"{cadence}: {int(differ.sum())} of {cols.n} columns differ from the frozen row's "
          f"trajectory after {nsteps} steps")
    assert differ.mean() >= 0.25
    drv = driver.OfflineDriver(cfg, cols, params=P, write=False, veg_clim=cadence, greenfrac=g)
    t = cfg.begdatetime
    for k in range(nsteps):
        drv.run(nsteps=1)
        got, gi = drv.cs.state.cpu().numpy(), drv.cs.isnow.cpu().numpy()
        want, wi = moving[k]
        ok = bit_equal(got, want).all(0)
        assert ok.all(), f"step {k + 1}: {(~ok).sum()} of {cols.n} columns differ"
        assert np.array_equal(gi, wi), f"step {k + 1}: ISNOW differs"
        row = drv.cs.static_f[SHD].cpu().numpy()
        assert np.array_equal(ibits(row), ibits(vegclim.shdfac_host(g, vegclim.quantise(t, cadence))))
        t = t + cfg.timestep
    assert drv.step_index == nsteps and t > datetime.datetime(2000, 1, 2)   # across a midnight
    drv.engine.close()


def _end(drv):
    return (drv.cs.state.cpu().numpy(), drv.cs.isnow.cpu().numpy(), drv.cs.status.cpu().numpy(),
            drv.cs.static_f.cpu().numpy())


def _same_end(a, b, rows=4):
    return all(np.array_equal(ibits(x) if x.dtype.kind == "f" else x,
                              ibits(y) if y.dtype.kind == "f" else y)
               for x, y in zip(a[:rows], b[:rows]))


@pytest.mark.parametrize("precision", [4, 8])
def test_stream_ranges(engine_lib, tmp_path, precision):
    """streams=1 and streams=2 give the same bits across a midnight."""
    nml = _nml(tmp_path)
    P, cols = mixed_columns()
    g = seasonal_table(cols.n, seed=4)
    ends = []
    for streams in (1, 2, 3):
        d = driver.OfflineDriver(config.Config(nml), cols, params=P, write=False, streams=streams,
                                 precision=precision, veg_clim="daily", greenfrac=g)
        d.run(nsteps=8)
        assert d.t == START + 8 * HOUR
        ends.append(_end(d))
        d.engine.close()
    assert _same_end(ends[0], ends[1]) and _same_end(ends[0], ends[2])
    want = vegclim.shdfac_host(g, datetime.datetime(2000, 1, 2), _np(precision))
    assert np.array_equal(ibits(ends[0][3][SHD]), ibits(want))
    # and the option did something: the run without it ends elsewhere
    d = driver.OfflineDriver(config.Config(nml), cols, params=P, write=False, precision=precision)
    d.run(nsteps=8)
    assert not _same_end(ends[0], _end(d), rows=1)
    d.engine.close()


def test_a_table_without_the_option_is_not_looked_at(engine_lib, tmp_path):
    """(tests/test_vegclim_host.py holds the refusals: they need no device.)"""
    cfg = config.Config(_nml(tmp_path))
    P, cols = mixed_columns(8)
    d = driver.OfflineDriver(cfg, cols, params=P, write=False, greenfrac=seasonal_table(8)[:3])
    assert d.veg_clim is None and d._veg_table is None
    d.engine.close()


def test_spinup(engine_lib, tmp_path):
    """spinup(2) over a two-day period with "daily": every pass starts from the
    start day's row, and the end state is a manual loop's that sets the row on
    the host."""
    nml = _nml(tmp_path, end=START + 48 * HOUR)
    P, cols = mixed_columns()
    g = seasonal_table(cols.n, seed=5)
    day = lambda t: vegclim.shdfac_host(g, vegclim.quantise(t, "daily"))  # noqa: E731
    a = driver.OfflineDriver(config.Config(nml), cols, params=P, write=False, veg_clim="daily",
                             greenfrac=g)
    a.spinup(1, report=False)
    assert (a.t, a.step_index) == (START, 0)
    # pass 1 left the last day's row; the first step of pass 2 re-forms the start day's
    assert np.array_equal(ibits(a.cs.static_f[SHD].cpu().numpy()), ibits(day(START + 47 * HOUR)))
    a.run(nsteps=1)
    assert np.array_equal(ibits(a.cs.static_f[SHD].cpu().numpy()), ibits(day(START)))
    assert not np.array_equal(ibits(day(START)), ibits(day(START + 47 * HOUR)))
    a.engine.close()
    b = driver.OfflineDriver(config.Config(nml), cols, params=P, write=False, veg_clim="daily",
                             greenfrac=g)
    b.spinup(2, report=False)
    spun = _end(b)
    b.engine.close()
    # the manual loop: a driver without the option per pass, the row set on the host
    prev = None
    for _ in range(2):
        m = driver.OfflineDriver(config.Config(nml), cols, params=P, write=False)
        if prev is not None:
            m.cs.state.copy_(_dev(prev[0]))
            m.cs.isnow.copy_(_dev(prev[1]))
        for _k in range(48):
            m.cs.static_f[SHD].copy_(_dev(day(m.t)))
            m.run(nsteps=1)
        assert m.t == START + 48 * HOUR
        prev = _end(m)
        m.engine.close()
    assert _same_end(spun, prev, rows=2)


# ---- 3. the driver, from files -----------------------------------------------------------
def _tool():
    spec = importlib.util.spec_from_file_location(
        "make_offline_case", os.path.join(ROOT, "tools", "make_offline_case.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _case(tmp, seasonal, hours=36):
    """make_offline_case's 6 x 16 grid of mixed columns from 20:00, hourly steps and files."""
    nml = _nml(tmp, end=START + hours * HOUR)
    _tool().main([nml, "--ny", "6", "--nx", "16", "--kind", "mixed"] +
                 (["--seasonal-greenfrac"] if seasonal else []))
    return nml


def _cfg(nml, tmp, name):
    cfg = config.Config(nml)
    cfg.outdir, cfg.resdir = str(tmp / f"out_{name}"), str(tmp / f"res_{name}")
    return cfg


@pytest.fixture(scope="module")
def seasonal_case(engine_lib, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("vegclim_files")
    nml = _case(tmp / "case", True)
    d = driver.OfflineDriver.from_files(_cfg(nml, tmp, "whole"), write=False, veg_clim="daily")
    d.run(nsteps=30)
    out = dict(tmp=tmp, nml=nml, whole=_end(d), perm=d.perm.copy(),
               row_grid_order=d.to_grid_order(d.cs.static_f[SHD].cpu().numpy()), grid=d.grid)
    d.engine.close()
    return out


def test_files_and_order(seasonal_case):
    """from_files in the coherent order: the row, taken back to land-point
    order, is the twin's from read_greenfrac's table."""
    cfg = config.Config(seasonal_case["nml"])
    g = ncio.read_greenfrac(cfg.constfile, seasonal_case["grid"])
    assert g.shape == (12, 96) and (g.max(0) - g.min(0) > 0.01).any()
    assert not np.array_equal(seasonal_case["perm"], np.arange(96))    # the order is on
    want = vegclim.shdfac_host(g, datetime.datetime(2000, 1, 3))       # step 30 starts 01-03 01:00
    assert np.array_equal(ibits(seasonal_case["row_grid_order"]), ibits(want))
    assert not np.array_equal(ibits(want), ibits(vegclim.shdfac_host(g, START)))
    # the driver's table is the file's in the engine's order
    d = driver.OfflineDriver.from_files(cfg, write=False, veg_clim="step")
    assert np.array_equal(ibits(d._veg_table.cpu().numpy()), ibits(g[:, d.perm]))
    d.run(nsteps=5)                                                    # the last step starts 00:00
    assert np.array_equal(ibits(d.to_grid_order(d.cs.static_f[SHD].cpu().numpy())),
                          ibits(vegclim.shdfac_host(g, START + 4 * HOUR)))
    d.engine.close()
    # a static file without the table is refused before any device work
    bare = seasonal_case["tmp"] / "bare.nc"
    from scipy.io import netcdf_file
    src = netcdf_file(cfg.constfile, "r", mmap=False)
    dst = netcdf_file(str(bare), "w")
    for name, size in src.dimensions.items():
        dst.createDimension(name, size)
    for name, v in src.variables.items():
        if name != "GREENFRAC":
            dst.createVariable(name, v.data.dtype, v.dimensions)[:] = v[:]
    dst.close()
    src.close()
    cfg.constfile = str(bare)
    with pytest.raises(ValueError, match="GREENFRAC"):
        driver.OfflineDriver.from_files(cfg, write=False, veg_clim="daily")


@pytest.mark.parametrize("kind", ["nc", "npz"])
def test_restart(seasonal_case, kind):
    """30 steps uninterrupted = 10 steps, a restart file, a new driver, 20 steps."""
    tmp, nml = seasonal_case["tmp"], seasonal_case["nml"]
    a = driver.OfflineDriver.from_files(_cfg(nml, tmp, f"a_{kind}"), write=False, veg_clim="daily")
    a.run(nsteps=10)
    assert a.t == START + 10 * HOUR
    path = str(tmp / f"restart10.{kind}")
    a.save_restart(path)
    a.engine.close()
    b = driver.OfflineDriver.from_files(_cfg(nml, tmp, f"b_{kind}"), write=False, veg_clim="daily")
    start_row = b.cs.static_f[SHD].cpu().numpy()
    b.load_restart(path)
    assert (b.t, b.step_index) == (START + 10 * HOUR, 10) and b._veg_key is None
    b.run(nsteps=1)
    g = ncio.read_greenfrac(b.cfg.constfile, b.grid)[:, b.perm]
    day2 = vegclim.shdfac_host(g, datetime.datetime(2000, 1, 2))
    assert np.array_equal(ibits(b.cs.static_f[SHD].cpu().numpy()), ibits(day2))
    assert not np.array_equal(ibits(start_row), ibits(day2))
    b.run(nsteps=19)
    # (state and ISNOW: a state file carries no status bits)
    assert _same_end(_end(b), seasonal_case["whole"], rows=2)
    assert np.array_equal(ibits(_end(b)[3]), ibits(seasonal_case["whole"][3]))
    b.engine.close()


def test_jump_back_in_time(seasonal_case):
    """One driver: 2 steps, a restart, on to step 10 (the next day's row), back
    to step 2 (the state file does not carry static_f), on to step 30."""
    tmp, nml = seasonal_case["tmp"], seasonal_case["nml"]
    d = driver.OfflineDriver.from_files(_cfg(nml, tmp, "jump"), write=False, veg_clim="daily")
    d.run(nsteps=2)
    path = str(tmp / "restart2.nc")
    d.save_restart(path)
    d.run(nsteps=8)
    g = ncio.read_greenfrac(d.cfg.constfile, d.grid)[:, d.perm]
    assert np.array_equal(ibits(d.cs.static_f[SHD].cpu().numpy()),
                          ibits(vegclim.shdfac_host(g, datetime.datetime(2000, 1, 2))))
    d.load_restart(path)
    assert (d.t, d.step_index) == (START + 2 * HOUR, 2)
    d.run(nsteps=1)
    assert np.array_equal(ibits(d.cs.static_f[SHD].cpu().numpy()),
                          ibits(vegclim.shdfac_host(g, datetime.datetime(2000, 1, 1))))
    d.run(nsteps=27)
    assert _same_end(_end(d), seasonal_case["whole"])
    d.engine.close()


def test_nothing_moves_when_nothing_should(engine_lib, tmp_path):
    """A climatology of 12 equal rows (the case writer's default file), either
    cadence: state, ISNOW, status, static_f and every output file's bytes are
    the run's without the option."""
    nml = _case(tmp_path / "case", False, hours=9)
    runs = {}
    for name, kw in (("off", {}), ("daily", dict(veg_clim="daily")), ("step", dict(veg_clim="step"))):
        cfg = _cfg(nml, tmp_path, name)
        d = driver.OfflineDriver.from_files(cfg, accumulate=True, state_out="all", **kw)
        d.run()
        assert d.step_index == 9 and d.t.day == 2 and len(d.written) == 3
        files = {os.path.basename(p): open(p, "rb").read() for p in d.written}
        runs[name] = (_end(d), files, d._veg_table is not None)
        d.engine.close()
    assert runs["off"][2] is False and runs["daily"][2] and runs["step"][2]
    for name in ("daily", "step"):
        assert _same_end(runs[name][0], runs["off"][0], rows=4), name
        assert runs[name][1].keys() == runs["off"][1].keys()
        for f, data in runs["off"][1].items():
            assert runs[name][1][f] == data, (name, f)
