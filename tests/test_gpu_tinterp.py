"""Forcing between input times on the GPU: nmp_ldasin_cosz against the COSZ
row nmp_forcing_from_ldasin_geo writes, nmp_forcing_from_ldasin_interp against
its numpy twin (tinterp.interp_host, given the device's own three COSZ rows)
bit for bit, the w1 = 0 path, the argument checks with a live engine, and the
offline driver with interp=True: every step's device forcing against the twin,
the run against one fed the same arrays from the host, restart inside an
interval, the held closing interval, a missing file, and the three block slots
with and without the read-ahead."""
import ctypes as C
import datetime
import glob
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

import noahmp_pkg  # noqa: F401
from golden_io import bit_equal
from noahmp_amd import config, driver, feeds, layout as L, ncio, timeman, tinterp
from noahmp_amd.regrid import downscale_host
from test_regrid_host import _block, bits
from test_tinterp_host import RAIN, SW, same

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V, F = L.LDASIN.index, L.FORCING.index
N, LD = 1031, 1100
T0 = datetime.datetime(2001, 3, 21, 9)
T1 = T0 + datetime.timedelta(hours=3)


def _engine(precision=4):
    from noahmp_amd.engine import Engine
    from noahmp_amd.params import Params
    return Engine(Params.builtin(), L.CASE_NML_OPTIONS, device=0, precision=precision)


def _solar(t):
    return timeman.solar_terms(timeman.julian(t), timeman.yearlen(t.year))


def _geo(seed=0):
    """(3, LD) geo of N columns over the globe, both poles and the equator
    among them; the pad columns hold NaN."""
    rng = np.random.default_rng(seed)
    lat = np.radians(rng.uniform(-89.0, 89.0, N))
    lat[:4] = np.radians([90.0, -90.0, 0.0, 89.999])
    lon = np.radians(rng.uniform(-180.0, 180.0, N))
    g = np.full((3, LD), np.nan)
    g[0, :N], g[1, :N], g[2, :N] = np.sin(lat), np.cos(lat), lon
    return g


def _pair(seed=0):
    """Two (NLDASIN, LD) blocks with NaN, +-0, a denormal and a NaN payload
    among their entries (the COSZ rows are the device's to write)."""
    b0, b1 = _block(LD, seed), _block(LD, seed + 50)
    b0[V("T2D"), 7], b1[V("Q2D"), 8], b0[V("SWDOWN"), 9], b1[V("SWDOWN"), 10] = (np.nan,) * 4
    b0[V("U2D"), 11], b1[V("U2D"), 11], b0[V("V2D"), 12], b1[V("V2D"), 12] = -0.0, 0.0, -0.0, -0.0
    b0[V("SWDOWN"), 13:16], b1[V("SWDOWN"), 14:17] = 0.0, -0.0
    b0[V("LWDOWN"), 17] = 1e-41
    b0[V("RAINRATE")].view(np.uint32)[18] = 0x7FC12345
    b1[V("PSFC"), 19] = np.nan
    return b0, b1


@pytest.fixture(scope="module")
def device_rows(engine_lib):
    """The geo, the two blocks with the device's COSZ rows at T0 and T1, on the
    host and on the device (shared, not modified)."""
    eng = _engine()
    g = _geo()
    b0, b1 = _pair()
    geo = torch.as_tensor(g, device=DEV)
    d0, d1 = torch.as_tensor(b0, device=DEV), torch.as_tensor(b1, device=DEV)
    eng.ldasin_cosz(d0, geo, _solar(T0), cols=(0, N))
    eng.ldasin_cosz(d1, geo, _solar(T1), cols=(0, N))
    torch.cuda.synchronize()
    h0, h1 = d0.cpu().numpy(), d1.cpu().numpy()
    eng.close()
    return g, geo, d0, d1, h0, h1, b0, b1


def test_ldasin_cosz_is_the_geo_kernels_row(engine_lib, device_rows):
    g, geo, d0, d1, h0, h1, b0, b1 = device_rows
    eng = _engine()
    for t, h, b, d in ((T0, h0, b0, d0), (T1, h1, b1, d1)):
        out = torch.full((L.NFORCING, LD), -7.0, device=DEV)
        eng.forcing_from_ldasin(d, out, cols=(0, N), geo=geo, solar=_solar(t))
        torch.cuda.synchronize()
        want = out.cpu().numpy()[F("COSZ")]
        assert np.array_equal(bits(h[V("COSZ"), :N]), bits(want[:N]))
        assert (want[N:] == -7.0).all()
        # the pad columns and the other 8 rows are untouched
        assert np.array_equal(bits(h[V("COSZ"), N:]), bits(b[V("COSZ"), N:]))
        assert np.array_equal(bits(h[:8]), bits(b[:8]))
    cz = h0[V("COSZ"), :N]
    assert (cz > 0.05).any() and (cz < 0).any() and ((cz > 0) & (cz < 0.05)).any()
    lat = np.arcsin(np.clip(g[0, :N], -1, 1))
    host = tinterp.cosz_row_host(lat, g[2, :N], T0, (g[0, :N], g[1, :N]))
    d = np.abs(bits(cz).astype(np.int64) - bits(host).astype(np.int64))
    print(f"ldasin_cosz: {int((d == 1).sum())} of {N} values differ from numpy's by 1 fp32 ulp, "
          f"{int((d > 1).sum())} by more")
    eng.close()


W1S = (0.0, 2.0 ** -20, 0.25, 1 / 3, 0.5, 1 - 2.0 ** -20)
MASKS = (0, RAIN, RAIN | SW, 0xFF)


@pytest.mark.parametrize("precision", [4, 8])
def test_interp_equals_the_twin(engine_lib, device_rows, precision):
    g, geo, d0, d1, h0, h1, _, _ = device_rows
    eng = _engine(precision)
    np_t = np.float32 if precision == 4 else np.float64
    t = T0 + datetime.timedelta(seconds=4500)
    solar = _solar(t)
    ulp1 = None
    for w1 in W1S:
        for mask in MASKS:
            for zen in (True, False):
                out = torch.full((L.NFORCING, LD), -7.0, dtype=eng.dtype, device=DEV)
                eng.forcing_from_ldasin_interp(d0, d1, w1, out, geo, solar, mask, zen, 0.05,
                                               cols=(0, N))
                torch.cuda.synchronize()
                got = out.cpu().numpy()
                assert (got[:, N:] == -7.0).all()
                got = got[:, :N]
                g32 = got.astype(np.float32)
                czt = g32[F("COSZ")]
                want = tinterp.interp_host(h0[:, :N], h1[:, :N], w1, czt, mask, zen, 0.05)
                assert same(g32, want), (w1, mask, zen)
                # an fp32 value widened: nothing but the rounding to fp32 happened
                assert got.dtype == np_t and bit_equal(got, g32.astype(np_t)).all()
                if ulp1 is None:
                    lat = np.arcsin(np.clip(g[0, :N], -1, 1))
                    host = tinterp.cosz_row_host(lat, g[2, :N], t, (g[0, :N], g[1, :N]))
                    ulp1 = int((np.abs(bits(czt).astype(np.int64) -
                                       bits(host).astype(np.int64)) == 1).sum())
                    # the cases the scheme distinguishes are all there
                    c0, c1 = h0[V("COSZ"), :N], h1[V("COSZ"), :N]
                    assert ((c0 < 0.05) & (c1 > 0.05)).any() and ((c1 < 0.05) & (c0 > 0.05)).any()
                    assert (czt <= 0).any() and ((czt > 0) & (c0 < 0.05) & (c1 < 0.05)).any()
    print(f"interp fp{8 * precision}: {ulp1} of {N} czt values differ from numpy's by 1 fp32 ulp")
    # three column ranges give the one-launch result
    whole = torch.full((L.NFORCING, LD), -7.0, dtype=eng.dtype, device=DEV)
    parts = torch.full((L.NFORCING, LD), -7.0, dtype=eng.dtype, device=DEV)
    eng.forcing_from_ldasin_interp(d0, d1, 1 / 3, whole, geo, solar, RAIN, True, 0.05, cols=(0, N))
    for rng in ((0, 300), (300, 777), (777, N)):
        eng.forcing_from_ldasin_interp(d0, d1, 1 / 3, parts, geo, solar, RAIN, True, 0.05,
                                       cols=rng)
    torch.cuda.synchronize()
    assert bit_equal(parts.cpu().numpy(), whole.cpu().numpy()).all()
    eng.close()


@pytest.mark.parametrize("precision", [4, 8])
def test_w1_zero_is_the_geo_launch(engine_lib, device_rows, precision):
    g, geo, d0, d1, _, _, _, _ = device_rows
    eng = _engine(precision)
    solar = _solar(T0)
    want = torch.full((L.NFORCING, LD), -7.0, dtype=eng.dtype, device=DEV)
    eng.forcing_from_ldasin(d0, want, cols=(0, N), geo=geo, solar=solar)
    nan1 = torch.full_like(d1, float("nan"))
    for blk1 in (nan1, None):
        for mask, zen in ((RAIN, True), (0, False), (0xFF, True)):
            out = torch.full((L.NFORCING, LD), -7.0, dtype=eng.dtype, device=DEV)
            eng.forcing_from_ldasin_interp(d0, blk1, 0.0, out, geo, solar, mask, zen, 0.05,
                                           cols=(0, N))
            torch.cuda.synchronize()
            assert bit_equal(out.cpu().numpy(), want.cpu().numpy()).all()
    eng.close()


def test_interp_entries_reject_bad_arguments(engine_lib, device_rows):
    from noahmp_amd.engine import _ptr
    g, geo, d0, d1, h0, _, _, _ = device_rows
    eng = _engine()
    lib, h = eng._lib, eng._h
    out = torch.full((L.NFORCING, LD), 7.0, device=DEV)
    blk = d0.clone()
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    sd, cd, ha0 = _solar(T0)

    def interp(eng=h, ncol=N, ld=LD, b0=d0, b1=d1, w1=0.5, mask=RAIN, zen=1, floor=0.05, geo=geo,
               out=out):
        return lib.nmp_forcing_from_ldasin_interp(eng, ncol, ld, _ptr(b0), _ptr(b1), w1, mask, zen,
                                                  floor, _ptr(geo), sd, cd, ha0, _ptr(out), s)

    def cosz(eng=h, ncol=N, ld=LD, geo=geo, blk=blk):
        return lib.nmp_ldasin_cosz(eng, ncol, ld, _ptr(geo), sd, cd, ha0, _ptr(blk), s)
    assert interp(eng=None) == -1 and cosz(eng=None) == -1
    assert interp(ld=N - 1) == -1 and cosz(ld=N - 1) == -1
    assert interp(ncol=-1) == -1 and cosz(ncol=-1) == -1
    for k in ("b0", "geo", "out"):
        assert interp(**{k: None}) == -1, k
        assert interp(w1=0.0, **{k: None}) == -1, k
    assert interp(b1=None) == -1
    for w1 in (1.0, -2.0 ** -30, 1.5, float("nan"), float("inf")):
        assert interp(w1=w1) == -1, w1
    assert interp(mask=1 << V("COSZ")) == -1 and interp(mask=1 << 31) == -1
    for floor in (0.0, -0.05, 1.0001, float("nan")):
        assert interp(floor=floor) == -1, floor
        assert interp(floor=floor, ncol=0) == -1       # the settings are still checked
    for k in ("geo", "blk"):
        assert cosz(**{k: None}) == -1, k
    assert interp(ncol=0) == 0 and cosz(ncol=0) == 0
    assert interp(ncol=0, b0=None, b1=None, geo=None, out=None) == 0   # nothing is looked at
    assert cosz(ncol=0, geo=None, blk=None) == 0
    torch.cuda.synchronize()
    assert (out == 7.0).all()
    assert np.array_equal(bits(blk.cpu().numpy()), bits(h0))
    # what is allowed: no floor without the zenith scheme, a floor of 1, block 1 unused at w1 = 0
    assert interp(zen=0, floor=0.0) == 0 and interp(floor=1.0) == 0
    assert interp(w1=0.0, b1=None) == 0
    torch.cuda.synchronize()
    eng.close()


# ---- the offline driver ---------------------------------------------------------------------
def _case(tmp_path, infreq="3 hour", dt=900, end=(2, 0), closing=True, fgrid=False):
    """make_offline_case's 4 x 8 example day (or a part of it) with its own
    input frequency and time step."""
    tmp_path.mkdir(exist_ok=True)
    text = open(os.path.join(ROOT, "examples", "offline_case.nml")).read()
    for k in ("geo_em.d01.nc", "init.nc", "ldasin", "ldasout", "restart"):
        text = text.replace(f"'{k}'", f"'{tmp_path / k}'").replace(f'"{k}"', f'"{tmp_path / k}"')
    text = text.replace("input_frequency = '1 hour'", f"input_frequency = '{infreq}'")
    text = text.replace("interval_seconds = 900", f"interval_seconds = {dt}")
    text = text.replace("end_day = 2 end_hour = 0", f"end_day = {end[0]} end_hour = {end[1]}")
    nml = tmp_path / "case.nml"
    nml.write_text(text)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import make_offline_case
    make_offline_case.main([str(nml), "--ny", "4", "--nx", "8"] +
                           (["--closing-file"] if closing else []) +
                           (["--forcing-grid", "3", "4"] if fgrid else []))
    cfg = config.Config(str(nml))
    assert cfg.input_interval == config.parse_frequency(infreq)
    assert os.path.isfile(ncio.ldasin_path(cfg.indir, cfg.enddatetime)) == closing
    return cfg


def _result(drv, cfg):
    files = sorted(glob.glob(os.path.join(cfg.outdir, "*.LDASOUT_DOMAIN1")))
    return (drv.to_grid_order(drv.cs.state.cpu().numpy()),
            drv.to_grid_order(drv.cs.isnow.cpu().numpy()), [open(f, "rb").read() for f in files])


def _same_run(a, b):
    return bit_equal(a[0], b[0]).all() and np.array_equal(a[1], b[1]) and len(a[2]) > 0 and \
        a[2] == b[2]


def _drive(cfg, tmp_path, tag, nsteps=None, **kw):
    cfg.outdir = str(tmp_path / f"out_{tag}")
    drv = driver.OfflineDriver.from_files(cfg, **kw)
    drv.run(nsteps)
    return drv


KINDS = {"ingest": dict(), "host-block": dict(ingest=False),
         "regrid-downscale": dict(downscale=True)}


@pytest.mark.parametrize("kind", list(KINDS))
def test_driver_steps_equal_the_twin(engine_lib, tmp_path, kind):
    """Every step's device forcing is interp_host of the interval's two blocks
    (the files' host blocks but for the device's COSZ rows; with downscale the
    device's exponential may move PSFC and Q2D by one ulp, so the device's
    blocks are the twin's input there); the run equals one fed those arrays
    through HostFeed, stepwise and uninterrupted."""
    fgrid = kind == "regrid-downscale"
    cfg = _case(tmp_path / "case", fgrid=fgrid)
    kw = dict(KINDS[kind])
    if fgrid:
        kw["forcing_grid"] = os.path.join(cfg.indir, "forcing_grid.nc")
    a = _drive(cfg, tmp_path, "a", nsteps=0, interp=True, **kw)
    assert a.feed.kind == "ldasin-interp" and a.interp
    assert (a.ingest is None) == (kind == "host-block")
    fr, every, fs = a.forcing, cfg.input_interval, []
    dz = fr.dz() if fgrid else None
    for k in range(96):
        t = a.t
        a.run(1)
        f = a.feed.last.f.cpu().numpy()
        ti = fr.input_time(t)
        w1 = tinterp.weights(t, ti, every)[1]
        blks = []
        for tb in (ti, ti + every)[:2 if w1 else 1]:
            dev = a.feed.blocks[tb][0].cpu().numpy()
            host = fr.block(tb).copy()
            if fgrid:
                host = downscale_host(np.vstack([host[:8], dev[8:]]), dz, 0.0065)
            d = np.abs(bits(dev[:8]).astype(np.int64) - bits(host[:8]).astype(np.int64))
            loose = [V("PSFC"), V("Q2D")] if fgrid else []
            assert d[loose].max(initial=0) <= 1 and np.delete(d, loose, 0).max() == 0, (k, tb)
            blks.append(dev)
        want = tinterp.interp_host(blks[0], blks[-1], w1, f[F("COSZ")], RAIN, True, 0.05)
        assert same(f, want), k
        if w1:   # and the step is not the held one
            assert not np.array_equal(f[F("SFCTMP")], blks[0][V("T2D")])
        fs.append(want)
    assert a.step_index == 96 and a.interp_held == []
    ra = _result(a, cfg)
    assert len(ra[2]) == 8 and np.isfinite(ra[0][L.s("STC")]).all()
    # the same arrays from the host, uninterrupted
    cfg.outdir = str(tmp_path / "out_b")
    b = driver.OfflineDriver.from_files(cfg, **kw)
    b.feed = feeds.HostFeed(lambda k, t: fs[k], b.cs.ncol, b.dtype, b.dev)
    b.run()
    rb = _result(b, cfg)
    c = _drive(cfg, tmp_path, "c", interp=True, **kw)
    assert _same_run(ra, rb) and _same_run(_result(c, cfg), rb)
    assert c.feed.up.count == 9                # one block per file, the closing one included
    # and interpolation does change the run
    h = _drive(cfg, tmp_path, "h", **kw)
    assert not bit_equal(_result(h, cfg)[0], rb[0]).all()
    for d in (a, b, c, h):
        d.engine.close()


def test_restart_inside_an_interval(engine_lib, tmp_path):
    cfg = _case(tmp_path / "case")
    u = _drive(cfg, tmp_path, "u", interp=True)
    ru = _result(u, cfg)
    r1 = _drive(cfg, tmp_path, "r", nsteps=17, interp=True)   # 04:15, inside [03:00, 06:00)
    path = str(tmp_path / "restart_0415.nc")
    r1.save_restart(path)
    r1.flush_output()
    r2 = driver.OfflineDriver.from_files(cfg, init=path, interp=True)
    assert r2.step_index == 17 and r2.t == cfg.begdatetime + 17 * cfg.timestep
    r2.run()
    assert r2.step_index == 96
    assert _same_run(_result(r2, cfg), ru)
    # a restart loaded into a running driver rebuilds both blocks
    r1.load_restart(path)
    assert r1.feed.blocks == {}
    r1.run()
    assert _same_run(_result(r1, cfg), ru)
    for d in (u, r1, r2):
        d.engine.close()


def test_closing_interval_runs_held_and_a_missing_file_raises(engine_lib, tmp_path):
    cfg = _case(tmp_path / "case", closing=False)
    a = _drive(cfg, tmp_path, "a", interp=True)
    last = cfg.enddatetime - cfg.input_interval
    assert a.interp_held == [last] and a.step_index == 96
    ra = _result(a, cfg)
    # that interval alone on the held path, from the interpolating run's state at its start
    b1 = _drive(cfg, tmp_path, "b", nsteps=84, interp=True)
    path = str(tmp_path / "restart_2100.nc")
    b1.save_restart(path)
    b1.flush_output()
    assert b1.interp_held == []
    b2 = driver.OfflineDriver.from_files(cfg, init=path)
    assert b2.feed.kind == "ldasin-ingest" and b2.t == last
    b2.run()
    assert _same_run(_result(b2, cfg), ra)
    # a missing file anywhere else
    gone = ncio.ldasin_path(cfg.indir, cfg.begdatetime + 2 * cfg.input_interval)
    os.remove(gone)
    m = _drive(cfg, tmp_path, "m", nsteps=0, interp=True)
    with pytest.raises(FileNotFoundError, match=os.path.basename(gone)):
        m.run()
    torch.cuda.synchronize()
    assert m.step_index == 13          # 03:15 is the first step that needs it
    for d in (a, b1, b2, m):
        d.engine.close()


@pytest.mark.parametrize("infreq,dt,end", [("2700 second", 1800, (1, 9)), ("1 hour", 900, (1, 12))])
def test_three_slots_with_and_without_read_ahead(engine_lib, tmp_path, infreq, dt, end):
    """12 input intervals; an input time that falls between two steps, and
    four steps per file: the read-ahead changes nothing."""
    cfg = _case(tmp_path / "case", infreq=infreq, dt=dt, end=end)
    res = {}
    for ingest in (True, False):
        for pf in (True, False):
            d = _drive(cfg, tmp_path, f"{int(ingest)}{int(pf)}", interp=True, ingest=ingest,
                       prefetch=pf)
            assert d.t == cfg.enddatetime and d.feed.up.count == 13 and d.interp_held == []
            assert len(d.feed.blocks) <= 3
            # the host-built block is formed ahead right after the launch; the
            # file's bytes are read ahead on a thread and go up once they are there
            if not pf or not ingest:
                assert d.feed.read_ahead == (12 if pf else 0)
            print(f"{infreq}, ingest={ingest}, prefetch={pf}: {d.feed.read_ahead} of 13 blocks "
                  "formed ahead of the step that needs them")
            res[ingest, pf] = _result(d, cfg)
            d.engine.close()
    for key in res:
        assert _same_run(res[key], res[True, False]), key


def test_offline_cli_interp(engine_lib, tmp_path):
    spec = importlib.util.spec_from_file_location("noahmp_offline",
                                                  os.path.join(ROOT, "noahmp_offline.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    cfg = _case(tmp_path / "plain")
    assert cli.main([str(tmp_path / "plain" / "case.nml"), "--interp"]) == 0
    assert len(glob.glob(os.path.join(cfg.outdir, "*.LDASOUT_DOMAIN1"))) == 8
    cfg = _case(tmp_path / "coarse", fgrid=True)
    assert cli.main([str(tmp_path / "coarse" / "case.nml"), "--forcing-grid",
                     os.path.join(cfg.indir, "forcing_grid.nc"), "--downscale", "--interp",
                     "--interp-hold", "RAINRATE,LWDOWN", "--interp-sw", "linear"]) == 0
    files = sorted(glob.glob(os.path.join(cfg.outdir, "*.LDASOUT_DOMAIN1")))
    assert len(files) == 8
    from noahmp_amd.params import Params
    grid, _, _ = ncio.read_static(cfg.constfile, Params.builtin().as_dict(), cfg.begdatetime)
    for f in files:
        assert np.isfinite(ncio.read_ldasout(f, grid)).all()
