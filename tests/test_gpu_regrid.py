"""Forcing on its own grid on the GPU: nmp_ldasin_regrid against its numpy
restatement (regrid.RegridPlan.apply_host) bit for bit, nmp_ldasin_downscale
against downscale_host (bit for bit but for the two rows that pass through the
double exponential), their argument checks, and the offline driver fed with
coarse LDASIN files: device-regridded, host-regridded and pre-regridded
model-grid files give the same run."""
import ctypes as C
import glob
import os

import numpy as np
import pytest
import torch

import noahmp_pkg  # noqa: F401
from golden_io import bit_equal, load
from noahmp_amd import cases, config, driver, layout as L, ncio
from noahmp_amd.regrid import RegridPlan, downscale_host, nearest_mask
from test_regrid_host import _block, _special_grids, bits

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NPTS = 35  # a 5 x 7 source


def _engine():
    from noahmp_amd.engine import Engine
    from noahmp_amd.params import Params
    return Engine(Params.builtin(), L.CASE_NML_OPTIONS, device=0, precision=4)


def _plan(ncol, seed=0):
    """Four random source entries per column of a 5 x 7 source, one in seven
    masked, normalised random weights with some exact ties; with room for them,
    one column without a valid entry and one with a corner past the grid."""
    rng = np.random.default_rng(seed)
    corner = rng.integers(0, NPTS, (4, ncol)).astype(np.int32)
    corner[rng.random((4, ncol)) < 1 / 7] = -1
    if ncol == 1:
        corner[:, 0] = (4, -1, 20, 34)
    w = np.where(corner >= 0, rng.integers(1, 9, (4, ncol)) / 8.0, 0.0)   # ties happen
    s = np.maximum(((w[0] + w[1]) + w[2]) + w[3], 0.125)
    w = w / s
    if ncol >= 3:
        corner[:, ncol // 2] = -1
        corner[2, ncol - 2] = NPTS
    return RegridPlan(ncol, NPTS, np.ascontiguousarray(corner), np.ascontiguousarray(w))


def _be_words(g):
    """fp32 grids as the file stores them, as the int32 words the engine takes."""
    return torch.as_tensor(np.ascontiguousarray(g.astype(">f4")).view(np.int32), device=DEV)


@pytest.mark.parametrize("ncol", [1, 257, 300])
def test_regrid_equals_apply_host(engine_lib, ncol):
    eng = _engine()
    g = _special_grids(np.random.default_rng(ncol))
    plan = _plan(ncol, seed=ncol)
    dplan, words = plan.to(DEV), _be_words(g)
    for near in ((), ("RAINRATE", "SWDOWN"), tuple(L.LDASIN[:-1])):
        out = torch.full((L.NLDASIN, ncol), -7.0, device=DEV)
        eng.ldasin_regrid(words, dplan, out, nearest_mask(near))
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        want = plan.apply_host(g, nearest=near)
        assert np.array_equal(bits(got[:8]), bits(want)), near
        assert (got[8] == -7.0).all()                       # COSZ is not written
        if ncol >= 3:
            assert (bits(got[:8, ncol // 2]) == 0x7FC00000).all()
            assert (bits(got[:8, ncol - 2]) == 0x7FC00000).all()
    with pytest.raises(AssertionError):
        eng.ldasin_regrid(words, plan, out)                 # the plan is not on the device
    with pytest.raises(AssertionError):
        eng.ldasin_regrid(words, _plan(ncol + 1).to(DEV), out)  # another block's plan
    with pytest.raises(AssertionError):
        eng.ldasin_regrid(words.float(), dplan, out.double())
    eng.close()


def test_regrid_launch_independence(engine_lib):
    """Two ranges with pointer offsets and ld > ncol give the whole call's bytes."""
    from noahmp_amd.engine import _ptr
    eng = _engine()
    n, a = 300, 131
    g = _special_grids(np.random.default_rng(9))
    plan = _plan(n, seed=9)
    d, words = plan.to(DEV).dev, _be_words(g)
    mask = nearest_mask(("RAINRATE",))
    whole = torch.zeros((L.NLDASIN, n), device=DEV)
    eng.ldasin_regrid(words, plan.to(DEV), whole, mask)
    parts = torch.zeros((L.NLDASIN, n), device=DEV)
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for lo, hi in ((0, a), (a, n)):
        rc = eng._lib.nmp_ldasin_regrid(eng._h, hi - lo, n, NPTS, _ptr(words), _ptr(d["corner"], lo),
                                        _ptr(d["weight"], lo), mask, _ptr(parts, lo), s)
        assert rc == 0
    torch.cuda.synchronize()
    assert np.array_equal(bits(parts.cpu().numpy()), bits(whole.cpu().numpy()))
    assert np.array_equal(bits(whole.cpu().numpy()[:8]), bits(plan.apply_host(g, nearest=(5,))))
    eng.close()


def test_downscale_equals_downscale_host(engine_lib):
    """T2D, LWDOWN and the untouched rows bit for bit; PSFC and Q2D pass through
    the double exponential, where the device's and glibc's results differ by at
    most one double ulp: after the rounding to fp32, at most one fp32 ulp."""
    eng = _engine()
    n = 300
    rng = np.random.default_rng(3)
    b = _block(n, seed=3)
    b[L.LDASIN.index("T2D")] += rng.uniform(0, 0.1, n).astype(np.float32)  # off the lattice
    dz = rng.uniform(-1500.0, 1500.0, n).astype(np.float32)
    dz[:4] = (0.0, -0.0, 1000.0, -1000.0)
    blk = torch.as_tensor(b, device=DEV)
    eng.ldasin_downscale(blk, torch.as_tensor(dz, device=DEV), 0.0065)
    torch.cuda.synchronize()
    got, want = blk.cpu().numpy(), downscale_host(b, dz, 0.0065)
    ulp1 = 0
    for i, name in enumerate(L.LDASIN):
        if name in ("PSFC", "Q2D"):
            d = np.abs(bits(got[i]).astype(np.int64) - bits(want[i]).astype(np.int64))
            ulp1 += int((d == 1).sum())
            assert d.max() <= 1, (name, int(d.max()))
        else:
            assert np.array_equal(bits(got[i]), bits(want[i])), name
    print(f"downscale: {ulp1} of {2 * n} PSFC/Q2D values differ from the host's by 1 fp32 ulp")
    assert (got[L.LDASIN.index("T2D"), 2:4] != b[L.LDASIN.index("T2D"), 2:4]).all()
    # dz = 0 is bit-identical on the device
    blk = torch.as_tensor(b, device=DEV)
    eng.ldasin_downscale(blk, torch.zeros(n, device=DEV), 0.0065)
    torch.cuda.synchronize()
    assert np.array_equal(bits(blk.cpu().numpy()), bits(b))
    with pytest.raises(AssertionError):
        eng.ldasin_downscale(blk, torch.zeros(n + 1, device=DEV), 0.0065)
    with pytest.raises(AssertionError):
        eng.ldasin_downscale(blk, torch.zeros(n, dtype=torch.float64, device=DEV), 0.0065)
    eng.close()


def test_regrid_entries_reject_bad_arguments(engine_lib):
    from noahmp_amd.engine import _ptr
    eng = _engine()
    lib, h = eng._lib, eng._h
    n = 64
    g = torch.zeros((8, NPTS), dtype=torch.int32, device=DEV)
    d = _plan(n).to(DEV).dev
    cn, w = d["corner"], d["weight"]
    blk = torch.full((L.NLDASIN, n), 7.0, device=DEV)
    dz = torch.full((n,), 100.0, device=DEV)
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    E_ARG = -1

    def regrid(eng=h, ncol=n, ld=n, npts=NPTS, g=g, cn=cn, w=w, out=blk):
        return lib.nmp_ldasin_regrid(eng, ncol, ld, npts, _ptr(g), _ptr(cn), _ptr(w), 0,
                                     _ptr(out), s)

    def down(eng=h, ncol=n, ld=n, dz=dz, out=blk):
        return lib.nmp_ldasin_downscale(eng, ncol, ld, _ptr(dz), 0.0065, _ptr(out), s)
    assert regrid(eng=None) == -1 and down(eng=None) == -1
    assert regrid(ld=n - 1) == E_ARG and down(ld=n - 1) == E_ARG
    assert regrid(ncol=-1) == E_ARG and down(ncol=-1) == E_ARG
    assert regrid(npts=0) == E_ARG and regrid(npts=-5) == E_ARG and regrid(npts=1 << 29) == E_ARG
    assert regrid(ncol=0, npts=0) == E_ARG       # sizes are still checked
    for k in ("g", "cn", "w", "out"):
        assert regrid(**{k: None}) == E_ARG, k
    for k in ("dz", "out"):
        assert down(**{k: None}) == E_ARG, k
    assert regrid(ncol=0) == 0 and down(ncol=0) == 0
    assert regrid(ncol=0, g=None, cn=None, w=None, out=None) == 0   # nothing is looked at
    torch.cuda.synchronize()
    assert (blk == 7.0).all()
    eng.close()


# ---- the offline driver on coarse files --------------------------------------------------
def _cols(g):
    return cases.ColumnSet(g["static_f"], g["static_i"], g["state0"], g["isnow0"], *([None] * 7))


def _coarse_case(tmp_path, g, hgt_m="flat"):
    """The traj_casenml columns on their grid, a 5 x 6 source grid around it and
    24 hourly LDASIN files on the source grid (the fixture's forcing of the
    first 30 columns at the 30 source points).  hgt_m: "flat" = the source's
    elevation interpolated to the model grid (every dz is 0), "real" = terrain
    of its own."""
    from test_config import write_case
    from test_ncio import grid_for
    cols = _cols(g)
    grid = grid_for(cols)
    static, init, indir = tmp_path / "geo_em.d01.nc", tmp_path / "init.nc", tmp_path / "ldasin"
    indir.mkdir()
    nml = write_case(tmp_path)
    text = open(nml).read().replace("'geo_em.d01.nc'", f"'{static}'").replace(
        '"init.nc"', f'"{init}"').replace("'ldasin'", f"'{indir}'")
    open(nml, "w").write(text)
    cfg = config.Config(nml)
    ncio.write_static(str(static), cols, grid)
    ncio.write_state(str(init), grid, g["state0"], g["isnow0"], cfg.begdatetime)
    lat, lon = grid.columns(grid.lat_deg), grid.columns(grid.lon_deg)
    rng = np.random.default_rng(0)
    fg = ncio.ForcingGrid(np.linspace(lat.max() + 1.0, lat.min() - 1.0, 5),   # north to south
                          np.linspace(lon.min() - 0.5, lon.max() + 0.5, 6),
                          hgt=rng.uniform(200.0, 1800.0, (5, 6)))
    plan = RegridPlan.bilinear(fg.lat, fg.lon, lat, lon)
    model = plan.interp_scalar(fg.hgt)
    if hgt_m == "real":
        model = model + rng.uniform(-400.0, 400.0, grid.n)
    fg.hgt_m = grid.scatter(model, 0.0)
    fgpath = str(tmp_path / "forcing_grid.nc")
    ncio.write_forcing_grid(fgpath, fg)
    t = cfg.begdatetime
    for k in range(0, 96, 4):  # hourly files (input_frequency '1 hour')
        ncio.write_ldasin(ncio.ldasin_path(str(indir), t), fg.as_grid(), g["forcing"][k][:, :30], t,
                          extras=False)
        t = t + cfg.input_interval
    return cfg, grid, fg, fgpath, plan


def _run(cfg, tmp_path, tag, **kw):
    cfg.outdir = str(tmp_path / f"out_{tag}")
    drv = driver.OfflineDriver.from_files(cfg, **kw)
    drv.run()
    assert drv.step_index == 96
    files = sorted(glob.glob(os.path.join(cfg.outdir, "*.LDASOUT_DOMAIN1")))
    assert len(files) == 8
    res = (drv.to_grid_order(drv.cs.state.cpu().numpy()),
           drv.to_grid_order(drv.cs.isnow.cpu().numpy()), [open(f, "rb").read() for f in files])
    return drv, res


def _same(a, b):
    return bit_equal(a[0], b[0]).all() and np.array_equal(a[1], b[1]) and a[2] == b[2]


@pytest.mark.parametrize("precision", [4, 8])
def test_driver_regrids_coarse_files(engine_lib, tmp_path, precision):
    """(a) the coarse files' bytes regridded on the device, (b) regridded on
    the host, (c) model-grid files written beforehand from apply_host of the
    same coarse files: the same state, ISNOW and LDASOUT bytes."""
    g = load("traj_casenml.npz")
    cfg, grid, fg, fgpath, plan = _coarse_case(tmp_path, g)
    near = ("RAINRATE",)
    a, ra = _run(cfg, tmp_path, "a", precision=precision, forcing_grid=fgpath, ingest=True,
                 nearest=near)
    assert a.ingest.count == 24 and a.raw_upload.count == 0
    assert tuple(a.ingest.host[0].shape) == (8, 30) and grid.shape[0] * grid.shape[1] == 40
    assert a.regrid_plan is not None and a.point is None
    b, rb = _run(cfg, tmp_path, "b", precision=precision, forcing_grid=fgpath, ingest=False,
                 nearest=near)
    assert b.ingest is None and b.raw_upload.count == 24
    # (c) pre-regridded files on the model grid
    pre = tmp_path / "ldasin_model"
    pre.mkdir()
    fr = a.forcing
    t = cfg.begdatetime
    inv = {v: k for k, v in ncio.LDASIN_MAP.items()}
    for _ in range(24):
        cols8 = plan.apply_host(fr.grid_raw(t), nearest=near)
        f12 = np.zeros((L.NFORCING, grid.n), np.float32)
        for i, var in enumerate(L.LDASIN[:-1]):
            f12[L.FORCING.index(inv[var])] = cols8[i]
        ncio.write_ldasin(ncio.ldasin_path(str(pre), t), grid, f12, t, extras=False)
        t = t + cfg.input_interval
    cfg.indir = str(pre)
    c, rc = _run(cfg, tmp_path, "c", precision=precision)
    assert c.ingest.count == 24 and tuple(c.ingest.host[0].shape) == (8, 40)
    assert _same(ra, rb) and _same(ra, rc)
    assert np.isfinite(ra[0][L.s("STC")]).all()
    for d in (a, b, c):
        d.engine.close()


def test_driver_downscales_on_the_device(engine_lib, tmp_path):
    g = load("traj_casenml.npz")
    flat = tmp_path / "flat"
    flat.mkdir()
    cfg, grid, fg, fgpath, _ = _coarse_case(flat, g, "flat")
    a, ra = _run(cfg, flat, "a", forcing_grid=fgpath)
    z, rz = _run(cfg, flat, "z", forcing_grid=fgpath, downscale=True)
    assert (z.dz == 0).all() and z.dz.dtype == torch.float32
    assert _same(ra, rz)                      # every dz is 0: byte-identical
    with pytest.raises(ValueError):
        driver.OfflineDriver.from_files(cfg, forcing_grid=fgpath, downscale=True, cosz="host")
    with pytest.raises(ValueError):
        driver.OfflineDriver.from_files(cfg, forcing_grid=fgpath, downscale=True,
                                        ldasin_upload=False)
    with pytest.raises(ValueError):
        driver.OfflineDriver.from_files(cfg, downscale=True)
    real = tmp_path / "real"
    real.mkdir()
    cfg, grid, fg, fgpath, _ = _coarse_case(real, g, "real")
    d1, r1 = _run(cfg, real, "dev", forcing_grid=fgpath, downscale=True, ingest=True)
    d2, r2 = _run(cfg, real, "host", forcing_grid=fgpath, downscale=True, ingest=False)
    assert d1.ingest.count == 24 and d2.raw_upload.count == 24
    assert float(d1.dz.abs().max()) > 100.0
    assert _same(r1, r2)                      # one device kernel corrects either block
    assert np.isfinite(r1[0]).all()
    assert not _same(r1, ra)                  # and the terrain does change the run
    # without the elevation fields in the file there is nothing to downscale with
    ncio.write_forcing_grid(fgpath, ncio.ForcingGrid(fg.lat, fg.lon))
    with pytest.raises(ValueError):
        driver.OfflineDriver.from_files(cfg, forcing_grid=fgpath, downscale=True)
    for d in (a, z, d1, d2):
        d.engine.close()


def test_offline_cli_runs_a_coarse_forcing_case(engine_lib, tmp_path):
    import importlib.util
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    nml = tmp_path / "case.nml"
    text = open(os.path.join(root, "examples", "offline_case.nml")).read()
    for k in ("geo_em.d01.nc", "init.nc", "ldasin", "ldasout", "restart"):
        text = text.replace(f"'{k}'", f"'{tmp_path / k}'").replace(f'"{k}"', f'"{tmp_path / k}"')
    nml.write_text(text)
    sys.path.insert(0, os.path.join(root, "tools"))
    import make_offline_case
    make_offline_case.main([str(nml), "--ny", "4", "--nx", "8", "--forcing-grid", "3", "4"])
    fgpath = str(tmp_path / "ldasin" / "forcing_grid.nc")
    fg = ncio.read_forcing_grid(fgpath)
    assert fg.shape == (3, 4) and fg.hgt is not None and fg.hgt_m.shape == (4, 8)
    first = sorted(glob.glob(str(tmp_path / "ldasin" / "*.LDASIN_DOMAIN1")))[0]
    assert ncio.read_ldasin(first)["T2D"].shape == (3, 4)
    spec = importlib.util.spec_from_file_location("noahmp_offline",
                                                  os.path.join(root, "noahmp_offline.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    assert cli.main([str(nml), "--forcing-grid", fgpath, "--downscale", "--nearest",
                     "RAINRATE"]) == 0
    files = sorted(glob.glob(str(tmp_path / "ldasout" / "*.LDASOUT_DOMAIN1")))
    assert len(files) == 8
    cfg = config.Config(str(nml))
    from noahmp_amd.params import Params
    grid, _, _ = ncio.read_static(cfg.constfile, Params.builtin().as_dict(), cfg.begdatetime)
    for f in files:
        d = ncio.read_ldasout(f, grid)
        assert d.shape == (L.NDIAG_OUT, 32) and np.isfinite(d).all()
