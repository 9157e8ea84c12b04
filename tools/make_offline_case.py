"""Write an offline case in the netCDF-3 layouts of noahmp_amd/ncio.py: the
static file, initial state and LDASIN forcing the namelist names, from the
seeded synthetic generator on a regular lat-lon grid.  noahmp_offline.py then
runs it from the files.

    python tools/make_offline_case.py case.nml [--ny 32 --nx 64 --kind conus]
                                      [--forcing-grid SY SX] [--closing-file]
                                      [--seasonal-greenfrac]

--forcing-grid SY SX: the LDASIN files are written on a coarser SY x SX
rectilinear grid that covers the model grid, with a forcing-grid file
(<input_directory>/forcing_grid.nc: the source axes, its elevation HGT and the
model terrain HGT_M, both synthetic) for `noahmp_offline.py --forcing-grid`.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import noahmp_pkg  # noqa: E402,F401
from noahmp_amd import cases, config, ncio, timeman  # noqa: E402
from noahmp_amd.params import Params  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("nmlfile")
    ap.add_argument("--ny", type=int, default=32)
    ap.add_argument("--nx", type=int, default=64)
    ap.add_argument("--lat0", type=float, default=30.0)
    ap.add_argument("--lon0", type=float, default=-120.0)
    ap.add_argument("--dlat", type=float, default=0.25)
    ap.add_argument("--kind", default="conus", choices=("mixed", "conus", "casenml"))
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--forcing-grid", type=int, nargs=2, default=None, metavar=("SY", "SX"),
                    help="write the LDASIN files on a coarser SY x SX grid, plus forcing_grid.nc")
    ap.add_argument("--closing-file", action="store_true",
                    help="also write the LDASIN file at enddatetime, which `noahmp_offline.py "
                         "--interp` reads as the last input interval's other end")
    ap.add_argument("--seasonal-greenfrac", action="store_true",
                    help="the static file's GREENFRAC gets a 12-month cycle that peaks in each "
                         "hemisphere's summer (for `noahmp_offline.py --veg-clim`) instead of "
                         "the columns' SHDFAC every month")
    a = ap.parse_args(argv)
    cfg = config.Config(a.nmlfile)
    lat = a.lat0 + a.dlat * np.arange(a.ny)[:, None] + 0.0 * np.arange(a.nx)[None, :]
    lon = a.lon0 + a.dlat * np.arange(a.nx)[None, :] + 0.0 * np.arange(a.ny)[:, None]
    grid = ncio.Grid(lat, lon, np.ones((a.ny, a.nx), bool))
    P = Params.builtin().as_dict()
    cols = cases.make_columns(grid.n, a.kind, P, seed=a.seed,
                              julian=timeman.julian(cfg.begdatetime))
    cols.static_f[0] = grid.lat_rad.astype(np.float32)  # LAT from the grid
    cols.lon = grid.lon_rad
    for path in (cfg.constfile, cfg.initfile):
        d = os.path.dirname(path)
        if d:
            os.makedirs(d, exist_ok=True)
    os.makedirs(cfg.indir, exist_ok=True)
    ncio.write_static(cfg.constfile, cols, grid,
                      greenfrac=_seasonal_greenfrac(cols) if a.seasonal_greenfrac else None)
    ncio.write_state(cfg.initfile, grid, cols.state, cols.isnow, cfg.begdatetime)
    fcols, fgrid, where = cols, grid, ""
    if a.forcing_grid:
        fcols, fgrid, where = _forcing_grid(a, cfg, lat, lon, P)
    every, t, k = cfg.input_interval, cfg.begdatetime, 0
    # (--closing-file: also the last interval's other end, the file at enddatetime)
    while t < cfg.enddatetime or (a.closing_file and t - every < cfg.enddatetime):
        f = cases.forcing_step(fcols, timeman.julian(t), timeman.yearlen(t.year), k, seed=a.seed)
        ncio.write_ldasin(ncio.ldasin_path(cfg.indir, t), fgrid, f, t, extras=False)
        t, k = t + every, k + 1
    print(f"{grid.n} columns, {k} LDASIN files in {cfg.indir}{where}; static {cfg.constfile}, "
          f"init {cfg.initfile}")


def _seasonal_greenfrac(cols):
    """(12, n) float32 mid-month GREENFRAC: the columns' SHDFAC at the peak of
    their hemisphere's summer (July north of the equator, January south of
    it), a fifth of it half a year later, a cosine between."""
    shd = np.asarray(cols.static_f[2], np.float64)
    peak = np.where(np.asarray(cols.static_f[0]) >= 0, 6.0, 0.0)
    m = np.arange(12.0)[:, None]
    g = shd[None, :] * (0.6 + 0.4 * np.cos(2.0 * np.pi * (m - peak[None, :]) / 12.0))
    return np.clip(g, 0.0, 1.0).astype(np.float32)


def _terrain(lat, lon, fine):
    """Synthetic terrain (m) at (lat, lon) degrees: broad ridges, plus -- on
    the model grid -- relief the coarse grid does not resolve."""
    h = 800.0 + 600.0 * np.sin(np.radians(lat) * 9.0) * np.cos(np.radians(lon) * 7.0)
    if fine:
        h = h + 150.0 * np.sin(np.radians(lat) * 160.0) * np.sin(np.radians(lon) * 140.0)
    return np.maximum(h, 0.0)


def _forcing_grid(a, cfg, lat, lon, P):
    """The SY x SX source grid around the model grid (half a model cell of
    margin), its synthetic columns for the forcing generator, and the
    forcing-grid file."""
    sy, sx = a.forcing_grid
    if sy < 2 or sx < 2:
        raise SystemExit("--forcing-grid needs at least 2 x 2 source points")
    pad = 0.5 * a.dlat
    slat = np.linspace(lat.min() - pad, lat.max() + pad, sy)
    slon = np.linspace(lon.min() - pad, lon.max() + pad, sx)
    fg = ncio.ForcingGrid(slat, slon, hgt=_terrain(slat[:, None], slon[None, :], False),
                          hgt_m=_terrain(lat, lon, True))
    path = os.path.join(cfg.indir, "forcing_grid.nc")
    ncio.write_forcing_grid(path, fg)
    sgrid = fg.as_grid()
    scols = cases.make_columns(sgrid.n, a.kind, P, seed=a.seed + 1,
                               julian=timeman.julian(cfg.begdatetime))
    scols.static_f[0] = sgrid.lat_rad.astype(np.float32)
    scols.lon = sgrid.lon_rad
    return scols, sgrid, f" on a {sy} x {sx} source grid ({path})"


if __name__ == "__main__":
    main()
