"""netCDF-3 files of the offline run: static grid, initial/restart state,
LDASIN forcing and LDASOUT output.

The reference names these files in its namelist (run/case.nml:2-11:
static_parameter_file, initialization_file, restart_file, input_directory,
output_directory) but ships no reader or writer for them (run/main.py stops
after the namelist).  This module supplies them in the
HRLDAS conventions Noah-MP offline runs use, as netCDF-3 classic files through
scipy.io.netcdf_file (no netCDF-4/HDF5 library exists in this image):

* static file (geo_em-style), dims (south_north, west_east[, month]):
  XLAT_M, XLONG_M (deg), LANDMASK, LU_INDEX (vegetation type), SCT_DOM (soil
  type), SLOPECAT, SOILCOLOR, SOILTEMP (deep soil T -> TBOT), GREENFRAC
  (12 monthly fractions -> SHDFAC by the date), SHDMAX (default: the
  GREENFRAC maximum), ZLVL, FOLN,
  ISLAKE/ISICE from the table's ISWATER/ISICE types;
* LDASIN, one file per input time, ``<YYYYMMDDHH>.LDASIN_DOMAIN1``:
  T2D, Q2D, U2D, V2D, PSFC, RAINRATE, SWDOWN, LWDOWN on (Time, south_north,
  west_east).  Optional extras COSZ, CO2AIR, O2AIR override the derived values
  (COSZ from the grid's lat/lon at the step's time, CO2AIR = 395e-6 PSFC,
  O2AIR = 0.209 PSFC);
* state file (initialization_file / restart_file): the engine's SoA state,
  one variable per state field (layer fields get a layer dimension), ISNOW,
  plus the model time -- the state SoA *is* the restart;
* LDASOUT, one file per output time, ``<YYYYMMDDHH>.LDASOUT_DOMAIN1``: the 16
  output fluxes on the grid, _FillValue off the land mask; an accumulating run
  (driver accumulate=True) appends its interval's 19 fields (layout.BUDGET) and
  stores the interval so far in its restart files (write_state accum,
  read_accum); a run with state output (driver state_out) appends the selected
  groups of the land state (layout.STATE_OUT), a layered group as one variable
  over (Time, soil_layers_stag | snow_layers, south_north, west_east),
  layer-major;
* REGIONS, one file per output time of a run with regions,
  ``<YYYYMMDDHH>.REGIONS_DOMAIN1``: dimension `region`, region_id, ncolumns,
  weight and one double variable per output field holding the regions'
  weighted means (write_regions / read_regions / read_regions_series); the
  region file such a run reads is an int REGION grid with an optional double
  AREA (read_region_map);
* forcing-grid file, for LDASIN files stored on a coarser rectilinear grid of
  their own (LdasinForcing(src=...), driver forcing_grid): double
  lat(src_south_north) and lon(src_west_east), optionally double HGT (the
  source's elevation) and int MASK (1 = valid) on (src_south_north,
  src_west_east) and double HGT_M(south_north, west_east), the model terrain
  (write_forcing_grid / read_forcing_grid).  The LDASIN files then carry their
  variables on (Time, src_south_north, src_west_east)-shaped grids.

Columns are the grid's land points (LANDMASK == 1) in row-major order.
"""
from __future__ import annotations

import datetime
import os

import numpy as np
from scipy.io import netcdf_file

from . import cases, layout as L, timeman

FILL = np.float32(-9999.0)
LDASIN_MAP = {"SFCTMP": "T2D", "Q2": "Q2D", "UU": "U2D", "VV": "V2D", "SFCPRS": "PSFC",
              "PSFC": "PSFC", "PRCP": "RAINRATE", "SOLDN": "SWDOWN", "LWDN": "LWDOWN"}
LDASIN_UNITS = {"T2D": "K", "Q2D": "kg kg-1", "U2D": "m s-1", "V2D": "m s-1", "PSFC": "Pa",
                "RAINRATE": "kg m-2 s-1", "SWDOWN": "W m-2", "LWDOWN": "W m-2",
                "COSZ": "1", "CO2AIR": "Pa", "O2AIR": "Pa"}
_LAYER_DIMS = {7: "snso_layers", 4: "soil_layers", 3: "snow_layers"}


def stamp(t: datetime.datetime) -> str:
    """HRLDAS file-time stamp YYYYMMDDHH; minutes are appended for off-hour
    times (input or output intervals below an hour)."""
    return t.strftime("%Y%m%d%H" if t.minute == 0 and t.second == 0 else "%Y%m%d%H%M")


def ldasin_path(indir: str, t: datetime.datetime) -> str:
    return os.path.join(indir, f"{stamp(t)}.LDASIN_DOMAIN1")


def ldasout_path(outdir: str, t: datetime.datetime) -> str:
    return os.path.join(outdir, f"{stamp(t)}.LDASOUT_DOMAIN1")


def _read(path: str):
    if not os.path.isfile(path):
        raise FileNotFoundError(path)
    return netcdf_file(path, "r", mmap=False)


# ---- grid -------------------------------------------------------------------------
class Grid:
    """Land points of a (south_north, west_east) grid, row-major."""

    def __init__(self, lat_deg: np.ndarray, lon_deg: np.ndarray, mask: np.ndarray):
        self.shape = tuple(mask.shape)
        self.lat_deg = np.asarray(lat_deg, np.float64)
        self.lon_deg = np.asarray(lon_deg, np.float64)
        self.mask = np.asarray(mask, bool)
        self.index = np.flatnonzero(self.mask.reshape(-1))

    @property
    def n(self) -> int:
        return int(self.index.size)

    def columns(self, field2d: np.ndarray) -> np.ndarray:
        return np.asarray(field2d).reshape(-1)[self.index]

    def scatter(self, cols: np.ndarray, fill=FILL) -> np.ndarray:
        out = np.full(self.shape[0] * self.shape[1], fill, np.asarray(cols).dtype)
        out[self.index] = cols
        return out.reshape(self.shape)

    @property
    def lat_rad(self) -> np.ndarray:
        return np.radians(self.columns(self.lat_deg))

    @property
    def lon_rad(self) -> np.ndarray:
        return np.radians(self.columns(self.lon_deg))


# ---- static file ----------------------------------------------------------------
def write_static(path: str, cols: cases.ColumnSet, grid: Grid, greenfrac=None):
    """A geo_em-style static file for `cols` laid on `grid` (tests / examples)."""
    ny, nx = grid.shape
    f = netcdf_file(path, "w")
    try:
        f.createDimension("south_north", ny)
        f.createDimension("west_east", nx)
        f.createDimension("month", 12)
        dims = ("south_north", "west_east")

        def put(name, data, kind="f4", units=None):
            v = f.createVariable(name, kind, dims)
            v[:] = data
            if units:
                v.units = units

        # f8 degrees: radians -> degrees -> radians returns the columns' f32 LAT exactly
        put("XLAT_M", grid.lat_deg, "f8", units="degrees_north")
        put("XLONG_M", grid.lon_deg, "f8", units="degrees_east")
        put("LANDMASK", grid.mask.astype(np.int32), "i4")
        sf, si = cols.static_f, cols.static_i
        for name, row in (("LU_INDEX", "VEGTYP"), ("SCT_DOM", "SOILTYP"), ("SLOPECAT", "SLOPETYP"),
                          ("SOILCOLOR", "SOILCOLOR")):
            put(name, grid.scatter(si[L.STATIC_I.index(row)].astype(np.int32), 0), "i4")
        put("SOILTEMP", grid.scatter(sf[L.STATIC_F.index("TBOT")]), units="K")
        put("ZLVL", grid.scatter(sf[L.STATIC_F.index("ZLVL")]), units="m")
        put("FOLN", grid.scatter(sf[L.STATIC_F.index("FOLN")]))
        if greenfrac is None:  # constant in time: the columns' SHDFAC every month
            greenfrac = np.repeat(sf[L.STATIC_F.index("SHDFAC")][None, :], 12, 0)
        put("SHDMAX", grid.scatter(sf[L.STATIC_F.index("SHDMAX")]))
        v = f.createVariable("GREENFRAC", "f4", ("month",) + dims)
        v[:] = np.stack([grid.scatter(np.asarray(g, np.float32)) for g in greenfrac])
    finally:
        f.close()


def read_static(path: str, params: dict, when: datetime.datetime):
    """(Grid, static_f (6, n) f32, static_i (6, n) i32) of a static file.
    SHDFAC is GREENFRAC interpolated to `when` (mid-month weights), SHDMAX its
    annual maximum; IST = 2 on the table's water type, ICE = 1 on its ice type."""
    f = _read(path)
    try:
        v = f.variables
        lat, lon = np.array(v["XLAT_M"][:]), np.array(v["XLONG_M"][:])
        mask = np.array(v["LANDMASK"][:]) == 1 if "LANDMASK" in v else np.ones(lat.shape, bool)
        grid = Grid(lat, lon, mask)
        n = grid.n
        col = lambda name, default: (grid.columns(np.array(v[name][:])) if name in v  # noqa: E731
                                     else np.full(n, default))
        lut = col("LU_INDEX", 7).astype(np.int32)
        slt = col("SCT_DOM", 6).astype(np.int32)
        gf = np.array(v["GREENFRAC"][:]) if "GREENFRAC" in v else None
        sf = np.zeros((L.NSTATIC_F, n), np.float32)
        si = np.zeros((L.NSTATIC_I, n), np.int32)
        sf[L.STATIC_F.index("LAT")] = np.radians(grid.columns(lat))
        sf[L.STATIC_F.index("ZLVL")] = col("ZLVL", 10.0)
        sf[L.STATIC_F.index("TBOT")] = col("SOILTEMP", 285.0)
        sf[L.STATIC_F.index("FOLN")] = col("FOLN", 1.0)
        if gf is not None:
            g = np.stack([grid.columns(gf[m]) for m in range(12)])
            sf[L.STATIC_F.index("SHDFAC")] = _month_weighted(g, when)
            sf[L.STATIC_F.index("SHDMAX")] = col("SHDMAX", 0.0) if "SHDMAX" in v else g.max(0)
        else:
            sf[L.STATIC_F.index("SHDFAC")] = 0.7
            sf[L.STATIC_F.index("SHDMAX")] = 0.8
        si[L.STATIC_I.index("VEGTYP")] = lut
        si[L.STATIC_I.index("SOILTYP")] = slt
        si[L.STATIC_I.index("SLOPETYP")] = col("SLOPECAT", 1)
        si[L.STATIC_I.index("SOILCOLOR")] = col("SOILCOLOR", 4)
        si[L.STATIC_I.index("IST")] = np.where(lut == params["iswater"], 2, 1)
        si[L.STATIC_I.index("ICE")] = np.where(lut == params["isice"], 1, 0)
        return grid, sf, si
    finally:
        f.close()


def read_greenfrac(path: str, grid: Grid):
    """The static file's 12 monthly GREENFRAC grids as a (12, n) float32 table
    of the grid's land points, in land-point order (the rows read_static
    interpolates SHDFAC from; vegclim.shdfac_host forms the row for any date),
    or None when the file has no GREENFRAC."""
    f = _read(path)
    try:
        if "GREENFRAC" not in f.variables:
            return None
        gf = np.array(f.variables["GREENFRAC"][:])
        return np.stack([grid.columns(gf[m]) for m in range(12)]).astype(np.float32)
    finally:
        f.close()


def _month_weighted(g12: np.ndarray, when: datetime.datetime) -> np.ndarray:
    """Linear interpolation between mid-month values (a monthly climatology at `when`)."""
    ylen = timeman.yearlen(when.year)
    t = 12.0 * timeman.julian(when) / ylen - 0.5
    m0 = int(np.floor(t)) % 12
    w = t - np.floor(t)
    return ((1.0 - w) * g12[m0] + w * g12[(m0 + 1) % 12]).astype(np.float32)


# ---- state (initialization / restart) ----------------------------------------------
def write_state(path: str, grid: Grid, state: np.ndarray, isnow: np.ndarray,
                t: datetime.datetime, step: int = 0, accum=None, extremes=None, intstats=None):
    """SoA state (56, n) + ISNOW on the grid; layer fields get a layer dimension.
    accum: (acc (NACC, n) float64, stor_beg (n,), steps) of an accumulating run
    part way through an output interval (driver.OfflineDriver(accumulate=True)),
    stored as double variables ACC_<name> (layout.ACC) and STOR_BEG and the
    global attribute accum_steps; read_accum reads them, read_state ignores
    them.
    extremes: (val (2*nseries, n), when (2*nseries, n) int32, steps, spec) of a
    run that tracks interval extremes (driver.OfflineDriver(extremes=...)),
    stored as variables EXT_<NAME>_MAX / _MIN in val's precision, EXTW_<NAME>_MAX
    / _MIN (int) and the global attributes extremes_steps and extremes_spec;
    read_extremes reads them, read_state ignores them.
    intstats: (acc (nitems, n) float64, cnt (3*nitems, n) int32, steps, spec) of
    a run that keeps interval statistics (driver.OfflineDriver(interval_stats=
    ...)), stored as double variables IST_<LABEL>_SUM, int variables
    IST_<LABEL>_COUNT / _RUN / _LONGEST and the global attributes intstats_steps
    and intstats_spec; read_intstats reads them, read_state ignores them."""
    ny, nx = grid.shape
    f = netcdf_file(path, "w")
    try:
        f.createDimension("south_north", ny)
        f.createDimension("west_east", nx)
        for w, d in _LAYER_DIMS.items():
            f.createDimension(d, w)
        f.model_time = t.isoformat()
        f.model_step = np.int32(step)
        f.state_layout = ",".join(n for n, _ in L.STATE_FIELDS)
        dims = ("south_north", "west_east")
        kind = "f8" if state.dtype == np.float64 else "f4"
        for name, w in L.STATE_FIELDS:
            o = L.STATE_OFF[name][0]
            if w == 1:
                v = f.createVariable(name, kind, dims)
                v[:] = grid.scatter(state[o].astype(kind), np.asarray(FILL, kind))
            else:
                v = f.createVariable(name, kind, (_LAYER_DIMS[w],) + dims)
                v[:] = np.stack([grid.scatter(state[o + k].astype(kind), np.asarray(FILL, kind))
                                 for k in range(w)])
        v = f.createVariable("ISNOW", "i4", dims)
        v[:] = grid.scatter(isnow.astype(np.int32), 0)
        if accum is not None:
            acc, stor_beg, nacc = accum
            assert acc.shape == (L.NACC, grid.n) and stor_beg.shape == (grid.n,)
            f.accum_steps = np.int32(nacc)
            fill = np.float64(FILL)
            for name, row in zip(L.ACC, acc):
                v = f.createVariable(f"ACC_{name}", "f8", dims)
                v[:] = grid.scatter(row.astype(np.float64), fill)
            v = f.createVariable("STOR_BEG", "f8", dims)
            v[:] = grid.scatter(stor_beg.astype(np.float64), fill)
        if extremes is not None:
            val, when, nsteps, spec = extremes
            names = _extremes_names(spec)
            assert val.shape == when.shape == (len(names), grid.n), (val.shape, when.shape)
            f.extremes_steps = np.int32(nsteps)
            f.extremes_spec = str(spec)
            xkind = "f8" if val.dtype == np.float64 else "f4"
            for name, vrow, wrow in zip(names, val, when):
                v = f.createVariable(f"EXT_{name}", xkind, dims)
                v[:] = grid.scatter(vrow, np.asarray(FILL, xkind))
                v = f.createVariable(f"EXTW_{name}", "i4", dims)
                v[:] = grid.scatter(wrow.astype(np.int32), 0)
        if intstats is not None:
            acc, cnt, nsteps, spec = intstats
            labels = _intstats_labels(spec)
            assert acc.shape == (len(labels), grid.n) and cnt.shape == (3 * len(labels), grid.n), \
                (acc.shape, cnt.shape)
            f.intstats_steps = np.int32(nsteps)
            f.intstats_spec = str(spec)
            for i, label in enumerate(labels):
                v = f.createVariable(f"IST_{label}_SUM", "f8", dims)
                v[:] = grid.scatter(acc[i].astype(np.float64), np.float64(FILL))
                for j, what in enumerate(_IST_COUNTERS):
                    v = f.createVariable(f"IST_{label}_{what}", "i4", dims)
                    v[:] = grid.scatter(cnt[3 * i + j].astype(np.int32), 0)
    finally:
        f.close()


def _extremes_names(spec: str) -> list:
    """<NAME>_MAX, <NAME>_MIN of every series of the spec: the rows of a run's
    running extremes (val and when, row 2s the maximum of series s)."""
    from . import extremes as X
    return [f"{s.name}_{m}" for s in X.parse(spec) for m in ("MAX", "MIN")]


def read_extremes(path: str, grid: Grid):
    """(val (2*nseries, n), when (2*nseries, n) int32, steps, spec) of a state
    file write_state stored a run's interval extremes in, or None when the file
    carries none (an initialization file, a run without the option)."""
    f = _read(path)
    try:
        if not hasattr(f, "extremes_steps") or not hasattr(f, "extremes_spec"):
            return None
        spec = f.extremes_spec.decode() if isinstance(f.extremes_spec, bytes) else f.extremes_spec
        names = _extremes_names(spec)
        val = np.stack([grid.columns(np.array(f.variables[f"EXT_{n}"][:])) for n in names])
        when = np.stack([grid.columns(np.array(f.variables[f"EXTW_{n}"][:])) for n in names])
        return val, when.astype(np.int32), int(f.extremes_steps), str(spec)
    finally:
        f.close()


# the three counter rows of an interval-statistics item, in row order
_IST_COUNTERS = ("COUNT", "RUN", "LONGEST")


def _intstats_labels(spec: str) -> list:
    """The labels of the spec's items: the rows of a run's running sums (and,
    three to an item, of its counters)."""
    from . import intstats as IS
    return [it.label for it in IS.parse(spec)]


def read_intstats(path: str, grid: Grid):
    """(acc (nitems, n) float64, cnt (3*nitems, n) int32, steps, spec) of a
    state file write_state stored a run's interval statistics in, or None when
    the file carries none (an initialization file, a run without the option)."""
    f = _read(path)
    try:
        if not hasattr(f, "intstats_steps") or not hasattr(f, "intstats_spec"):
            return None
        spec = f.intstats_spec.decode() if isinstance(f.intstats_spec, bytes) else f.intstats_spec
        labels = _intstats_labels(spec)
        acc = np.stack([grid.columns(np.array(f.variables[f"IST_{n}_SUM"][:])) for n in labels])
        cnt = np.stack([grid.columns(np.array(f.variables[f"IST_{n}_{w}"][:]))
                        for n in labels for w in _IST_COUNTERS])
        return acc.astype(np.float64), cnt.astype(np.int32), int(f.intstats_steps), str(spec)
    finally:
        f.close()


def read_state(path: str, grid: Grid, dtype=np.float32):
    """(state (56, n), isnow (n,), time, step) from a state file on `grid`."""
    f = _read(path)
    try:
        layout = f.state_layout.decode() if isinstance(f.state_layout, bytes) else f.state_layout
        assert layout == ",".join(n for n, _ in L.STATE_FIELDS), "state layout"
        st = np.zeros((L.NSTATE, grid.n), dtype)
        for name, w in L.STATE_FIELDS:
            o = L.STATE_OFF[name][0]
            a = np.array(f.variables[name][:])
            if w == 1:
                st[o] = grid.columns(a)
            else:
                for k in range(w):
                    st[o + k] = grid.columns(a[k])
        isnow = grid.columns(np.array(f.variables["ISNOW"][:])).astype(np.int32)
        mt = f.model_time.decode() if isinstance(f.model_time, bytes) else f.model_time
        return st, isnow, datetime.datetime.fromisoformat(mt), int(f.model_step)
    finally:
        f.close()


def read_accum(path: str, grid: Grid):
    """(acc (NACC, n) float64, stor_beg (n,) float64, steps) of a state file
    write_state stored an accumulating run's interval in, or None when the
    file carries none (an initialization file, a run without accumulation)."""
    f = _read(path)
    try:
        if "STOR_BEG" not in f.variables or not hasattr(f, "accum_steps"):
            return None
        acc = np.stack([grid.columns(np.array(f.variables[f"ACC_{name}"][:], np.float64))
                        for name in L.ACC])
        stor = grid.columns(np.array(f.variables["STOR_BEG"][:], np.float64))
        return acc, stor, int(f.accum_steps)
    finally:
        f.close()


# ---- forcing grid (LDASIN files on their own, coarser grid) -----------------------
class ForcingGrid:
    """The rectilinear grid a run's LDASIN files are stored on when it is not
    the model grid: lat (ny,) and lon (nx,) degrees, and optionally hgt
    (ny, nx) the source's elevation in m, mask (ny, nx) bool (true = a valid
    source point) and hgt_m, the model terrain on the run's own grid."""

    def __init__(self, lat, lon, hgt=None, mask=None, hgt_m=None):
        self.lat = np.asarray(lat, np.float64)
        self.lon = np.asarray(lon, np.float64)
        self.shape = (int(self.lat.size), int(self.lon.size))
        self.hgt = None if hgt is None else np.asarray(hgt, np.float64).reshape(self.shape)
        self.mask = None if mask is None else np.asarray(mask).reshape(self.shape) == 1
        self.hgt_m = None if hgt_m is None else np.asarray(hgt_m, np.float64)

    @property
    def npts(self) -> int:
        return self.shape[0] * self.shape[1]

    def as_grid(self) -> Grid:
        """The source points as a Grid (every point a 'land point'), for
        write_ldasin of a file on this grid."""
        lat = self.lat[:, None] + 0.0 * self.lon[None, :]
        lon = self.lon[None, :] + 0.0 * self.lat[:, None]
        return Grid(lat, lon, np.ones(self.shape, bool))


def write_forcing_grid(path: str, fg: ForcingGrid):
    """A forcing-grid file: double lat(src_south_north), lon(src_west_east),
    optional double HGT and int MASK (1 = valid) on (src_south_north,
    src_west_east), optional double HGT_M(south_north, west_east)."""
    f = netcdf_file(path, "w")
    try:
        f.createDimension("src_south_north", fg.shape[0])
        f.createDimension("src_west_east", fg.shape[1])
        v = f.createVariable("lat", "f8", ("src_south_north",))
        v[:] = fg.lat
        v.units = "degrees_north"
        v = f.createVariable("lon", "f8", ("src_west_east",))
        v[:] = fg.lon
        v.units = "degrees_east"
        dims = ("src_south_north", "src_west_east")
        if fg.hgt is not None:
            v = f.createVariable("HGT", "f8", dims)
            v[:] = fg.hgt
            v.units = "m"
        if fg.mask is not None:
            v = f.createVariable("MASK", "i4", dims)
            v[:] = fg.mask.astype(np.int32)
        if fg.hgt_m is not None:
            if fg.hgt_m.ndim != 2:
                raise ValueError("hgt_m must be on the run's (south_north, west_east) grid")
            f.createDimension("south_north", fg.hgt_m.shape[0])
            f.createDimension("west_east", fg.hgt_m.shape[1])
            v = f.createVariable("HGT_M", "f8", ("south_north", "west_east"))
            v[:] = fg.hgt_m
            v.units = "m"
    finally:
        f.close()


def read_forcing_grid(path: str) -> ForcingGrid:
    f = _read(path)
    try:
        v = f.variables
        for k in ("lat", "lon"):
            if k not in v:
                raise ValueError(f"{path}: no {k} variable")
        opt = lambda k: np.array(v[k][:]) if k in v else None  # noqa: E731
        return ForcingGrid(np.array(v["lat"][:]), np.array(v["lon"][:]), opt("HGT"), opt("MASK"),
                           opt("HGT_M"))
    finally:
        f.close()


# ---- LDASIN ---------------------------------------------------------------------
def write_ldasin(path: str, grid: Grid, forcing: np.ndarray, t: datetime.datetime,
                 extras=True):
    """One LDASIN file from a (12, n) forcing slice; `extras` (True, or a
    tuple of some of "COSZ", "CO2AIR", "O2AIR") also stores those fields, so
    that with all three the file reproduces the slice exactly."""
    ny, nx = grid.shape
    f = netcdf_file(path, "w")
    try:
        f.createDimension("Time", None)
        f.createDimension("south_north", ny)
        f.createDimension("west_east", nx)
        f.valid_time = t.isoformat()
        dims = ("Time", "south_north", "west_east")
        names = dict(LDASIN_MAP)
        names.pop("SFCPRS")  # SFCPRS and PSFC share the PSFC variable
        for x in (("COSZ", "CO2AIR", "O2AIR") if extras is True else (extras or ())):
            names[x] = x
        for fld, var in names.items():
            v = f.createVariable(var, "f4", dims)
            v[0] = grid.scatter(forcing[L.FORCING.index(fld)].astype(np.float32))
            v.units = LDASIN_UNITS[var]
    finally:
        f.close()


def read_ldasin(path: str) -> dict:
    f = _read(path)
    try:
        return {k: np.array(v[0] if v.dimensions[0] == "Time" else v[:])
                for k, v in f.variables.items()}
    finally:
        f.close()


class LdasinForcing:
    """Forcing provider for driver.OfflineDriver from LDASIN files: the file of
    the latest input time <= the step's start time (input_frequency, counted
    from the run's start), held constant over the input interval.

    Two forms: `__call__` gives the 12 noahmp_sflx forcing fields built on the
    host; `raw` gives the LDASIN block as the files carry it (the 8 variables
    plus the step's COSZ, fp32, layout.LDASIN order), from which the engine
    forms the other fields on the device (nmp_forcing_from_ldasin) -- a third
    fewer bytes to build and upload per step, the same values.

    Both are filled by `threads` host threads over column chunks (numpy
    releases the GIL in its elementwise loops); every element is computed by
    the same expression as in one pass, so the values do not depend on it.
    COSZ, a double cosine per column and step, dominated the host's time."""

    def __init__(self, indir: str, grid: Grid, begin: datetime.datetime,
                 every: datetime.timedelta, cols: slice | None = None, threads: int | None = None,
                 src: "ForcingGrid | None" = None, nearest=()):
        """cols: the land points this rank steps, in engine order (a slice or an
        index array; default: all of them in grid order).  threads: host
        threads (default NMP_HOST_THREADS, else 8).
        src: the files are stored on this ForcingGrid instead of the model
        grid; every variable is then interpolated to this rank's columns by
        their bilinear plan (regrid.RegridPlan, `plan`), on the host in _load
        (apply_host) or on the device from grid_raw's bytes
        (nmp_ldasin_regrid) -- the same bits.  nearest: the LDASIN variables
        that take their nearest source point instead.  Without src every byte
        and code path is as before."""
        self.indir, self.grid, self.begin, self.every = indir, grid, begin, every
        self.cols = cols if cols is not None else slice(0, grid.n)
        self.src, self.plan, self.nearest_mask = src, None, 0
        self.nearest = tuple(v if isinstance(v, str) else L.LDASIN[int(v)] for v in nearest)
        # shape and size of the grid the files are stored on
        self.file_shape = tuple(grid.shape) if src is None else tuple(src.shape)
        self.npts = self.file_shape[0] * self.file_shape[1]
        if src is not None:
            from .regrid import RegridPlan, nearest_mask
            self.nearest_mask = nearest_mask(self.nearest)
            self.plan = RegridPlan.bilinear(src.lat, src.lon,
                                            grid.columns(grid.lat_deg)[self.cols],
                                            grid.columns(grid.lon_deg)[self.cols], src.mask)
        self._t, self._fields = None, None
        self.lat, self.lon = self.grid.lat_rad[self.cols], self.grid.lon_rad[self.cols]
        # the latitude factors of COSZ, once (timeman.cosz evaluates the same
        # numpy functions on the same values every step)
        self._sincos_lat = (np.sin(self.lat), np.cos(self.lat))
        # file grid point of each engine column: one gather per variable
        self._gidx = np.asarray(grid.index)[self.cols]
        self.threads = max(1, int(threads if threads is not None else
                                  os.environ.get("NMP_HOST_THREADS", 8)))
        # shared by the read-ahead thread (_load) and the caller (_chunks);
        # its threads start on first use
        from concurrent.futures import ThreadPoolExecutor
        self._pool = ThreadPoolExecutor(self.threads) if self.threads > 1 else None

    def input_time(self, t: datetime.datetime) -> datetime.datetime:
        k = (t - self.begin) // self.every
        return self.begin + k * self.every

    def _load(self, ti: datetime.datetime) -> dict:
        """This rank's columns of every variable of the input time's file, in
        engine order and native byte order: one gather per variable straight
        from the mapped file through the composite index (engine column ->
        grid point), the variables on the provider's threads.  The values are
        read_ldasin's, selected by grid.columns and then `cols`."""
        path = ldasin_path(self.indir, ti)
        if not os.path.isfile(path):
            raise FileNotFoundError(path)
        f = netcdf_file(path, "r", mmap=True)
        out = {}
        try:
            names = list(f.variables)

            def one(k):
                v = f.variables[k]
                s = np.asarray(v[0] if v.dimensions[0] == "Time" else v[:]).reshape(-1)
                if self.plan is not None:  # the source grid's values at the columns
                    if s.dtype.kind != "f" or s.dtype.itemsize != 4:
                        s = s.astype(np.float32)
                    out[k] = self.plan.apply_host(s, nearest=k in self.nearest)
                    return
                out[k] = s[self._gidx].astype(s.dtype.newbyteorder("="))
            self._map(one, names)
        finally:
            f.close()
        return out

    def _map(self, fn, items):
        """fn(item) for every item, on the provider's threads."""
        if self._pool is None or len(items) < 2:
            for x in items:
                fn(x)
            return
        for fut in [self._pool.submit(fn, x) for x in items]:
            fut.result()

    def fields(self, t: datetime.datetime) -> dict:
        """The LDASIN variables of the step starting at t (this rank's columns).
        The next input time's file is read ahead on a background thread while
        the steps of this one run (a missing next file only fails when a
        step needs it)."""
        ti = self.input_time(t)
        if ti != self._t:
            ahead = getattr(self, "_ahead", None)
            if ahead is not None and ahead[0] == ti:
                self._fields = ahead[1].result()
            else:
                self._fields = self._load(ti)
            self._t = ti
            if getattr(self, "_reader", None) is None:
                from concurrent.futures import ThreadPoolExecutor
                self._reader = ThreadPoolExecutor(1)
            nxt = ti + self.every
            self._ahead = (nxt, self._reader.submit(self._load, nxt))
        return self._fields

    def _chunks(self, fill):
        """fill(slice) over column chunks, on the provider's threads."""
        n = self.lat.shape[0]
        k = min(self.threads, max(1, n // 65536))
        sl = [slice(n * i // k, n * (i + 1) // k) for i in range(k)]
        self._map(fill, sl)

    def _cosz(self, fl: dict, t: datetime.datetime, c: slice) -> np.ndarray:
        if "COSZ" in fl:
            return fl["COSZ"][c]
        return timeman.cosz(self.lat[c], self.lon[c], timeman.julian(t), timeman.yearlen(t.year),
                            sincos_lat=(self._sincos_lat[0][c], self._sincos_lat[1][c]))

    def __call__(self, step: int, t: datetime.datetime, out: np.ndarray | None = None):
        fl = self.fields(t)
        f = np.empty((L.NFORCING, self.lat.shape[0]), np.float32) if out is None else out
        F = L.FORCING.index

        def fill(c):
            for fld, var in LDASIN_MAP.items():
                f[F(fld), c] = fl[var][c]
            # every field is an fp32 value (the LDASIN precision), also when
            # `out` is an fp64 engine's buffer
            psfc = fl["PSFC"][c].astype(np.float64)
            f32 = np.float32
            f[F("COSZ"), c] = np.asarray(self._cosz(fl, t, c)).astype(f32)
            f[F("CO2AIR"), c] = fl["CO2AIR"][c] if "CO2AIR" in fl else (395.0e-6 * psfc).astype(f32)
            f[F("O2AIR"), c] = fl["O2AIR"][c] if "O2AIR" in fl else (0.209 * psfc).astype(f32)
        self._chunks(fill)
        return f

    def raw(self, step: int, t: datetime.datetime, out: np.ndarray | None = None):
        """(NLDASIN, n) fp32 LDASIN block of the step starting at t, written
        into `out` when given (e.g. a pinned upload buffer); None when the file
        carries CO2AIR / O2AIR of its own (then only the 12-field form holds
        them)."""
        fl = self.fields(t)
        if "CO2AIR" in fl or "O2AIR" in fl:
            return None
        r = np.empty((L.NLDASIN, self.lat.shape[0]), np.float32) if out is None else out

        def fill(c):
            for i, var in enumerate(L.LDASIN):
                r[i, c] = self._cosz(fl, t, c) if var == "COSZ" else fl[var][c]
        self._chunks(fill)
        return r

    def block(self, t: datetime.datetime, out: np.ndarray | None = None):
        """The LDASIN block of the input interval holding t without the
        per-step COSZ: the 8 file variables (and the file's own COSZ when it
        carries one; else that row is left as it is), for a host that uploads
        them once per input interval and forms COSZ on the device
        (nmp_forcing_from_ldasin_geo with `geo`).  None when the file carries
        CO2AIR / O2AIR of its own."""
        fl = self.fields(t)
        if "CO2AIR" in fl or "O2AIR" in fl:
            return None
        r = np.empty((L.NLDASIN, self.lat.shape[0]), np.float32) if out is None else out
        rows = [(i, v) for i, v in enumerate(L.LDASIN) if v != "COSZ" or "COSZ" in fl]

        def fill(c):
            for i, var in rows:
                r[i, c] = fl[var][c]
        self._chunks(fill)
        return r

    def variables(self, t: datetime.datetime) -> frozenset:
        """The variable names of the input file of t (its header only, cached
        per input time)."""
        ti = self.input_time(t)
        cache = self.__dict__.setdefault("_vars_cache", {})
        if ti in cache:
            self._vars_t, (self._vars, self._ingestible) = ti, cache[ti]
        if getattr(self, "_vars_t", None) != ti:
            path = ldasin_path(self.indir, ti)
            if not os.path.isfile(path):
                raise FileNotFoundError(path)
            f = netcdf_file(path, "r", mmap=True)
            try:
                self._vars = frozenset(f.variables)
                # the device ingest takes the 8 variables as fp32 grids
                npts = self.npts
                self._ingestible = all(
                    k in f.variables and f.variables[k].data.dtype == np.dtype(">f4") and
                    f.variables[k].data.size in (npts, npts * f.variables[k].data.shape[0])
                    and f.variables[k].data.shape[-2:] == self.file_shape
                    for k in L.LDASIN[:-1])
            finally:
                f.close()
            self._vars_t = ti
            cache[ti] = (self._vars, self._ingestible)
            while len(cache) > 4:   # the current and next input times, a few back
                del cache[min(cache)]
        return self._vars

    def ingestible(self, t: datetime.datetime) -> bool:
        """The input file of t holds the 8 LDASIN variables as fp32 grids of
        the run's shape -- with `src`, of the source grid's (what grid_raw and
        nmp_ldasin_ingest / nmp_ldasin_regrid take)."""
        self.variables(t)
        return self._ingestible

    def point(self) -> np.ndarray:
        """int32 (n,): the file grid point (row-major index) of each engine
        column -- nmp_ldasin_ingest's `point`.  Files on their own grid
        (`src`) have `plan` in its place."""
        if self.plan is not None:
            raise ValueError("files on their own grid have no point per column: use plan")
        return self._gidx.astype(np.int32)

    def dz(self) -> np.ndarray:
        """float32 (n,): the model terrain at each engine column minus the
        source grid's elevation interpolated to it (plan.interp_scalar, in
        double) -- nmp_ldasin_downscale's dz.  Needs HGT and HGT_M."""
        if self.src is None or self.src.hgt is None or self.src.hgt_m is None:
            raise ValueError("downscaling needs a forcing grid with HGT and HGT_M")
        if tuple(self.src.hgt_m.shape) != tuple(self.grid.shape):
            raise ValueError(f"HGT_M is {self.src.hgt_m.shape}, the run's grid {self.grid.shape}")
        model = self.grid.columns(self.src.hgt_m)[self.cols]
        return (model - self.plan.interp_scalar(self.src.hgt)).astype(np.float32)

    def grid_raw(self, t: datetime.datetime, out: np.ndarray | None = None):
        """The input file's 8 LDASIN variables (layout.LDASIN order, COSZ
        excluded) as the file stores them: (8, npts) big-endian fp32 grids,
        copied byte for byte into `out` (any 4-byte dtype, e.g. a pinned
        upload buffer's int32 view), one variable per provider thread.  The
        engine selects this rank's columns, applies its order and the byte
        order on the device (nmp_ldasin_ingest)."""
        path = ldasin_path(self.indir, self.input_time(t))
        if not os.path.isfile(path):
            raise FileNotFoundError(path)
        npts = self.npts
        r = np.empty((L.NLDASIN - 1, npts), ">f4") if out is None else out
        assert r.shape == (L.NLDASIN - 1, npts) and r.dtype.itemsize == 4
        f = netcdf_file(path, "r", mmap=True)
        try:
            def one(i):
                v = f.variables[L.LDASIN[i]]
                s = np.asarray(v[0] if v.dimensions[0] == "Time" else v[:]).reshape(-1)
                assert s.dtype == np.dtype(">f4"), f"{L.LDASIN[i]}: {s.dtype}"
                r[i].view(">f4")[...] = s
            self._map(one, list(range(L.NLDASIN - 1)))
        finally:
            f.close()
        return r

    def file_cosz(self, t: datetime.datetime) -> bool:
        """The input file of t carries COSZ (then it, not the solar geometry, is the step's)."""
        return "COSZ" in self.variables(t)

    def geo(self) -> np.ndarray:
        """(3, n) float64 per column: sin lat, cos lat, lon (radians) -- the
        column factors of timeman.cosz, the same values it evaluates."""
        return np.stack([self._sincos_lat[0], self._sincos_lat[1],
                         np.asarray(self.lon, np.float64)])


# ---- LDASOUT ----------------------------------------------------------------------
def write_ldasout(path: str, grid: Grid, diag: np.ndarray, t: datetime.datetime,
                  cols: np.ndarray | None = None, pool=None, names=L.DIAG_OUT):
    """The 16 output fluxes (NMP_O_*, (16, n)) on the grid.  cols: column j of
    diag is land point cols[j] (an engine order; default: land-point order).
    pool: an executor that scatters the fields in parallel.  names: the
    variables' names, one per row of diag (an accumulating run's 35:
    layout.DIAG_OUT_ACC)."""
    assert diag.shape[0] == len(names)
    ny, nx = grid.shape
    kind = "f8" if diag.dtype == np.float64 else "f4"
    idx = np.asarray(grid.index) if cols is None else np.asarray(grid.index)[cols]
    # the fields scattered straight into the file's (big-endian) element type
    full = np.empty((len(names), ny * nx), np.dtype(kind).newbyteorder(">"))

    def one(i):
        full[i].fill(FILL)
        full[i][idx] = diag[i]
    if pool is None:
        for i in range(len(names)):
            one(i)
    else:
        for fut in [pool.submit(one, i) for i in range(len(names))]:
            fut.result()
    f = netcdf_file(path, "w")
    try:
        f.createDimension("Time", None)
        f.createDimension("south_north", ny)
        f.createDimension("west_east", nx)
        f.valid_time = t.isoformat()
        variables = _ldasout_variables(names)
        for d, w in _layer_dims(variables):
            f.createDimension(d, w)
        for name, i, w, ldim in variables:
            if ldim is None:
                v = f.createVariable(name, kind, ("Time", "south_north", "west_east"))
                v._FillValue = np.asarray(FILL, kind)
                v[0] = full[i].reshape(ny, nx)
            else:  # layer-major: the group's consecutive grids are the variable's bytes
                v = f.createVariable(name, kind, ("Time", ldim, "south_north", "west_east"))
                v._FillValue = np.asarray(FILL, kind)
                v[0] = full[i:i + w].reshape(w, ny, nx)
    finally:
        f.close()


def _ldasout_variables(names):
    """(variable, first row, rows, layer dimension or None) of an output
    block's row names: the rows NAME_1..NAME_w of a layered state-output group
    (stateout.row_names) are one variable over a layer dimension."""
    from .stateout import variables
    return variables(names)


def _layer_dims(variables):
    """(dimension, length) of the layer dimensions the variables use, in order
    of first use."""
    from .stateout import LAYER_DIMS
    out = []
    for _, _, _, ldim in variables:
        if ldim is not None and ldim not in [d for d, _ in out]:
            out.append((ldim, LAYER_DIMS[ldim]))
    return out


def _nc_name(s: str) -> bytes:
    b = s.encode("latin1")
    return np.array(len(b), ">i4").tobytes() + b + b"\x00" * (-len(b) % 4)


def ldasout_header(grid: Grid, kind: str, t: datetime.datetime, names=L.DIAG_OUT) -> bytes:
    """The netCDF-3 classic header write_ldasout's file has (one record of the
    16 flux variables, or of `names`, over (Time, south_north, west_east), the
    valid_time global attribute, each variable's _FillValue), built from the format's
    layout: magic, numrecs, dimension / attribute / variable lists, each
    variable's type, per-record size and data offset.  The rows NAME_1..NAME_w
    of a layered state-output group are one variable over a layer dimension
    (soil_layers_stag, snow_layers), declared only when such a group is
    present; without one the bytes are what they were."""
    ny, nx = grid.shape
    i4 = lambda v: np.array(v, ">i4").tobytes()  # noqa: E731
    item = np.dtype(kind).itemsize
    nc_type = {4: 5, 8: 6}[item]                 # NC_FLOAT, NC_DOUBLE
    fill = np.asarray(FILL, np.dtype(kind).newbyteorder(">")).tobytes()
    variables = _ldasout_variables(names)
    ldims = _layer_dims(variables)                # only with a layered state-output group
    h = [b"CDF\x01", i4(1), i4(10), i4(3 + len(ldims))]  # NC_DIMENSION
    for name, n in (("Time", 0), ("south_north", ny), ("west_east", nx), *ldims):
        h += [_nc_name(name), i4(n)]
    dimid = {d: 3 + k for k, (d, _) in enumerate(ldims)}
    vt = t.isoformat().encode("latin1")
    h += [i4(12), i4(1), _nc_name("valid_time"), i4(2), i4(len(vt)), vt,
          b"\x00" * (-len(vt) % 4)]               # NC_ATTRIBUTE, NC_CHAR
    h += [i4(11), i4(len(variables))]            # NC_VARIABLE
    metas, vsizes = [], []
    for name, _, w, ldim in variables:
        vsize = w * ny * nx * item
        vsize += -vsize % 4
        shape = [i4(3), i4(0), i4(1), i4(2)] if ldim is None else \
            [i4(4), i4(0), i4(dimid[ldim]), i4(1), i4(2)]
        metas.append([_nc_name(name), *shape, i4(12), i4(1),
                      _nc_name("_FillValue"), i4(nc_type), i4(1), fill, i4(nc_type), i4(vsize)])
        vsizes.append(vsize)
    size = sum(len(x) for x in h) + sum(sum(len(x) for x in m) + 4 for m in metas)
    if size + sum(vsizes) > 2**31 - 1:  # CDF-1 offsets are signed 32-bit
        raise ValueError(f"LDASOUT of {len(names)} {ny} x {nx} {kind} grids exceeds the classic "
                         "format's 2 GiB offsets")
    begin = size
    for m, vsize in zip(metas, vsizes):
        h += m + [i4(begin)]                     # begin (32-bit offsets, version 1)
        begin += vsize
    return b"".join(h)


def write_ldasout_grids(path: str, grid: Grid, grids_be: np.ndarray, t: datetime.datetime,
                        names=L.DIAG_OUT):
    """An LDASOUT file from the 16 fluxes (or the fields `names`) already on
    the file's grids in its byte order (nmp_ldasout_grid's output: (16, npts) big-endian fp32 or
    fp64, FILL off the land points): the header and the bytes, one write --
    the same file write_ldasout produces from the columns."""
    kind = {4: "f4", 8: "f8"}[grids_be.dtype.itemsize]
    ny, nx = grid.shape
    assert grids_be.shape == (len(names), ny * nx) and grids_be.flags.c_contiguous
    with open(path, "wb") as f:
        f.write(ldasout_header(grid, kind, t, names))
        f.write(memoryview(grids_be).cast("B"))


def read_ldasout(path: str, grid: Grid, names=L.DIAG_OUT) -> np.ndarray:
    """The rows `names` of an LDASOUT file as columns; NAME_<k> is layer k
    (from 1) of a layered state-output variable NAME."""
    raw = read_ldasin(path)
    rows = {}
    for name, i, w, ldim in _ldasout_variables(names):
        for k in range(w):
            rows[i + k] = grid.columns(raw[name] if ldim is None else raw[name][k])
    return np.stack([rows[i] for i in range(len(names))])


# ---- REGIONS (region-aggregated output) ------------------------------------------
def regions_path(outdir: str, t: datetime.datetime) -> str:
    return os.path.join(outdir, f"{stamp(t)}.REGIONS_DOMAIN1")


def write_region_map(path: str, grid: Grid, region: np.ndarray, area: np.ndarray | None = None):
    """A region file on the run's grid: int REGION(south_north, west_east)
    (< 0: in no region) and, when given, double AREA (the points' weights)."""
    ny, nx = grid.shape
    f = netcdf_file(path, "w")
    try:
        f.createDimension("south_north", ny)
        f.createDimension("west_east", nx)
        dims = ("south_north", "west_east")
        v = f.createVariable("REGION", "i4", dims)
        v[:] = np.asarray(region, np.int32).reshape(ny, nx)
        if area is not None:
            v = f.createVariable("AREA", "f8", dims)
            v[:] = np.asarray(area, np.float64).reshape(ny, nx)
    finally:
        f.close()


def read_region_map(path: str, grid: Grid):
    """(region (n,) int64, area (n,) float64 or None) of the grid's land points
    (land-point order) from a region file on `grid`.  Points off the land mask
    are no columns and so are in no region."""
    f = _read(path)
    try:
        v = f.variables
        if "REGION" not in v:
            raise ValueError(f"{path}: no REGION variable")
        reg = np.array(v["REGION"][:])
        if reg.shape != grid.shape:
            raise ValueError(f"{path}: REGION is {reg.shape}, the run's grid {grid.shape}")
        if reg.dtype.kind not in "iu":
            raise ValueError(f"{path}: REGION must be an integer variable, not {reg.dtype}")
        area = None
        if "AREA" in v:
            area = grid.columns(np.array(v["AREA"][:], np.float64))
        return grid.columns(reg).astype(np.int64), area
    finally:
        f.close()


def write_regions(path: str, region_id, ncolumns, weight, means: np.ndarray,
                  t: datetime.datetime, names=L.DIAG_OUT):
    """One output time's region means: dimension `region`, region_id (int),
    ncolumns (int), weight (double: the plan's wsum) and one double variable
    per output field (`names`, the rows of means (nfield, nregion)) holding the
    regions' weighted means; the LDASOUT file's valid_time attribute."""
    means = np.asarray(means, np.float64)
    nreg = int(np.asarray(region_id).size)
    assert means.shape == (len(names), nreg), (means.shape, len(names), nreg)
    f = netcdf_file(path, "w")
    try:
        f.createDimension("region", nreg)
        f.valid_time = t.isoformat()
        for name, kind, a in (("region_id", "i4", region_id), ("ncolumns", "i4", ncolumns),
                              ("weight", "f8", weight)):
            v = f.createVariable(name, kind, ("region",))
            v[:] = np.asarray(a).astype(kind)
        for name, row in zip(names, means):
            v = f.createVariable(name, "f8", ("region",))
            v[:] = row
    finally:
        f.close()


_REGION_META = ("region_id", "ncolumns", "weight")


def read_regions(path: str) -> dict:
    """A REGIONS file: region_id, ncolumns, weight, names (the fields in file
    order), means (nfield, nregion) float64 and time."""
    f = _read(path)
    try:
        names = [k for k in f.variables if k not in _REGION_META]
        vt = f.valid_time.decode() if isinstance(f.valid_time, bytes) else f.valid_time
        nreg = f.dimensions["region"]
        out = {k: np.array(f.variables[k][:]).astype(np.float64 if k == "weight" else np.int64)
               for k in _REGION_META}
        out["names"] = names
        out["means"] = (np.stack([np.array(f.variables[k][:], np.float64) for k in names])
                        if names else np.zeros((0, nreg)))
        out["time"] = datetime.datetime.fromisoformat(vt)
        return out
    finally:
        f.close()


def read_regions_series(outdir: str) -> dict:
    """A run's REGIONS files stacked in time order: times (list), names,
    region_id, ncolumns, weight and means (time, field, region)."""
    import glob
    files = sorted(glob.glob(os.path.join(outdir, "*.REGIONS_DOMAIN1")))
    if not files:
        raise FileNotFoundError(os.path.join(outdir, "*.REGIONS_DOMAIN1"))
    recs = sorted((read_regions(p) for p in files), key=lambda r: r["time"])
    first = recs[0]
    for r in recs[1:]:
        if r["names"] != first["names"] or not np.array_equal(r["region_id"], first["region_id"]):
            raise ValueError(f"{outdir}: the REGIONS files do not share fields and regions")
    return dict(times=[r["time"] for r in recs], names=first["names"],
                region_id=first["region_id"], ncolumns=first["ncolumns"],
                weight=first["weight"], means=np.stack([r["means"] for r in recs]))
