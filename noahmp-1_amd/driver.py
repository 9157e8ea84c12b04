"""Offline driver: the time loop behind run/main.py.

The reference's driver parses the namelist and stops (run/main.py:12-14;
offline/noahmp_config.py has no time loop, forcing reader or writer, SURVEY
8f).  `OfflineDriver` is that missing loop around the engine:

* steps begdatetime -> enddatetime by `timestep` (Config), calling
  `Engine.step` for every column each step; JULIAN / YEARLEN / COSZ are
  computed per step at the step's start time (timeman.py);
* forcing comes from a provider `forcing(step, t) -> (12, n)` array; the
  reference's LDASIN files are not in the repository, so `SyntheticForcing`
  (the seeded diurnal generator the tests and bench use) is the default;
  `forcing="device"` generates the synthetic forcing on the GPU instead
  (`DeviceSyntheticForcing`, nmp_forcing_synth);
* output steps (Config.output_frequency) write the 16 surface fluxes as
  ``<outdir>/<YYYYMMDDHH>.LDASOUT_DOMAIN1`` (netCDF-3 on the grid, ncio.py)
  when the columns come from a grid, else ``<outdir>/<YYYYMMDDHH>.LDASOUT.npz``;
  with ``accumulate=True`` each file also carries the interval's accumulated
  output (layout.BUDGET: means, totals and the water budget's closure, added up
  on the device after every step: nmp_accumulate / nmp_accum_finish);
  with ``state_out`` each file also carries the selected groups of the land
  state -- soil, snow and canopy fields (layout.STATE_OUT), formed on the
  device from the state the output step left (nmp_state_output);
  with ``extremes`` each file also carries the interval's extremes of the
  selected series -- their maximum, their minimum and the time each occurred
  (extremes.py), tracked on the device after every step (nmp_extremes_update /
  nmp_extremes_output);
  with ``interval_stats`` each file also carries the interval's means of the
  selected series and, for series with a condition, the time the condition
  held, its longest spell and the value-seconds beyond its threshold
  (intstats.py), added up on the device after every step (nmp_intstats_update /
  nmp_intstats_output);
  with ``veg_clim`` the vegetation fraction SHDFAC follows the static file's
  monthly GREENFRAC climatology through the run, re-formed on the device from
  the resident table (nmp_static_monthly; vegclim.py states the scheme) instead
  of staying at the run's first instant;
  with ``regions`` each output step also writes the regions' weighted means of
  every output field as ``<YYYYMMDDHH>.REGIONS_DOMAIN1`` (nmp_region_reduce on
  the output block, on rank 0; ``write_grids=False`` then drops the grids);
* restart steps (Config.restart_frequency, calendar months allowed) write the
  complete SoA state (``RESTART.<YYYYMMDDHH>_DOMAIN1.nc`` on a grid, else
  ``.npz``), which `load_restart` reads back -- the state SoA *is* the restart
  (SURVEY 8f item 2);
* `OfflineDriver.from_files` builds the run from the namelist's files: the
  static file (grid, types), the initialization file (state) and the LDASIN
  directory (forcing), all netCDF-3 (ncio.py).

Multi-rank: each rank drives its own column shard (shard.shard_range of the
land points; `from_files` reads only its slice); at output steps the
diagnostics are gathered to rank 0 (shard.DiagGather, dst=0, ragged shards
allowed), which writes them for the whole grid.

How the forcing reaches the GPU is feeds.py's (one feed per forcing path, chosen
by `feeds.feed_kind`); the output rows' producers, the `OutputBlock` that lays
them out and plans each step for them, and the files' `OutputWriter` are
output.py's.  `OfflineDriver` is the loop around them.

`phase_s` accumulates the host time of the loop's parts (file headers,
forcing, launch enqueue, output hand-off, the whole iteration), for the
offline-driver timing (tools/offline_timing.py).
"""
from __future__ import annotations

import datetime
import os
import time
from collections import defaultdict

import numpy as np
import torch
import torch.distributed as dist

from . import (cases, extremes as xtr, intstats as ist, layout as L, ncio, shard, stateout,
               timeman, vegclim)
from .config import Config
from .engine import ColumnState, Engine, StreamShards
from .feeds import (DeviceSyntheticForcing, ForcingUpload, HostFeed,  # noqa: F401  (re-exported)
                    SyntheticForcing, feed_kind, make_feed)
from .order import coherent_order
from .output import OutputBlock, OutputWriter, chain
from .params import Params
from .regions import area_weights, plan_from_args


def _stamp(t: datetime.datetime) -> str:
    return t.strftime("%Y%m%d%H")


def _is_boundary(t: datetime.datetime, t0: datetime.datetime, every) -> bool:
    if every is None:
        return False
    if isinstance(every, str):  # 'Nmonth': calendar month boundaries at 00:00 of day 1
        n = int(every[:-5])
        months = (t.year - t0.year) * 12 + (t.month - t0.month)
        return t.day == 1 and t.hour == 0 and t.minute == 0 and t.second == 0 and months % n == 0 \
            and t != t0
    return (t - t0) % every == datetime.timedelta(0)


def _shard_extent(n: int, dev) -> tuple[int, int, bool]:
    """(the ranks' column counts summed, this rank's first column among them,
    whether this rank writes the output) for a rank that holds n columns."""
    if not dist.is_initialized():
        return n, 0, True
    on_host = dist.get_backend() == "gloo"
    t = torch.tensor([n], dtype=torch.int64, device="cpu" if on_host else dev)
    dist.all_reduce(t)
    total = int(t.item())
    first = shard.shard_range(total, dist.get_rank(), dist.get_world_size())[0]
    return total, first, dist.get_rank() == 0


def region_columns(path: str, grid: ncio.Grid, perm: np.ndarray | None = None,
                   weights="area"):
    """(region id, weight) of every engine column from a region file on the
    run's grid (ncio.read_region_map): the grid's land points, laid out in the
    engine's column order `perm` (land point of each column; None = grid
    order) like every other per-column input.  A point off the land mask is no
    column; a column with REGION < 0 is in no region.  weights: "area" = the
    file's AREA if it has one, else cos(latitude) in double; "equal" = 1; an
    array = one weight per land point in grid order, taken as given."""
    reg, area = ncio.read_region_map(path, grid)
    if isinstance(weights, str):
        if weights == "area":
            w = area if area is not None else area_weights(grid.lat_rad)
        elif weights == "equal":
            w = np.ones(grid.n, np.float64)
        else:
            raise ValueError(f"region_weights must be 'area', 'equal' or an array, not {weights!r}")
    else:
        w = np.asarray(weights, np.float64)
        if w.shape != (grid.n,):
            raise ValueError(f"region weights must have shape ({grid.n},), not {w.shape}")
    if perm is None:
        return reg, w
    return reg[perm], w[perm]


class OfflineDriver:
    def __init__(self, cfg: Config, cols: cases.ColumnSet, device: int = 0,
                 params: Params | None = None, forcing=None, precision: int = 4,
                 math: str = "ref", zsoil=cases.CASE_NML_ZSOIL, write: bool = True,
                 streams: int = 2, grid: ncio.Grid | None = None, ldasin_upload: bool = True,
                 cosz: str = "device", ingest: bool = True, accumulate: bool = False,
                 regions=None, region_weights="area", write_grids: bool = True,
                 downscale: bool = False, lapse_rate: float = 0.0065, interp: bool = False,
                 hold=("RAINRATE",), sw_zenith: bool = True, cosz_floor: float = 0.05,
                 prefetch: bool = True, state_out=None, veg_clim: str | None = None,
                 greenfrac=None, extremes=None, interval_stats=None):
        """cols: this rank's columns (all of them on a single rank); under an
        initialised process group they must be the rank's shard_range block of
        the global column set.  ldasin_upload: with a provider that has
        `raw` (LDASIN files), upload the files' variables and form the forcing
        on the device (False: the 12-field host form, for comparison).
        cosz: with ldasin_upload, "device" forms COSZ on the device from the
        columns' geometry (the files' variables then go up once per input
        interval), "host" computes it on the host and uploads it every step.
        ingest: with cosz="device", upload each file's bytes as it stores them
        (its big-endian grids, ncio.LdasinForcing.grid_raw) and select, order
        and byte-swap this rank's columns on the device (nmp_ldasin_ingest)
        instead of on the host (ncio.LdasinForcing.block).
        accumulate: also write each output interval's accumulated output
        (layout.BUDGET: time means of the energy fluxes, totals of the water
        fluxes, the water storage's change and the budget's residual) after
        the output step's 16 fluxes -- 35 fields per file.  Every step then
        writes its fluxes (DIAG_OUT_LEVEL) and nmp_accumulate adds them up on
        the range's stream right after the step; output steps also close the
        interval there (nmp_water_storage, nmp_accum_finish).  Off (the
        default), every code path and output byte is as without it.
        regions: per-column int region ids in the order of `cols` (< 0: in no
        region); under a process group, of the global column set in global
        column order (rank 0 reduces the gathered block, so the sums' bytes do
        not depend on the world size).  Output steps then also write the
        regions' weighted means of every output field (REGIONS files,
        ncio.write_regions), reduced on the device from the output block
        (nmp_region_reduce).  region_weights: "area" = cos(latitude) of the
        columns in double (single rank), "equal" = 1, or an array like
        `regions`.  write_grids=False (only with regions) skips the LDASOUT
        grids, their copy and their file.  Without regions nothing changes.
        downscale: with a provider whose files lie on their own grid
        (ncio.LdasinForcing(src=...) with HGT and HGT_M), correct every
        resident LDASIN block on the device for the elevation difference
        between the model terrain and the source grid (nmp_ldasin_downscale,
        lapse_rate in K/m), on the upload stream right after the block is
        formed there or uploaded; needs ldasin_upload and cosz="device".
        interp: with LDASIN files as resident blocks, the steps between two
        input times take their forcing from both files (feeds.LdasinInterpFeed,
        nmp_forcing_from_ldasin_interp; tinterp.py states the scheme) instead
        of holding the earlier file's values: linear in time, except the
        variables named in `hold` (block 0's values; RAINRATE is an interval
        rate) and SWDOWN, which with sw_zenith follows the step's own COSZ
        through the end points' clearness ratios SWDOWN / max(COSZ, cosz_floor)
        (sw_zenith=False: linear like the others).  The last interval runs
        held when the file at its end does not exist (`interp_held`).
        prefetch=False forms every block at the step that first needs it
        instead of reading ahead.  Refused with cosz="host",
        ldasin_upload=False, a provider without files or device-synthetic
        forcing.  Off (the default), every code path and output byte is as
        without it.
        state_out: "all", a comma-separated string or an iterable of
        state-output group names (layout.STATE_OUT: soil moisture and
        temperature, the snow pack, canopy water, LAI, the water table, the
        water storage, the carbon pools, ...).  Output steps then also form
        those groups' rows from the state on each range's stream right after
        the step (nmp_state_output; after nmp_accum_finish when accumulating)
        and write them after the fluxes, a layered group as one variable over
        a layer dimension.  REGIONS files carry the fluxes and the groups that
        cannot hold the fill value.  Refused in a run that writes no output.
        None (the default): every code path and output byte is as without it.
        veg_clim: "daily" or "step": SHDFAC (row NMP_F_SHDFAC of static_f, the
        vegetated fraction of every column with opt_veg = 1; other opt_veg
        values do not read it) follows `greenfrac`, the (12, ncol) monthly
        climatology of this driver's own columns (ncio.read_greenfrac, in the
        order of `cols`), through the run: the table goes up once, and before a
        step whose instant -- the step's start with "step", 00:00 of its day
        with "daily" (vegclim.quantise) -- differs from the one the row was
        last formed for, each range forms its own columns of the row on its
        stream ahead of its step (nmp_static_monthly; vegclim.shdfac_host is
        the numpy form).  The row is a function of that instant alone: nothing
        travels in restarts, and load_restart, a jump in time and spinup()'s
        rewind re-form it.  Refused without a table or with one of another
        shape.  None (the default): no table, no hook, every code path and
        output byte is as without it.
        extremes: "T2M,TRAD:max,PRCP:max+tmax", or an iterable of names or
        (name, stats) pairs (extremes.parse: the output fluxes, the forcing
        rows, the single-row state fields and the soil layers SMC1..4,
        SH2O1..4, STC1..4; stats of max, min, tmax, tmin, default max+min).
        Every step then folds its values into the interval's running maxima and
        minima on each range's stream right after the step (nmp_extremes_update,
        after nmp_accumulate when accumulating), and output steps write the
        rows <NAME>_MAX, _MIN, _TMAX, _TMIN (nmp_extremes_output; times in
        seconds from the interval's start to the end of the step that set the
        extreme) after the fluxes and the budget rows and before the state
        rows.  With a series of the output fluxes every step writes its fluxes
        (DIAG_OUT_LEVEL; into the one scratch block that accumulation reads
        too); without one the steps between output steps stay at DIAG_NONE.
        REGIONS files carry the rows; restarts carry the interval so far
        (save_restart).  Refused in a run that writes no output.  None (the
        default): every code path and output byte is as without it.
        interval_stats: "T2M,FROST=T2M@lt273.15:dur+spell,GDD=SFCTMP@gt278.15:deg",
        or an iterable of such items (intstats.parse: the series of `extremes`;
        without a condition the interval's mean, with gt, ge, lt or le and a
        threshold, under a label, the time the condition held, its longest
        unbroken spell and the value-seconds beyond the threshold).  Every step
        then adds its values to the interval's running sums and counters on
        each range's stream right after the step (nmp_intstats_update, after
        accumulation's and extremes' calls), and output steps write the rows
        <LABEL>_MEAN, _DUR, _DEG, _SPELL (nmp_intstats_output) after the
        extremes rows and before the state rows.  The interval's step count is
        the driver's.  With an item of the output fluxes every step writes its
        fluxes into the one scratch block; without one the steps between output
        steps stay at DIAG_NONE.  REGIONS files carry the rows; restarts carry
        the interval so far.  Refused in a run that writes no output, and when
        a row name occurs twice in the run's output.  None (the default):
        nothing is allocated or enqueued, every code path and output byte is
        as without it."""
        # (a bad veg_clim or table is refused before any device work)
        self.veg_clim, gf_host = veg_clim, None
        if veg_clim is not None:
            vegclim.quantise(cfg.begdatetime, veg_clim)
            if greenfrac is None:
                raise ValueError("veg_clim needs greenfrac, the (12, ncol) monthly table")
            gf_host = vegclim.check_table(greenfrac, int(np.asarray(cols.isnow).shape[0]))
        self.state_mask = 0
        if state_out is not None:
            self.state_mask = stateout.parse_groups(state_out)
            if not write or cfg.output_interval is None:
                raise ValueError("state_out needs a run that writes output")
        ext_series = None
        if extremes is not None:
            ext_series = xtr.parse(extremes)
            if not write or cfg.output_interval is None:
                raise ValueError("extremes needs a run that writes output")
        stat_items = None
        if interval_stats is not None:
            stat_items = ist.parse(interval_stats)
            if not write or cfg.output_interval is None:
                raise ValueError("interval_stats needs a run that writes output")
        if not write_grids and regions is None:
            raise ValueError("write_grids=False needs regions: the run would write nothing")
        # (a bad cosz, downscale or interp is refused before any device work)
        kind = feed_kind(forcing, ldasin_upload, cosz, ingest, downscale, interp)
        iopts = None
        if interp:
            from . import tinterp
            tinterp.check_args(0.0, tinterp.hold_mask(hold), sw_zenith, cosz_floor)
            iopts = dict(ingest=ingest, hold=tuple(hold), sw_zenith=sw_zenith,
                         cosz_floor=cosz_floor, end=cfg.enddatetime, prefetch=prefetch)
        dz_host = forcing.dz() if downscale else None  # ValueError without HGT and HGT_M
        self.cfg, self.grid = cfg, grid
        # from_files: the land point of each column of the whole set, and of this rank's
        self.perm, self.cols_index = None, None
        self.engine = Engine(params or Params.builtin(), cfg.engine_options(), device, precision,
                             math)
        self.dtype = self.engine.dtype
        self.dev = torch.device("cuda", device)
        self.cs = ColumnState.from_host(cols, self.dev, self.dtype)
        # column ranges on their own streams: launch tails overlap (engine.StreamShards)
        self.ranges = StreamShards(self.engine, self.cs, streams)
        # veg_clim: the resident climatology, and the instant SHDFAC was last formed for
        self._veg_table, self._veg_key = None, None
        if gf_host is not None:
            self._veg_table = torch.as_tensor(gf_host, device=self.dev)
        total, first, rank0 = _shard_extent(self.cs.ncol, self.dev)
        if forcing == "device":
            # draws keyed by the global column index: the forcing of a column
            # does not depend on the world size
            forcing = DeviceSyntheticForcing(cases.climate(cols), seed=0, first_col=first)
        self.forcing = forcing or SyntheticForcing(cols)
        self.zsoil = [float(z) for z in zsoil]
        self.dt = cfg.timestep.total_seconds()
        self.t, self.step_index, self.write = cfg.begdatetime, 0, write
        # spin-up: where the run stands before its first step, the shard's place
        # among the ranks' columns, and the columns' latitudes (the mean's weights)
        self._start, self._first_col, self._total = (self.t, self.step_index), first, total
        self._lat = np.asarray(cols.static_f[L.STATIC_F.index("LAT")], np.float64)
        self.spinup_history, self.spinup_stop = [], None
        self._spin = None
        self.accumulate = bool(accumulate)
        # the output rows: their producers, layout and per-step plan (output.OutputBlock)
        block = self.block = OutputBlock(self.engine, self.cs, self.dt, self.accumulate,
                                         ext_series, self.state_mask, stat_items)
        self.out_names, self.diag = block.names, block.diag
        self.accum, self.extremes, self.intstats = block.accum, block.extremes, block.intstats
        nout = len(self.out_names)
        if nout > L.NDIAG_OUT and grid is not None:
            # a grid whose 35 fields or state rows do not pass the classic
            # format's offsets fails here, not on a writer thread after the
            # first interval
            ncio.ldasout_header(grid, "f4" if self.dtype == torch.float32 else "f8",
                                cfg.begdatetime, self.out_names)
        # the 12-field host form, which every run has, and the run's own path
        host = HostFeed(self.forcing, self.cs.ncol, self.dtype, self.dev, bool(downscale))
        feed = self.feed = make_feed(kind, host, self.engine, self.cs.ncol, self.dtype, self.dev,
                                     float(lapse_rate), dz_host, iopts)
        self.interp = bool(interp)
        self.upload, self.raw_upload, self.raw_fbuf = host.upload, feed.raw_upload, feed.raw_fbuf
        self.geo, self.ingest, self.point = feed.geo, feed.ingest, feed.point
        self.regrid_plan, self.dz = feed.regrid_plan, feed.dz
        self.downscale, self.lapse_rate = bool(downscale), float(lapse_rate)
        # single-rank output: grids and copies on a stream of their own, so the
        # next steps need not wait for them (only the next output step waits
        # for the diagnostics buffer to be read: _diag_free)
        self.out_stream, self._diag_free = None, None
        self.phase_s = defaultdict(float)
        self.gather = None
        if dist.is_initialized():
            self.gather = shard.DiagGather(nout, total, self.dtype, self.dev, dst=0)
            if self.gather.n_local != self.cs.ncol:
                raise ValueError(f"rank {dist.get_rank()} holds {self.cs.ncol} columns, its "
                                 f"shard_range block of {total} has {self.gather.n_local}")
        self.write_grids = bool(write_grids)
        self.region_plan = None
        if regions is not None and rank0:
            lat = cols.static_f[L.STATIC_F.index("LAT")] if total == cols.n else None
            self.region_plan = plan_from_args(regions, region_weights, total, lat).to(self.dev)
        # the output staging buffers up front, out of the time loop (OutputWriter)
        self.output = OutputWriter(self.engine, cfg, grid, block, total, self.dtype, self.dev,
                                   write and cfg.output_interval is not None and rank0,
                                   self.region_plan, self.write_grids)
        self.written, self.regions_written = self.output.written, self.output.regions_written
        self.n_out = 0

    @classmethod
    def from_files(cls, cfg: Config, device: int = 0, params: Params | None = None,
                   init: str | None = None, order: str | None = "lon-snow-type",
                   host_threads: int | None = None, forcing_grid: str | None = None,
                   nearest=(), regions=None, region_weights="area", veg_clim: str | None = None,
                   **kw) -> "OfflineDriver":
        """The run the namelist describes: static file (cfg.constfile), initial
        state (cfg.initfile, or `init`) and LDASIN forcing (cfg.indir every
        cfg.input_frequency), netCDF-3 files in the layouts of ncio.py.
        forcing_grid: the path of a forcing-grid file (ncio.read_forcing_grid):
        the LDASIN files are stored on that coarser rectilinear grid and are
        interpolated to the columns (bilinear; the variables named in `nearest`
        take their nearest source point) -- on the device from the files'
        bytes (nmp_ldasin_regrid) where a model-grid file would be ingested,
        else on the host, the same bits.  downscale, lapse_rate: see __init__;
        dz = the file's HGT_M at the column minus its HGT interpolated to it.

        order: the land points are laid out in the engine in this coherent
        order (order.coherent_order; None = grid order).  The permutation is
        applied when columns are read from the files and undone when they are
        written, so files always hold the grid.
        host_threads: threads that build each step's forcing on the host
        (ncio.LdasinForcing; default NMP_HOST_THREADS, else 8).
        regions: the path of a region file on the run's grid (int REGION,
        optional double AREA; region_columns); region_weights "area" then
        uses AREA if the file has it, else cos(latitude).
        veg_clim: see __init__; the table is the static file's GREENFRAC
        (ncio.read_greenfrac), laid out like every other per-column input:
        the coherent order and this rank's block."""
        P = params or Params.builtin()
        grid, sf, si = ncio.read_static(cfg.constfile, P.as_dict(), cfg.begdatetime)
        st, isn, t0, step = ncio.read_state(init or cfg.initfile, grid)
        perm = np.arange(grid.n) if order is None else coherent_order(grid.lon_rad, si, isn,
                                                                      order, band_deg=4.0)
        idx = perm
        if dist.is_initialized():  # this rank's block of the (ordered) land points
            s0, cnt = shard.shard_range(grid.n, dist.get_rank(), dist.get_world_size())
            idx = perm[s0:s0 + cnt]
        cols = cases.ColumnSet(sf[:, idx], si[:, idx], st[:, idx], isn[idx], grid.lon_rad[idx],
                               *([None] * 6))
        if veg_clim is not None:
            vegclim.quantise(cfg.begdatetime, veg_clim)
            gf = ncio.read_greenfrac(cfg.constfile, grid)
            if gf is None:
                raise ValueError(f"veg_clim needs GREENFRAC in the static file {cfg.constfile}")
            kw = dict(kw, veg_clim=veg_clim, greenfrac=gf[:, idx])
        fkw = {}
        if forcing_grid is not None:
            fkw = dict(src=ncio.read_forcing_grid(os.fspath(forcing_grid)), nearest=nearest)
        elif kw.get("downscale") or nearest:
            raise ValueError("downscale and nearest need forcing_grid")
        forcing = ncio.LdasinForcing(cfg.indir, grid, cfg.begdatetime, cfg.input_interval,
                                     cols=idx, threads=host_threads, **fkw)
        if regions is not None:
            # the whole (ordered) column set's ids and weights: rank 0 reduces
            # the gathered block
            regions, region_weights = region_columns(os.fspath(regions), grid, perm,
                                                     region_weights)
        drv = cls(cfg, cols, device, P, forcing, grid=grid, regions=regions,
                  region_weights=region_weights, **kw)
        drv.t, drv.step_index = t0, step
        drv._start = (t0, step)
        drv.perm, drv.cols_index, drv.output.perm = perm, idx, perm
        for p in drv.block.carried:  # an initialization file written part way through an interval
            p.restore(p.nc[1](init or cfg.initfile, grid), idx)
        return drv

    @property
    def interp_held(self) -> list:
        """The input times whose interval ran held although interp is on: the
        closing interval of a run without a file at its end (noted once each)."""
        return getattr(self.feed, "interp_held", [])

    def to_grid_order(self, a: np.ndarray) -> np.ndarray:
        """(..., n) columns of the whole set in engine order -> land-point order."""
        if self.perm is None:
            return a
        out = np.empty_like(a)
        out[..., self.perm] = a
        return out

    # ---- restart -----------------------------------------------------------------
    def save_restart(self, path: str):
        """The interval so far travels with the state (output.OutputBlock.carried;
        a producer's `npz` names its npz arrays, `nc` ncio.write_state's keyword):
        accumulation's accumulators, beginning storage and step count; the running
        extremes, the steps that set them, the interval's step count and the spec;
        the interval statistics' sums and counters, step count and spec."""
        self.ranges.join()
        carried = [(p, p.state()) for p in self.block.carried]
        if path.endswith(".nc"):
            kw = {p.nc[0]: tuple(self.to_grid_order(v) if isinstance(v, np.ndarray) else v
                                 for v in st) for p, st in carried}
            ncio.write_state(path, self.grid, self.to_grid_order(self.cs.state.cpu().numpy()),
                             self.to_grid_order(self.cs.isnow.cpu().numpy()), self.t,
                             self.step_index, **kw)
            return
        extra = {k: np.int64(v) if isinstance(v, int) else np.asarray(v)
                 for p, st in carried for k, v in zip(p.npz, st)}
        np.savez(path, **extra, time=np.array(self.t.isoformat()), step=np.int64(self.step_index),
                 state=self.cs.state.cpu().numpy(), isnow=self.cs.isnow.cpu().numpy(),
                 static_f=self.cs.static_f.cpu().numpy(), static_i=self.cs.static_i.cpu().numpy(),
                 status=self.cs.status.cpu().numpy(), zsoil=np.asarray(self.zsoil, np.float32),
                 layout=np.array(",".join(n for n, _ in L.STATE_FIELDS)))

    def load_restart(self, path: str):
        """With accumulation on, a restart that carries an interval's
        accumulation state (save_restart of an accumulating run) resumes that
        interval; one without it starts a fresh interval at this point: zero
        accumulators and the beginning storage formed from the loaded state,
        so the next output's totals and means cover the steps from here.
        With extremes on, likewise: a restart that carries an interval's
        extremes under this run's spec resumes it; one without them, or with
        another spec, starts a fresh interval here, so the next output's
        extremes cover the steps from here.  Interval statistics follow the
        same rule."""
        self.ranges.join()  # no range may still be stepping the state being replaced
        self.feed.reset()   # resident blocks and read-ahead belong to the old time
        self._veg_key = None  # veg_clim: SHDFAC is re-formed for the restart's time
        if path.endswith(".nc"):
            st, isn, self.t, self.step_index = ncio.read_state(path, self.grid,
                                                               self.cs.state.cpu().numpy().dtype)
            idx = slice(None) if self.cols_index is None else self.cols_index
            self.cs.state.copy_(torch.as_tensor(np.ascontiguousarray(st[:, idx]),
                                                device=self.dev))
            self.cs.isnow.copy_(torch.as_tensor(np.ascontiguousarray(isn[idx]), device=self.dev))
            for p in self.block.carried:
                p.restore(p.nc[1](path, self.grid), idx)
            self._start = (self.t, self.step_index)
            return
        with np.load(path, allow_pickle=False) as z:
            assert str(z["layout"]) == ",".join(n for n, _ in L.STATE_FIELDS), "state layout"
            for name in ("state", "isnow", "static_f", "static_i", "status"):
                getattr(self.cs, name).copy_(torch.as_tensor(z[name], device=self.dev))
            self.t = datetime.datetime.fromisoformat(str(z["time"]))
            self.step_index = int(z["step"])
            self.zsoil = [float(v) for v in z["zsoil"]]
            for p in self.block.carried:
                p.restore(tuple(z[k] for k in p.npz) if p.npz[0] in z.files else None)
        self._start = (self.t, self.step_index)

    # ---- time loop -----------------------------------------------------------------
    # the interpreter's thread switch interval while the loop runs: the file
    # reader and writer threads hand the GIL back within this instead of 5 ms
    SWITCH_INTERVAL_S = 0.0005

    def run(self, nsteps: int | None = None):
        import sys
        old = sys.getswitchinterval()
        sys.setswitchinterval(min(old, self.SWITCH_INTERVAL_S))
        try:
            return self._run(nsteps)
        finally:
            sys.setswitchinterval(old)

    def _run(self, nsteps: int | None = None):
        cfg, phase, clock = self.cfg, self.phase_s, time.perf_counter
        total = cfg.step_count() if nsteps is None else nsteps
        rank = dist.get_rank() if dist.is_initialized() else 0
        for _ in range(total):
            if self.t >= cfg.enddatetime:
                break
            t_iter = clock()
            t0 = self.t
            t1 = t0 + cfg.timestep
            out = _is_boundary(t1, cfg.begdatetime, cfg.output_interval) and self.write
            # the ranges wait for the caller's current stream (state set-up,
            # restart copies, the gather fence assemble() left there) and for
            # what the feed names: the upload of this step's buffer or block
            cur = torch.cuda.current_stream(self.dev)
            tp = clock()
            self.feed.read(t0)
            phase["read"] += clock() - tp
            tp = clock()
            f, pre, after, _, _ = self.feed.step(self.step_index, t0, cur)
            phase["forcing"] += clock() - tp
            tp = clock()
            diag, b = self.diag, None
            if out and self.gather is not None:
                b = self.n_out % len(self.gather.bufs)
                self.gather.release(b, self.ranges.streams)
                diag = self.gather.local(b)
            if out and self._diag_free is not None:
                after = after + (self._diag_free,)  # the output stream's last read of `diag`
            dstep, level, post = self.block.plan(f, diag, out)
            if self._veg_table is not None:
                pre = chain((self._veg_pre(t0), pre))
            self.ranges.step(f, self.zsoil, self.dt, timeman.julian(t0), timeman.yearlen(t0.year),
                             dstep, level, after=after, pre=pre, post=post)
            self.feed.launched(t0, self.ranges.producers)
            phase["launch"] += clock() - tp
            tp = clock()
            self.t, self.step_index = t1, self.step_index + 1
            if out:
                self._output_step(t1, b, rank)
            phase["output"] += clock() - tp
            if _is_boundary(t1, cfg.begdatetime, cfg.restart_interval) and self.write:
                os.makedirs(cfg.resdir, exist_ok=True)
                name = (f"RESTART.{_stamp(t1)}_DOMAIN1.nc" if self.grid is not None and
                        not dist.is_initialized() else f"RESTART.{_stamp(t1)}.r{rank}.npz")
                self.save_restart(os.path.join(cfg.resdir, name))
            phase["loop"] += clock() - t_iter
        self.ranges.join()
        torch.cuda.synchronize(self.dev)
        self.flush_output()
        return self

    def _veg_pre(self, t0: datetime.datetime):
        """What a step that starts at t0 with veg_clim puts ahead of the feed's
        `pre`: nothing while SHDFAC stands for the step's instant, else the
        range's columns of the row for that instant."""
        when = vegclim.quantise(t0, self.veg_clim)
        if when == self._veg_key:
            return None
        self._veg_key = when
        m0, m1, w = vegclim.month_weights(when)
        row = self.cs.static_f[L.STATIC_F.index("SHDFAC")]

        def pre(st, rng):
            self.engine.static_monthly(self._veg_table, m0, m1, w, row, stream=st, cols=rng)
        return pre

    def _output_step(self, t1: datetime.datetime, b, rank: int):
        """Hand the output step's block to the writer: the gathered one
        (buffer b) on the current stream, or -- single rank -- the run's own on
        the output stream, after this step and beside the next ones."""
        if self.gather is not None:
            self.gather.start(b, producers=self.ranges.producers)
            d = self.gather.assemble(b)
            self.n_out += 1
            ost = torch.cuda.current_stream(self.dev)
        else:
            if self.out_stream is None:
                self.out_stream = torch.cuda.Stream(self.dev)
            ost = self.out_stream
            self.ranges.join(ost)
            d = self.diag
        if rank == 0:
            os.makedirs(self.cfg.outdir, exist_ok=True)
            path = (ncio.ldasout_path(self.cfg.outdir, t1) if self.grid is not None else
                    os.path.join(self.cfg.outdir, f"{_stamp(t1)}.LDASOUT.npz"))
            freed = self.output.write(d, path, t1, ost)
            if self.gather is None:
                self._diag_free = freed

    def flush_output(self):
        """Wait until every output file issued so far is written (raises a
        writer's error)."""
        self.output.flush()

    # ---- spin-up -------------------------------------------------------------------
    def spinup(self, loops: int, tol=None, min_loops: int = 1, report: bool = True,
               drift_map: bool = False):
        """Bring the state to equilibrium with the forcing: run from where the
        driver stands to cfg.enddatetime up to `loops` times, each pass from
        the state the pass before left, writing nothing, and measure on the
        device how far the state at the end of each pass lies from the end of
        the pass before (nmp_state_drift per column range, nmp_drift_reduce
        once over the rank's block; spinup.py states both in numpy).  Only
        while the driver stands at the time it was constructed or loaded for
        (RuntimeError otherwise); after every pass, the last included, time
        and step index go back there, the feed forgets its resident blocks and
        an accumulating run starts a fresh interval from the spun-up state.
        The state, ISNOW and the status bits stay: `run()` afterwards is the
        production run from the spun-up state.

        tol: the groups' tolerances (spinup.parse_tol: "SOIL_M=0.001,SOIL_T=
        0.01", a dict or 7 numbers; a group not named never holds the loop up).
        The loop ends early once at least min_loops passes have run and no
        column's drift exceeds its group's tolerance.  None: every pass runs
        and the drift is only reported.  There are no default tolerances.
        Each pass appends a spinup.SpinupRecord to `spinup_history` (per group
        the largest drift, its global column, the weighted mean, the count of
        columns over the tolerance); `spinup_stop` says why the loop ended.
        The mean's weights are cos(latitude) of the columns in double
        (regions.area_weights), 1 where the latitudes are not finite.

        Under a process group every rank reduces its shard; the largest
        drift, its column as a global index and the count are combined
        exactly, so they and the stop decision are the same at any world
        size.  The mean adds the ranks' weighted sums and weights in rank
        order on the host: its last bits depend on the world size.

        report: rank 0 writes <outdir>/SPINUP.json (history, groups, units,
        tolerances, stop reason).  drift_map (a run on a grid, single rank):
        the last pass's 7 drift rows on the grid as
        <outdir>/SPINUP_DRIFT_DOMAIN1, variables DRIFT_<GROUP>."""
        from . import spinup as sp
        loops, min_loops = int(loops), int(min_loops)
        if loops < 1 or min_loops < 1:
            raise ValueError("spinup: loops and min_loops must be at least 1")
        if drift_map and (self.grid is None or dist.is_initialized()):
            raise ValueError("spinup: drift_map needs a run on a grid, on a single rank")
        if (self.t, self.step_index) != self._start:
            raise RuntimeError("spinup: the run has moved on from the time it was constructed "
                               f"or loaded for ({self._start[0].isoformat()})")
        if self.t >= self.cfg.enddatetime:
            raise ValueError("spinup: no step lies between the start and enddatetime")
        tol_arr = np.full(L.NDRIFT, np.inf) if tol is None else sp.parse_tol(tol)
        n = self.cs.ncol
        if self._spin is None:
            w = area_weights(self._lat) if np.isfinite(self._lat).all() else np.ones(n)
            self._spin = dict(
                weight=torch.as_tensor(np.ascontiguousarray(w, np.float64), device=self.dev),
                snap=torch.zeros((L.NTRACKED, n), dtype=self.dtype, device=self.dev),
                drift=torch.zeros((L.NDRIFT, n), dtype=self.dtype, device=self.dev))
        snap, drift, weight = self._spin["snap"], self._spin["drift"], self._spin["weight"]
        self._drift_pass(snap, None)
        write, self.write = self.write, False   # no LDASOUT, REGIONS or RESTART file
        self.spinup_stop = f"ran all {loops} loops"
        try:
            for k in range(1, loops + 1):
                self.run()
                self._drift_pass(snap, drift)
                res = self.engine.drift_reduce(drift, tol_arr, weight)
                rec = self._spinup_record(k, res, tol_arr)
                self.spinup_history.append(rec)
                self._rewind()
                if tol is not None and k >= min_loops and rec.converged:
                    self.spinup_stop = f"converged after loop {k}"
                    break
        finally:
            self.write = write
        rank0 = not dist.is_initialized() or dist.get_rank() == 0
        if report and rank0:
            import json
            os.makedirs(self.cfg.outdir, exist_ok=True)
            with open(os.path.join(self.cfg.outdir, "SPINUP.json"), "w") as f:
                json.dump({"groups": list(L.DRIFT_GROUPS),
                           "units": [L.DRIFT_UNITS[g] for g in L.DRIFT_GROUPS],
                           "tol": sp.SpinupRecord(0, tol=tol_arr.tolist()).as_json()["tol"],
                           "min_loops": min_loops, "loops": loops, "stop": self.spinup_stop,
                           "start": self._start[0].isoformat(),
                           "end": self.cfg.enddatetime.isoformat(),
                           "history": [r.as_json() for r in self.spinup_history]}, f, indent=1)
        if drift_map:
            self._write_drift_map(drift)
        return self

    def _drift_pass(self, snap: torch.Tensor, drift):
        """nmp_state_drift for every column range on its stream, after the
        caller's stream; then the caller's stream waits for the ranges."""
        cur = torch.cuda.current_stream(self.dev)
        for st, rng in zip(self.ranges.streams, self.ranges.ranges):
            st.wait_stream(cur)
            self.engine.state_drift(self.cs, snap, drift, stream=st, cols=rng)
        self.ranges.join()

    def _rewind(self):
        """Back to the run's start with the state as it is."""
        self.ranges.join()
        self.t, self.step_index = self._start
        self.feed.reset()   # resident blocks and read-ahead belong to the old time
        for p in self.block.carried:
            p.restore(None)

    def _spinup_record(self, k: int, res, tol_arr):
        """The loop's record from this rank's reduction; under a process group
        from every rank's, combined as spinup() documents."""
        from . import spinup as sp
        mx, arg, count = res.max.copy(), res.arg.copy(), res.count.copy()
        arg[arg >= 0] += self._first_col
        wsum, wtot = res.wsum.copy(), np.float64(res.wtot)
        if dist.is_initialized():
            on_host = dist.get_backend() == "gloo"
            words = np.concatenate([mx.view(np.int64), arg, wsum.view(np.int64), count,
                                    np.array([wtot]).view(np.int64)])
            mine = torch.as_tensor(words, device="cpu" if on_host else self.dev)
            every = [torch.empty_like(mine) for _ in range(dist.get_world_size())]
            dist.all_gather(every, mine)
            g = L.NDRIFT
            parts = [e.cpu().numpy() for e in every]
            mx, arg = np.zeros(g), np.full(g, -1, np.int64)
            count, wsum, wtot = np.zeros(g, np.int64), np.zeros(g), np.float64(0.0)
            for p in parts:                         # rank order
                pm, pa = p[:g].view(np.float64), p[g:2 * g]
                for i in range(g):
                    if pa[i] < 0:
                        continue
                    n1, n2 = np.isnan(mx[i]), np.isnan(pm[i])
                    if arg[i] < 0 or (n2 and not n1) or (not n1 and not n2 and pm[i] > mx[i]) \
                            or (n1 == n2 and (n1 or pm[i] == mx[i]) and pa[i] < arg[i]):
                        mx[i], arg[i] = pm[i], pa[i]
                count = count + p[3 * g:4 * g]
                wsum = wsum + p[2 * g:3 * g].view(np.float64)
                wtot = wtot + p[4 * g:].view(np.float64)[0]
        with np.errstate(all="ignore"):
            mean = wsum / wtot
        return sp.SpinupRecord(k, mx.tolist(), [int(a) for a in arg], mean.tolist(),
                               [int(c) for c in count], tol_arr.tolist())

    def _write_drift_map(self, drift: torch.Tensor):
        """The drift rows on the grid (nmp_ldasout_grid) under the LDASOUT
        header, stamped with the run's start time."""
        npts = self.grid.shape[0] * self.grid.shape[1]
        f32 = self.dtype == torch.float32
        out = torch.empty((L.NDRIFT, npts), device=self.dev,
                          dtype=torch.int32 if f32 else torch.int64)
        self.engine.ldasout_grid(drift, self.output.point(), out, float(ncio.FILL))
        a = out.cpu().numpy()
        os.makedirs(self.cfg.outdir, exist_ok=True)
        ncio.write_ldasout_grids(os.path.join(self.cfg.outdir, "SPINUP_DRIFT_DOMAIN1"), self.grid,
                                 a.view(">f4" if f32 else ">f8"), self._start[0],
                                 [f"DRIFT_{g}" for g in L.DRIFT_GROUPS])
