#!/usr/bin/env python3
"""Offline Noah-MP run on the MI355X engine: counterpart of run/main.py.

    python noahmp_offline.py [case.nml] [--ncol N] [--kind casenml|mixed|conus]
                             [--device D] [--restart FILE] [--accumulate]
                             [--state-out all|NAME[,NAME...]]
                             [--regions FILE [--region-weights area|equal]
                              [--regions-only]]
                             [--forcing-grid FILE [--downscale] [--lapse-rate K_PER_M]
                              [--nearest RAINRATE,SWDOWN]]
                             [--interp [--interp-hold VAR[,VAR]]
                              [--interp-sw zenith|linear|hold] [--cosz-floor X]]
                             [--veg-clim [daily|step]]

Reads the namelist like the reference (noahmp_amd.config.Config ==
offline/noahmp_config.Config) and then does what the reference driver does
not yet do: runs the time loop through the engine (noahmp_amd.driver).

When the namelist's static_parameter_file exists, the run comes from files
(netCDF-3, noahmp_amd/ncio.py): grid and surface types from the static file,
the state from initialization_file (or --restart), forcing from the LDASIN
files in input_directory; output goes to LDASOUT files.
`tools/make_offline_case.py` writes such a set from the synthetic generator.
Otherwise the columns and forcing are the seeded synthetic set (`--kind
casenml` = the run/case.nml column of SURVEY 8d config #1, replicated --ncol
times).
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import noahmp_pkg  # noqa: E402,F401
from noahmp_amd import cases, config, driver, timeman  # noqa: E402
from noahmp_amd.params import Params  # noqa: E402

DEFAULT_NAMELIST_FILE = "case.nml"


def _spinup(drv, cfg, a):
    """--spinup-loops: the spin-up before the production run, one line per loop."""
    from noahmp_amd import layout
    t0 = time.perf_counter()
    drv.spinup(a.spinup_loops, tol=a.spinup_tol, min_loops=a.spinup_min_loops or 1,
               drift_map=a.spinup_map)
    el = time.perf_counter() - t0
    for r in drv.spinup_history:
        print(f"spin-up loop {r.loop}: " + "  ".join(
            f"{g} max {m:.6g} ({c} over)" for g, m, c in zip(layout.DRIFT_GROUPS, r.max, r.count)))
    print(f"spin-up: {drv.spinup_stop} in {el:.2f} s")
    if a.spinup_restart:
        os.makedirs(cfg.resdir, exist_ok=True)
        stamp = drv.t.strftime("%Y%m%d%H")
        path = os.path.join(cfg.resdir, f"RESTART.{stamp}_DOMAIN1.spinup" +
                            (".nc" if drv.grid is not None else ".npz"))
        drv.save_restart(path)
        print(f"spin-up: state written to {path}")


def build_parser():
    ap = argparse.ArgumentParser(description="Noah-MP Land Surface Model (MI355X engine)")
    ap.add_argument("nmlfile", nargs="?", default=DEFAULT_NAMELIST_FILE, help="configuration file")
    ap.add_argument("--ncol", type=int, default=1)
    ap.add_argument("--kind", default="casenml", choices=("casenml", "mixed", "conus", "global"))
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--restart", default=None, help="restart file to start from")
    ap.add_argument("--device-forcing", action="store_true",
                    help="synthetic cases: generate the forcing on the GPU every step "
                         "(nmp_forcing_synth) instead of on the host")
    ap.add_argument("--precision", type=int, default=4, choices=(4, 8),
                    help="engine precision (fp32, the reference's, or fp64)")
    ap.add_argument("--cosz", default="device", choices=("device", "host"),
                    help="netCDF cases: COSZ formed on the device from the grid (default) or "
                         "computed on the host and uploaded every step")
    ap.add_argument("--no-ingest", action="store_true",
                    help="netCDF cases: build each LDASIN block on the host instead of "
                         "uploading the file's bytes for the device to select and order")
    ap.add_argument("--accumulate", action="store_true",
                    help="also write each output interval's accumulated output: time means "
                         "of the energy fluxes, totals of the water fluxes (ACCPRCP, ACCECAN, "
                         "..., SFCRNOFF, UGDRNOFF) and the water budget's closure (DSTOR, "
                         "WBRES) -- 35 fields per LDASOUT file instead of 16")
    ap.add_argument("--state-out", default=None, metavar="all|NAME[,NAME...]",
                    help="also write the land state at every output time: the named groups of "
                         "soil, snow and canopy fields (SOIL_M, SOIL_W, SOIL_T, SNEQV, SNOWH, TG, "
                         "TV, LAI, SAI, ZWT, WA, CANWAT, ISNOW, SNOWLIQ, TWS, SOILSAT, ROOT_M, "
                         "CARBON, SNOW_T, SNOW_Z, SNOWT_AVG), or all of them")
    ap.add_argument("--extremes", default=None, metavar="NAME[:STAT[+STAT]][,NAME...]",
                    help="also write each output interval's extremes of the named series: an "
                         "output flux (FSH, T2M, RUNSRF, ...), a forcing row (PRCP, SFCTMP, ...), "
                         "a state field (TG, SNEQV, ...) or a soil layer (SMC1..4, SH2O1..4, "
                         "STC1..4), each with stats of max, min, tmax, tmin (default max+min), "
                         "e.g. T2M,TRAD:max,PRCP:max+tmax -- variables <NAME>_MAX, _MIN and the "
                         "seconds into the interval at which each occurred, _TMAX, _TMIN")
    ap.add_argument("--interval-stats", default=None,
                    metavar="[LABEL=]NAME[@OPc][:STAT[+STAT]][,...]",
                    help="also write each output interval's statistics of the named series "
                         "(the series of --extremes): without a condition the interval's mean, "
                         "e.g. T2M,SMC1 -- variables T2M_MEAN, SMC1_MEAN; with a condition gt, "
                         "ge, lt or le and a threshold, under a label, the seconds it held "
                         "(dur, the default), its longest unbroken spell (spell) and the "
                         "value-seconds beyond the threshold (deg), e.g. "
                         "FROST=T2M@lt273.15:dur+spell,GDD=SFCTMP@gt278.15:deg -- variables "
                         "FROST_DUR, FROST_SPELL, GDD_DEG")
    ap.add_argument("--regions", default=None, metavar="FILE",
                    help="netCDF cases: a region file on the run's grid (int REGION, optional "
                         "double AREA); every output time then also writes the regions' "
                         "weighted means of the output fields (<stamp>.REGIONS_DOMAIN1)")
    ap.add_argument("--region-weights", default="area", choices=("area", "equal"),
                    help="weights of the region means: the file's AREA (else cos(latitude)), "
                         "or 1 for every column")
    ap.add_argument("--regions-only", action="store_true",
                    help="with --regions: write the REGIONS files and no LDASOUT grids")
    ap.add_argument("--forcing-grid", default=None, metavar="FILE",
                    help="netCDF cases: the LDASIN files are stored on the coarser rectilinear "
                         "grid this file describes (lat, lon, optional HGT, MASK, HGT_M) and are "
                         "interpolated to the model grid on the device (nmp_ldasin_regrid)")
    ap.add_argument("--downscale", action="store_true",
                    help="with --forcing-grid: correct T2D, PSFC, Q2D and LWDOWN for the "
                         "elevation difference HGT_M - HGT (nmp_ldasin_downscale)")
    ap.add_argument("--lapse-rate", type=float, default=0.0065, metavar="K_PER_M",
                    help="lapse rate of --downscale (default 0.0065 K/m)")
    ap.add_argument("--nearest", default="", metavar="VAR[,VAR]",
                    help="with --forcing-grid: LDASIN variables that take their nearest source "
                         "point instead of the bilinear value, e.g. RAINRATE,SWDOWN")
    ap.add_argument("--interp", action="store_true",
                    help="netCDF cases: interpolate the forcing between input times on the "
                         "device (nmp_forcing_from_ldasin_interp) instead of holding each file's "
                         "values over its input interval")
    ap.add_argument("--interp-hold", default="RAINRATE", metavar="VAR[,VAR]",
                    help="with --interp: LDASIN variables held at the earlier file's value "
                         "(default RAINRATE, an interval rate)")
    ap.add_argument("--interp-sw", default="zenith", choices=("zenith", "linear", "hold"),
                    help="with --interp: SWDOWN follows the step's own COSZ through the files' "
                         "clearness ratios (default), or is interpolated linearly, or held")
    ap.add_argument("--cosz-floor", type=float, default=0.05, metavar="X",
                    help="with --interp-sw zenith: lower bound of COSZ in the clearness ratio "
                         "SWDOWN / max(COSZ, X) (default 0.05)")
    ap.add_argument("--veg-clim", nargs="?", const="daily", default=None,
                    choices=("daily", "step"),
                    help="netCDF cases: the vegetation fraction SHDFAC follows the static file's "
                         "monthly GREENFRAC through the run, re-formed on the device once per "
                         "model day (daily, the bare flag) or before every step (step), instead "
                         "of staying at the run's first instant (nmp_static_monthly).  Only "
                         "opt_veg = 1 reads SHDFAC: with other values the option has no effect")
    ap.add_argument("--spinup-loops", type=int, default=None, metavar="N",
                    help="before the run, spin the state up: run the period up to N times, "
                         "each pass from the state the pass before left, writing no output, "
                         "and report the state's drift between passes (measured on the device)")
    ap.add_argument("--spinup-tol", default=None, metavar="G=X[,G=X]",
                    help="with --spinup-loops: stop once no column's drift exceeds these "
                         "tolerances (groups SOIL_M, SOIL_T, SNEQV, WA, ZWT, TWS, CARBON; a "
                         "group not named never holds the loop up)")
    ap.add_argument("--spinup-min-loops", type=int, default=None, metavar="M",
                    help="with --spinup-tol: run at least M passes (default 1)")
    ap.add_argument("--spinup-map", action="store_true",
                    help="netCDF cases: write the last pass's drift on the grid "
                         "(SPINUP_DRIFT_DOMAIN1)")
    ap.add_argument("--spinup-restart", action="store_true",
                    help="write the spun-up state at the start time as a restart file "
                         "(RESTART.<stamp>_DOMAIN1.spinup.nc, or .npz without a grid)")
    return ap


def main(argv=None):
    ap = build_parser()
    a = ap.parse_args(argv)
    if a.spinup_loops is None and (a.spinup_tol is not None or a.spinup_min_loops is not None
                                   or a.spinup_map or a.spinup_restart):
        ap.error("--spinup-tol, --spinup-min-loops, --spinup-map and --spinup-restart need "
                 "--spinup-loops")
    if a.spinup_loops is not None:
        from noahmp_amd import spinup
        if a.spinup_loops < 1 or (a.spinup_min_loops is not None and a.spinup_min_loops < 1):
            ap.error("--spinup-loops and --spinup-min-loops must be at least 1")
        if a.spinup_tol is not None:
            try:
                spinup.parse_tol(a.spinup_tol)
            except ValueError as e:
                ap.error(str(e))
    if a.regions_only and not a.regions:
        ap.error("--regions-only needs --regions")
    if (a.downscale or a.nearest) and not a.forcing_grid:
        ap.error("--downscale and --nearest need --forcing-grid")
    cfg = config.Config(a.nmlfile)
    P = Params.builtin()
    skw = {}
    if a.state_out is not None:
        from noahmp_amd import stateout
        try:
            stateout.parse_groups(a.state_out)
        except ValueError as e:
            ap.error(str(e))
        skw = dict(state_out=a.state_out)
    if a.extremes is not None:
        from noahmp_amd import extremes
        try:
            extremes.parse(a.extremes)
        except ValueError as e:
            ap.error(str(e))
        skw.update(extremes=a.extremes)
    if a.interval_stats is not None:
        from noahmp_amd import intstats
        try:
            intstats.parse(a.interval_stats)
        except ValueError as e:
            ap.error(str(e))
        skw.update(interval_stats=a.interval_stats)
    if os.path.isfile(cfg.constfile):
        rkw = dict(skw)
        if a.regions:
            rkw.update(regions=a.regions, region_weights=a.region_weights,
                       write_grids=not a.regions_only)
        if a.forcing_grid:
            rkw.update(forcing_grid=a.forcing_grid, downscale=a.downscale,
                       lapse_rate=a.lapse_rate,
                       nearest=tuple(v for v in a.nearest.split(",") if v))
        if a.interp:
            hold = [v for v in a.interp_hold.split(",") if v]
            if a.interp_sw == "hold" and "SWDOWN" not in hold:
                hold.append("SWDOWN")
            rkw.update(interp=True, hold=tuple(hold), sw_zenith=a.interp_sw == "zenith",
                       cosz_floor=a.cosz_floor)
        if a.veg_clim:
            rkw.update(veg_clim=a.veg_clim)
        drv =driver.OfflineDriver.from_files(cfg, device=a.device, params=P, init=a.restart,
                                              precision=a.precision, cosz=a.cosz,
                                              ingest=not a.no_ingest, accumulate=a.accumulate,
                                              **rkw)
        a.ncol = drv.cs.ncol
    else:
        if a.regions or a.forcing_grid or a.interp or a.veg_clim:
            ap.error("--regions, --forcing-grid, --interp and --veg-clim need a run from files "
                     "(the namelist's static_parameter_file)")
        cols = cases.make_columns(a.ncol, a.kind, P.as_dict(), seed=0,
                                  julian=timeman.julian(cfg.begdatetime))
        drv = driver.OfflineDriver(cfg, cols, device=a.device, params=P,
                                   forcing="device" if a.device_forcing else None,
                                   precision=a.precision, accumulate=a.accumulate, **skw)
        if a.restart:
            drv.load_restart(a.restart)
    if a.spinup_loops is not None:
        if a.spinup_map and drv.grid is None:
            ap.error("--spinup-map needs a run from files (a grid)")
        _spinup(drv, cfg, a)
    t0 = time.perf_counter()
    drv.run()
    el = time.perf_counter() - t0
    print(f"{drv.step_index} steps x {a.ncol} columns to {drv.t.isoformat()} in {el:.2f} s; "
          f"{len(drv.written) + len(drv.regions_written)} output files in {cfg.outdir}; "
          "status bits set on "
          f"{int((drv.cs.status != 0).sum())} columns")
    if drv.interp_held:
        print("interp: no input file at the end of the interval of "
              f"{', '.join(t.isoformat() for t in drv.interp_held)}; it ran held")
    return 0


if __name__ == "__main__":
    sys.exit(main())
