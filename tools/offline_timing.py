"""The offline driver at scale: the host path north_star
names (the repo's Python driver calling the engine through ctypes), timed on
a 1,048,576-column netCDF case from the namelist's files.

Writes a case (tools/make_offline_case.py: static file, initial state, hourly
LDASIN files without CO2AIR / O2AIR, the standard HRLDAS set) for
examples/offline_case.nml's day (96 steps of 900 s, output every 3 hours),
then runs `OfflineDriver.from_files` over it in each upload mode and
precision: the 12 forcing fields built on the host and uploaded (48 B per
column per step in fp32, 96 in fp64), the LDASIN block (the files' 8
variables + COSZ, fp32, 36 B) expanded on the device (nmp_forcing_from_ldasin),
and that block uploaded once per input file with COSZ formed on the device
(cosz="device", nmp_forcing_from_ldasin_geo: no upload between files), built
on the host or -- the default -- formed on the device from the file's bytes
as stored (ingest, nmp_ldasin_ingest: the host only copies them).
After 4 warm-up steps the remaining steps are timed, wall clock between two
synchronizes, with the driver's own per-phase host times (`phase_s`: LDASIN
file reads, forcing build + upload enqueue, launch enqueue, output gather +
LDASOUT writes).  The engine alone on the same columns with resident forcing
is timed alongside, the ceiling the driver approaches.

    python tools/offline_timing.py --out profiles/r06/offline_driver.json

--forcing-grid SY SX times the forcing-on-its-own-grid path instead: the same
case with its LDASIN files on a coarse SY x SX source grid (e.g. 128 256),
regridded on the device (nmp_ldasin_regrid), with and without the elevation
downscaling, against the same values fed as pre-regridded model-grid files
(nmp_ldasin_ingest) -- ms per step and bytes uploaded per input interval.

--interp-runs N times interpolation between input times instead: the same case
with 3-hourly files, N fresh runs each with interp=True and without (the held
path), interleaved -- ms per step of every run, median and range per variant.

--state-out-runs N times state output instead: N fresh runs each with
state_out="all" and without, interleaved, reported the same way.

--veg-clim-runs N times the vegetation fraction's updates instead: the case
with a seasonal GREENFRAC, N fresh runs each without veg_clim and with
veg_clim="step", interleaved, reported the same way.

--extremes-runs N times the interval extremes instead: N fresh runs of each of
--variants (default off,state,diag: without the option, with a spec of state
and forcing series only, with a spec that has flux series and so writes the
fluxes every step), interleaved with the order rotated, reported the same way.

--interval-stats-runs N does the same for the interval statistics (variants
off, state, diag: means and conditioned items of state and forcing series only,
and a spec with flux items).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402

import noahmp_pkg  # noqa: E402,F401
from noahmp_amd import config, driver, layout as L  # noqa: E402


def write_namelist(d: str) -> str:
    text = open(os.path.join(ROOT, "examples", "offline_case.nml")).read()
    for k in ("geo_em.d01.nc", "init.nc", "ldasin", "ldasout", "restart"):
        text = text.replace(f"'{k}'", f"'{os.path.join(d, k)}'").replace(
            f'"{k}"', f'"{os.path.join(d, k)}"')
    p = os.path.join(d, "case.nml")
    with open(p, "w") as f:
        f.write(text)
    return p


# the "upload" label of a run's forcing path (feeds.feed_kind)
UPLOAD_LABEL = {"host": "12 fields", "device-synth": "12 fields", "ldasin-step": "ldasin block",
                "ldasin-block": "ldasin block + device cosz",
                "ldasin-ingest": "file bytes, device ingest + cosz",
                "ldasin-regrid": "coarse file bytes, device regrid",
                "ldasin-interp": "file bytes, device ingest + interpolation in time"}


def time_driver(cfg, precision, ldasin, warm, steps, threads, cosz="host", ingest=False, **kw):
    import torch
    t0 = time.perf_counter()
    drv = driver.OfflineDriver.from_files(cfg, precision=precision, ldasin_upload=ldasin,
                                          host_threads=threads, cosz=cosz, ingest=ingest, **kw)
    setup = time.perf_counter() - t0
    drv.run(nsteps=warm)
    torch.cuda.synchronize()
    drv.phase_s.clear()
    n_written = len(drv.written)
    upl = drv.ingest or drv.raw_upload or drv.upload
    up0 = upl.count
    t0 = time.perf_counter()
    drv.run(nsteps=steps)
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    n = drv.cs.ncol
    outs = len(drv.written) - n_written
    puts = upl.count - up0
    bytes_per_put = upl.host[0].numel() * upl.host[0].element_size()
    kind = UPLOAD_LABEL[drv.feed.kind] + (
        " + downscale" if drv.feed.kind == "ldasin-regrid" and drv.downscale else "")
    res = {"precision": precision, "upload": kind, "host_threads": threads, "ncol": n,
           "steps": steps, "output_steps": outs, "uploads": puts,
           "wall_s": el, "ms_per_step": el * 1e3 / steps, "colsteps_per_s": n * steps / el,
           "phase_ms_per_step": {k: v * 1e3 / steps for k, v in drv.phase_s.items()},
           "pcie_up_bytes_per_step": bytes_per_put * puts / steps,
           "pcie_up_bytes_per_input_interval": bytes_per_put,
           "pcie_down_bytes_per_output_step": L.NDIAG_OUT * precision * n,
           "setup_s": setup,
           "status_nonzero_cols": int((drv.cs.status != 0).sum().item())}
    state = drv.cs.state.cpu().numpy()
    drv.engine.close()
    return res, state, drv


def time_engine(drv_like, precision, steps):
    """The engine alone: the driver's columns (same order), resident forcing
    (one step's fields), two stream ranges, no output."""
    import torch
    from noahmp_amd.engine import StreamShards
    cs, eng = drv_like.cs, driver.Engine(drv_like.engine.params, drv_like.cfg.engine_options(),
                                         0, precision)
    f = drv_like.upload.dev[0] if drv_like.raw_upload is None else drv_like.raw_fbuf[0]
    sh = StreamShards(eng, cs, 2)
    jul = 1.0
    for _ in range(4):
        sh.step(f, drv_like.zsoil, drv_like.dt, jul, 366)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        sh.step(f, drv_like.zsoil, drv_like.dt, jul, 366)
    sh.join()
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    eng.close()
    return {"precision": precision, "ms_per_step": el * 1e3 / steps,
            "colsteps_per_s": cs.ncol * steps / el}


def coarse_forcing_runs(a, nml):
    """The case on a coarse source grid, device-regridded (with and without
    downscaling), against pre-regridded model-grid files of the same values."""
    import make_offline_case
    from noahmp_amd import ncio
    from noahmp_amd.params import Params
    make_offline_case.main([nml, "--ny", str(a.ny), "--nx", str(a.nx), "--kind", "mixed",
                            "--forcing-grid", *[str(v) for v in a.forcing_grid]])
    cfg = config.Config(nml)
    coarse = cfg.indir
    fgpath = os.path.join(coarse, "forcing_grid.nc")
    grid, _, _ = ncio.read_static(cfg.constfile, Params.builtin().as_dict(), cfg.begdatetime)
    fr = ncio.LdasinForcing(coarse, grid, cfg.begdatetime, cfg.input_interval,
                            src=ncio.read_forcing_grid(fgpath))
    pre = os.path.join(a.dir, "ldasin_model")
    os.makedirs(pre, exist_ok=True)
    inv = {v: k for k, v in ncio.LDASIN_MAP.items()}
    t = cfg.begdatetime
    while t < cfg.enddatetime:
        cols8 = fr.plan.apply_host(fr.grid_raw(t))
        f12 = np.zeros((L.NFORCING, grid.n), np.float32)
        for i, var in enumerate(L.LDASIN[:-1]):
            f12[L.FORCING.index(inv[var])] = cols8[i]
        ncio.write_ldasin(ncio.ldasin_path(pre, t), grid, f12, t, extras=False)
        t = t + cfg.input_interval
    print(f"pre-regridded model-grid files written to {pre}", flush=True)
    runs, states = [], []
    for indir, kw in ((pre, {}), (coarse, dict(forcing_grid=fgpath)),
                      (coarse, dict(forcing_grid=fgpath, downscale=True))):
        cfg.indir = indir
        r, st, drv = time_driver(cfg, 4, True, a.warm, a.steps, a.threads, "device", True, **kw)
        states.append(st)
        r["state_equals_first_run"] = bool(np.array_equal(states[0].view(np.uint8),
                                                          st.view(np.uint8)))
        print(json.dumps(r), flush=True)
        runs.append(r)
        del drv
    return runs


def interp_runs(a, nml):
    """The case with 3-hourly files (and the closing one): fresh runs with
    interp (resident blocks of both ends, nmp_forcing_from_ldasin_interp every
    step) and without (today's held path), interleaved; ms per step of each
    run, and each variant's median and range."""
    import make_offline_case
    text = open(nml).read().replace("input_frequency = '1 hour'", "input_frequency = '3 hour'")
    with open(nml, "w") as f:
        f.write(text)
    make_offline_case.main([nml, "--ny", str(a.ny), "--nx", str(a.nx), "--kind", "mixed",
                            "--closing-file"])
    cfg = config.Config(nml)
    runs = {"held": [], "interp": []}
    for i in range(a.interp_runs):
        for name, kw in (("held", {}), ("interp", dict(interp=True))):
            r, _, drv = time_driver(cfg, 4, True, a.warm, a.steps, a.threads, "device", True, **kw)
            r["variant"], r["round"] = name, i
            print(json.dumps(r), flush=True)
            runs[name].append(r)
            del drv
    summary = {}
    for name, rs in runs.items():
        ms = sorted(r["ms_per_step"] for r in rs)
        summary[name] = {"runs": len(ms), "median_ms_per_step": float(np.median(ms)),
                         "min_ms_per_step": ms[0], "max_ms_per_step": ms[-1]}
    print(json.dumps(summary), flush=True)
    return {"case": f"{a.ny} x {a.nx} land points (mixed USGS/STAS columns), 900-s steps, "
                    "3-hourly LDASIN with the closing file, 3-hourly LDASOUT; fp32, file bytes "
                    "ingested on the device; fresh drivers, variants interleaved",
            "summary": summary, "driver": runs["held"] + runs["interp"]}


def state_out_runs(a, nml):
    """The case as it is: fresh runs with state_out="all" (nmp_state_output on
    the 8 output steps, 55 grids per LDASOUT file) and without (16 grids),
    interleaved; ms per step of each run, and each variant's median and
    range."""
    import make_offline_case
    make_offline_case.main([nml, "--ny", str(a.ny), "--nx", str(a.nx), "--kind", "mixed"])
    cfg = config.Config(nml)
    runs = {"plain": [], "state_out": []}
    for i in range(a.state_out_runs):
        for name, kw in (("plain", {}), ("state_out", dict(state_out="all"))):
            r, _, drv = time_driver(cfg, 4, True, a.warm, a.steps, a.threads, "device", True, **kw)
            r["variant"], r["round"] = name, i
            r["pcie_down_bytes_per_output_step"] = len(drv.out_names) * 4 * drv.cs.ncol
            print(json.dumps(r), flush=True)
            runs[name].append(r)
            del drv
    summary = {}
    for name, rs in runs.items():
        ms = sorted(r["ms_per_step"] for r in rs)
        summary[name] = {"runs": len(ms), "median_ms_per_step": float(np.median(ms)),
                         "min_ms_per_step": ms[0], "max_ms_per_step": ms[-1]}
    print(json.dumps(summary), flush=True)
    return {"case": f"{a.ny} x {a.nx} land points (mixed USGS/STAS columns), 900-s steps, "
                    "hourly LDASIN, 3-hourly LDASOUT; fp32, file bytes ingested on the device; "
                    "fresh drivers, variants interleaved",
            "summary": summary, "driver": runs["plain"] + runs["state_out"]}


def veg_clim_runs(a, nml):
    """The case with a seasonal GREENFRAC: fresh runs without veg_clim and with
    veg_clim="step" (the worst case: nmp_static_monthly before every step of
    every range; "daily" enqueues it once per model day), interleaved; ms per
    step of each run, and each variant's median and range.  --variants picks
    other sets, e.g. "off" alone to time a tree without the option on a case
    written before (--keep-case)."""
    if not (a.keep_case and os.path.exists(config.Config(nml).constfile)):
        import make_offline_case
        make_offline_case.main([nml, "--ny", str(a.ny), "--nx", str(a.nx), "--kind", "mixed",
                                "--seasonal-greenfrac"])
    cfg = config.Config(nml)
    names = [v for v in a.variants.split(",") if v]
    runs = {v: [] for v in names}
    for i in range(a.veg_clim_runs):
        for name in names:
            kw = {} if name == "off" else dict(veg_clim=name)
            r, _, drv = time_driver(cfg, 4, True, a.warm, a.steps, a.threads, "device", True, **kw)
            r["variant"], r["round"] = name, i
            print(json.dumps(r), flush=True)
            runs[name].append(r)
            del drv
    summary = {}
    for name, rs in runs.items():
        ms = sorted(r["ms_per_step"] for r in rs)
        summary[name] = {"runs": len(ms), "median_ms_per_step": float(np.median(ms)),
                         "min_ms_per_step": ms[0], "max_ms_per_step": ms[-1]}
    print(json.dumps(summary), flush=True)
    return {"case": f"{a.ny} x {a.nx} land points (mixed USGS/STAS columns, seasonal GREENFRAC), "
                    "900-s steps, hourly LDASIN, 3-hourly LDASOUT; fp32, file bytes ingested on "
                    "the device; fresh drivers, variants interleaved",
            "summary": summary, "driver": [r for v in names for r in runs[v]]}


# --extremes-runs: the specs of the two variants with the option on
EXTREMES_SPECS = {"state": "PRCP:max+tmax,SFCTMP,TG,SNEQV,SMC1,STC1",
                  "diag": "T2M,TRAD,FSH:max+tmax,RUNSRF:max+tmax,PRCP:max+tmax,TG"}


# --interval-stats-runs: likewise
INTSTATS_SPECS = {"state": "TG,SNEQV,SMC1,STC1,FROST=SFCTMP@lt273.15:dur+spell+deg,"
                           "WET=PRCP@gt0:dur+spell",
                  "diag": "T2M,TRAD,TG,HEAT=FSH@gt0:deg,RUNOFF=RUNSRF@gt0:dur+spell,"
                          "WET=PRCP@gt0:dur+spell"}


def extremes_runs(a, nml, option="extremes", specs=None, count=None):
    """Fresh runs without extremes ("off"), with state and forcing series only
    ("state": the steps between output steps stay at DIAG_NONE) and with flux
    series ("diag": every step writes its fluxes), interleaved, the order
    rotated from round to round; ms per step of each run, and each variant's
    median and range.  "off" alone with --keep-case times this tree on a case
    written before, next to another tree's runs on the same files.
    option, specs, count: the same for another option of the driver that takes
    a spec (interval_stats with INTSTATS_SPECS)."""
    if not (a.keep_case and os.path.exists(config.Config(nml).constfile)):
        import make_offline_case
        make_offline_case.main([nml, "--ny", str(a.ny), "--nx", str(a.nx), "--kind", "mixed"])
    cfg = config.Config(nml)
    names = [v for v in a.variants.split(",") if v]
    runs = {v: [] for v in names}
    specs = EXTREMES_SPECS if specs is None else specs
    for i in range(a.extremes_runs if count is None else count):
        for name in names[i % len(names):] + names[:i % len(names)]:
            kw = {} if name == "off" else {option: specs[name]}
            r, _, drv = time_driver(cfg, 4, True, a.warm, a.steps, a.threads, "device", True, **kw)
            r["variant"], r["round"] = name, i
            r["pcie_down_bytes_per_output_step"] = len(drv.out_names) * 4 * drv.cs.ncol
            print(json.dumps(r), flush=True)
            runs[name].append(r)
            del drv
    summary = {}
    for name, rs in runs.items():
        ms = sorted(r["ms_per_step"] for r in rs)
        summary[name] = {"runs": len(ms), "median_ms_per_step": float(np.median(ms)),
                         "min_ms_per_step": ms[0], "max_ms_per_step": ms[-1]}
        if name != "off":
            summary[name]["spec"] = specs[name]
    print(json.dumps(summary), flush=True)
    return {"case": f"{a.ny} x {a.nx} land points (mixed USGS/STAS columns), 900-s steps, "
                    "hourly LDASIN, 3-hourly LDASOUT; fp32, file bytes ingested on the device; "
                    "fresh drivers, variants interleaved, order rotated",
            "summary": summary, "driver": [r for v in names for r in runs[v]]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--extremes-runs", type=int, default=0, metavar="N",
                    help="time N fresh runs each of --variants (off, state, diag: without "
                         "extremes, with state / forcing series, with flux series), interleaved, "
                         "instead")
    ap.add_argument("--interval-stats-runs", type=int, default=0, metavar="N",
                    help="the same for interval_stats: means and conditioned items of state / "
                         "forcing series (state), with flux items (diag)")
    ap.add_argument("--veg-clim-runs", type=int, default=0, metavar="N",
                    help="time N fresh runs each without veg_clim and with veg_clim='step', "
                         "interleaved, instead")
    ap.add_argument("--variants", default=None, metavar="NAME[,NAME]",
                    help="with --veg-clim-runs: the variants to time (off, daily, step; default "
                         "off,step); with --extremes-runs or --interval-stats-runs: off, state, "
                         "diag (default all three)")
    ap.add_argument("--keep-case", action="store_true",
                    help="with --veg-clim-runs, --extremes-runs or --interval-stats-runs: reuse the "
                         "case files in "
                         "--dir if they exist")
    ap.add_argument("--state-out-runs", type=int, default=0, metavar="N",
                    help="time N fresh runs each with and without state_out='all', interleaved, "
                         "instead")
    ap.add_argument("--interp-runs", type=int, default=0, metavar="N",
                    help="time N fresh runs each with and without interp on 3-hourly files, "
                         "interleaved, instead")
    ap.add_argument("--forcing-grid", type=int, nargs=2, default=None, metavar=("SY", "SX"),
                    help="time the coarse-forcing path against pre-regridded files instead")
    ap.add_argument("--ny", type=int, default=1024)
    ap.add_argument("--nx", type=int, default=1024)
    ap.add_argument("--dir", default=os.path.join(os.environ.get("TMPDIR", "/tmp"), "nmp_case"))
    ap.add_argument("--warm", type=int, default=4)
    ap.add_argument("--steps", type=int, default=92)
    ap.add_argument("--precisions", default="4,8")
    ap.add_argument("--threads", type=int, default=8, help="host threads of the threaded runs")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    os.makedirs(a.dir, exist_ok=True)
    nml = write_namelist(a.dir)
    if a.variants is None:
        a.variants = "off,state,diag" if a.extremes_runs or a.interval_stats_runs else "off,step"
    if a.interp_runs or a.state_out_runs or a.veg_clim_runs or a.extremes_runs or \
            a.interval_stats_runs:
        res = (interp_runs(a, nml) if a.interp_runs else state_out_runs(a, nml)
               if a.state_out_runs else veg_clim_runs(a, nml) if a.veg_clim_runs
               else extremes_runs(a, nml) if a.extremes_runs
               else extremes_runs(a, nml, "interval_stats", INTSTATS_SPECS,
                                  a.interval_stats_runs))
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                json.dump(res, f, indent=1)
        return 0
    if a.forcing_grid:
        runs = coarse_forcing_runs(a, nml)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                json.dump({"case": f"{a.ny} x {a.nx} land points, LDASIN on a "
                                   f"{a.forcing_grid[0]} x {a.forcing_grid[1]} source grid",
                           "driver": runs}, f, indent=1)
        return 0
    import make_offline_case
    t0 = time.perf_counter()
    make_offline_case.main([nml, "--ny", str(a.ny), "--nx", str(a.nx), "--kind", "mixed"])
    t_case = time.perf_counter() - t0
    print(f"case written in {t_case:.1f} s", flush=True)
    cfg = config.Config(nml)
    runs, engine = [], []
    for prec in [int(p) for p in a.precisions.split(",")]:
        states = []
        # round 5's path (12 fields, one host thread), the threaded host build,
        # and the LDASIN block expanded on the device
        # and the block once per file with COSZ formed on the device
        for ldasin, threads, cz, ing in ((False, 1, "host", False), (False, a.threads, "host", False),
                                         (True, a.threads, "host", False),
                                         (True, a.threads, "device", False),
                                         (True, a.threads, "device", True)):
            r, st, drv = time_driver(cfg, prec, ldasin, a.warm, a.steps, threads, cz, ing)
            states.append(st)
            r["state_equals_first_run"] = bool(np.array_equal(states[0].view(np.uint8),
                                                              st.view(np.uint8)))
            if cz == "device":  # COSZ from the device's double cosine: columns apart by 1 ulp
                iv = np.uint32 if st.dtype == np.float32 else np.uint64
                r["state_cols_differing_from_first_run"] = int(
                    (states[0].view(iv) != st.view(iv)).any(0).sum())
            print(json.dumps(r), flush=True)
            runs.append(r)
        e = time_engine(drv, prec, a.steps)
        print(json.dumps(e), flush=True)
        engine.append(e)
        del drv
    out = {"case": f"{a.ny} x {a.nx} land points (mixed USGS/STAS columns), examples/"
                   f"offline_case.nml day: 900-s steps, hourly LDASIN, 3-hourly LDASOUT",
           "case_write_s": t_case, "driver": runs, "engine_resident_forcing": engine}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
