"""The file-format kernels around the step (GPU box): per-launch time and
achieved HBM bandwidth against their algorithmic bytes, at 1,048,576 columns.

  forcing_from_ldasin      reads the 9-row fp32 block (36 B), writes 12 fields
                           (48 B fp32 / 96 B fp64)
  forcing_from_ldasin_geo  reads 8 rows (32 B) + geo (24 B), writes 12 fields;
                           one double cosine per column
  forcing_from_ldasin_interp  reads both blocks of the input interval (2 x 36 B
                           with the zenith scheme, counted whole although a
                           held row of block 1 is not loaded; 2 x 32 B for the
                           linear case, which reads no COSZ row) + geo (24 B),
                           writes 12 fields; one double cosine and, with the
                           zenith scheme, two double divisions per column
  ldasin_cosz              reads geo (24 B), writes one row (4 B); one double
                           cosine per column, once per input file
  ldasin_ingest            reads 8 gathered 4-byte words + the point (36 B),
                           writes 8 rows (32 B)
  ldasin_regrid            reads 4 corners + 4 weights (48 B) and 32 gathered
                           words of a small 128 x 256 source grid (cache
                           resident: not counted), writes 8 rows (32 B);
                           bilinear, and RAINRATE + SWDOWN nearest
  ldasin_downscale         reads dz + 4 rows (20 B), writes 4 rows (16 B); two
                           double exponentials and five double divisions
  ldasout_grid             fills 16 grids (64 B per grid point), then reads 16
                           fluxes + the point (68 B) and scatters them (64 B)
  state_output             every group: reads 44 state rows, ISNOW and 3 static
                           rows (192 B fp32), writes 39 rows (156 B); SOIL_M
                           alone: reads 4 rows, writes 4
                           (stateout.algorithmic_bytes)
  state_drift              reads 24 state rows, ISNOW, IST and the 13-row
                           snapshot, writes 7 drift rows and the snapshot
                           (236 B fp32, 464 B fp64); the snapshot alone: reads
                           the state rows, writes 13
  drift_reduce             both passes: reads 7 drift rows and the weight
                           (36 B fp32, 64 B fp64) (spinup.algorithmic_bytes)
  static_monthly           reads two of the table's 12 fp32 rows (8 B), writes
                           the SHDFAC row (4 B fp32, 8 B fp64)
  accumulate               reads 16 flux rows and PRCP, reads and writes the 17
                           double accumulators (340 B fp32, 408 B fp64)
  water_storage            reads IST and, of a soil column, ISNOW and 13 state
                           rows (counted for every column), writes one value
  extremes_update          a step past the interval's first that sets no new
                           extreme: per series reads the value and the running
                           maximum and minimum (12 B fp32, 24 B fp64), writes
                           nothing; with 4 and with 16 series
  extremes_output          every stat of every series: reads val and when
                           (16 B fp32, 24 B fp64 per series), writes 4 rows
  intstats_update          a step past the interval's first, half of the items
                           conditioned with a threshold that holds on about
                           half of the columns: a mean item reads the value and
                           reads and writes its double sum (20 B fp32, 24 B
                           fp64); a conditioned one reads the value, the sum
                           and three counters and writes the sum, the count and
                           the run, rows counted whole (40 B fp32, 44 B fp64);
                           with 4 and with 16 items
  intstats_output          every stat of every item: a mean item reads its sum
                           and writes 1 row, a conditioned one reads the sum
                           and two counters and writes 3 rows

The two gather/scatter kernels are timed with the grid points in the
columns' own order (`point` = identity: coalesced) and fully shuffled (every
lane a different cache line: the worst case; the driver's coherent order lies
between, mostly runs of neighbouring points).  Times are HIP events around
`--reps` back-to-back launches on one stream (mean per launch); run under
`rocprofv3 --kernel-trace --stats` for the kernels' own durations.  Prints
one JSON line per kernel, precision and point order.

    python tools/io_kernels_bench.py [--ncol 1048576] [--reps 50] [--kernels NAME[,NAME]]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import noahmp_pkg  # noqa: E402,F401
from noahmp_amd import (cases as cases_mod, extremes as xtr, intstats as ist,  # noqa: E402
                        layout as L, spinup, stateout, timeman)
from noahmp_amd.engine import ColumnState, Engine  # noqa: E402
from noahmp_amd.params import Params  # noqa: E402

PEAK_GBS = 8000.0  # MI355X HBM3E (/opt/skills/guides/MI355X_MICROARCH.md)


def timed(fn, reps):
    s = torch.cuda.current_stream()
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(s)
    for _ in range(reps):
        fn()
    b.record(s)
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def _drift_reduce_args(eng, drift, weight, tol):
    """nmp_drift_reduce's arguments with the engine's own buffers
    (Engine.drift_reduce also copies the result to the host and waits for it:
    timed here are the two launches alone)."""
    import ctypes as C
    from noahmp_amd.engine import _ptr
    n, g = int(drift.shape[1]), L.NDRIFT
    buf = eng._drift_bufs(n)
    buf["tol"].copy_(torch.as_tensor(tol, device=drift.device))
    w = buf["words"]
    return (eng._h, n, n, _ptr(drift), _ptr(weight), _ptr(buf["tol"]), _ptr(buf["partial"]),
            _ptr(w, 0), _ptr(w, g), _ptr(w, 2 * g), _ptr(w, 3 * g), _ptr(w, 4 * g),
            C.c_void_p(torch.cuda.current_stream().cuda_stream))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ncol", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=None, help="also write the results as one JSON list")
    ap.add_argument("--kernels", default=None, metavar="NAME[,NAME]",
                    help="time only these kernels (default: all)")
    a = ap.parse_args()
    only = set(a.kernels.split(",")) if a.kernels else None
    n, dev = a.ncol, "cuda:0"
    rng = np.random.default_rng(0)
    npts = n
    points = {"identity": torch.arange(n, dtype=torch.int32, device=dev),
              "shuffled": torch.as_tensor(rng.permutation(npts)[:n].astype(np.int32), device=dev)}
    lat = np.radians(rng.uniform(-60, 70, n))
    lon = np.radians(rng.uniform(-180, 180, n))
    geo = torch.as_tensor(np.stack([np.sin(lat), np.cos(lat), lon]), device=dev)
    blk = torch.as_tensor(rng.uniform(1, 2, (L.NLDASIN, n)).astype(np.float32), device=dev)
    grid_be = torch.as_tensor(rng.integers(0, 2**31 - 1, (L.NLDASIN - 1, npts), dtype=np.int32),
                              device=dev)
    solar = timeman.solar_terms(172.5, 366)
    # a 128 x 256 source around the columns of a regular model grid, in its row-major order
    from noahmp_amd.regrid import RegridPlan, nearest_mask
    ny = max(1, int(np.sqrt(n)))
    nx = -(-n // ny)
    jj, ii = np.divmod(np.arange(n), nx)
    plan = RegridPlan.bilinear(np.linspace(24.0, 51.0, 128), np.linspace(-126.0, -65.0, 256),
                               25.0 + 25.0 * jj / ny, -125.0 + 59.0 * ii / nx).to(dev)
    src_be = torch.as_tensor(rng.uniform(1, 2, (L.NLDASIN - 1, plan.npts)).astype(">f4").view(
        np.int32), device=dev)
    dz = torch.as_tensor(rng.uniform(-500, 500, n).astype(np.float32), device=dev)
    blk2 = torch.as_tensor(rng.uniform(250, 300, (L.NLDASIN, n)).astype(np.float32), device=dev)
    near = nearest_mask(("RAINRATE", "SWDOWN"))
    # the interval's other block, and the driver's default hold (RAINRATE)
    blk_b = torch.as_tensor(rng.uniform(1, 2, (L.NLDASIN, n)).astype(np.float32), device=dev)
    hold = 1 << L.LDASIN.index("RAINRATE")
    # state output: a mixed column set (every ISNOW, soil and lake, all types)
    P = Params.builtin()
    so_cols = cases_mod.make_columns(n, "mixed", P.as_dict(), seed=0)
    so_cs = {4: ColumnState.from_host(so_cols, dev, torch.float32),
             8: ColumnState.from_host(so_cols, dev, torch.float64)}
    vc_tab = torch.as_tensor(rng.random((12, n)).astype(np.float32), device=dev)
    out = []
    for prec in (4, 8):
        eng = Engine(Params.builtin(), L.CASE_NML_OPTIONS, device=0, precision=prec)
        dt = torch.float32 if prec == 4 else torch.float64
        f = torch.empty((L.NFORCING, n), dtype=dt, device=dev)
        diag = torch.as_tensor(rng.normal(size=(L.NDIAG_OUT, n)), device=dev).to(dt)
        grids = torch.empty((L.NDIAG_OUT, npts), device=dev,
                            dtype=torch.int32 if prec == 4 else torch.int64)
        cases = [
            ("forcing_from_ldasin", None, lambda: eng.forcing_from_ldasin(blk, f),
             n * (36 + 12 * prec)),
            ("forcing_from_ldasin_geo", None, lambda: eng.forcing_from_ldasin(blk, f, geo=geo,
                                                                              solar=solar),
             n * (32 + 24 + 12 * prec)),
            ("forcing_from_ldasin_interp", "zenith, RAINRATE held",
             lambda: eng.forcing_from_ldasin_interp(blk, blk_b, 1 / 3, f, geo, solar, hold, True,
                                                    0.05),
             n * (2 * 36 + 24 + 12 * prec)),
            ("forcing_from_ldasin_interp", "linear, none held",
             lambda: eng.forcing_from_ldasin_interp(blk, blk_b, 1 / 3, f, geo, solar, 0, False,
                                                    0.05),
             n * (2 * 32 + 24 + 12 * prec)),
        ]
        if prec == 4:
            cases.append(("ldasin_cosz", None, lambda: eng.ldasin_cosz(blk_b, geo, solar),
                          n * (24 + 4)))
        for order, pt in points.items():
            cases.append(("ldasout_grid", order,
                          lambda pt=pt: eng.ldasout_grid(diag, pt, grids, -9999.0),
                          npts * 16 * prec + n * (16 * prec + 4 + 16 * prec)))
            if prec == 4:
                cases.append(("ldasin_ingest", order,
                              lambda pt=pt: eng.ldasin_ingest(grid_be, pt, blk),
                              n * (32 + 4 + 32)))
        if prec == 4:
            cases += [("ldasin_regrid", "bilinear",
                       lambda: eng.ldasin_regrid(src_be, plan, blk2), n * (48 + 32)),
                      ("ldasin_regrid", "2 nearest",
                       lambda: eng.ldasin_regrid(src_be, plan, blk2, near), n * (48 + 32)),
                      # (in place: repeated launches drift the block's values; timing only)
                      ("ldasin_downscale", None,
                       lambda: eng.ldasin_downscale(blk2, dz, 0.0065), n * (20 + 16))]
        # state output: every group (44 state rows, ISNOW and 3 static rows
        # read, 39 rows written) and SOIL_M alone (4 rows read, 4 written)
        so_out = torch.empty((L.NXROWS, n), dtype=dt, device=dev)
        for label in ("all", "SOIL_M"):
            mask = stateout.parse_groups(label)
            nrow = len(stateout.rows(mask))
            cases.append(("state_output", label,
                          lambda mask=mask, nrow=nrow: eng.state_output(so_cs[prec], mask,
                                                                        so_out[:nrow], -9999.0),
                          n * stateout.algorithmic_bytes(mask, prec)))
        # spin-up drift: the per-column kernel measuring a loop and arming the
        # next (and taking the snapshot alone), and the reduction with weights
        sp_bytes = spinup.algorithmic_bytes(prec)
        sp_snap = torch.zeros((L.NTRACKED, n), dtype=dt, device=dev)
        sp_drift = torch.as_tensor(rng.random((L.NDRIFT, n)), device=dev).to(dt)
        sp_w = torch.as_tensor(np.cos(lat), device=dev)
        sp_tol = np.full(L.NDRIFT, 0.5)
        cases += [("state_drift", "drift + snapshot",
                   lambda: eng.state_drift(so_cs[prec], sp_snap, sp_drift),
                   n * sp_bytes["state_drift"]),
                  ("state_drift", "snapshot only",
                   lambda: eng.state_drift(so_cs[prec], sp_snap),
                   n * sp_bytes["state_drift_snapshot"])]
        dr_args = _drift_reduce_args(eng, sp_drift, sp_w, sp_tol)
        cases.append(("drift_reduce", "weights, both passes",
                      lambda: eng._lib.nmp_drift_reduce(*dr_args), n * sp_bytes["drift_reduce"]))
        # vegetation fraction: SHDFAC between two months of the resident table
        vc_row = torch.empty(n, dtype=dt, device=dev)
        cases.append(("static_monthly", None,
                      lambda: eng.static_monthly(vc_tab, 5, 6, 1 / 3, vc_row), n * (8 + prec)))
        # accumulated output and interval extremes: the every-step kernels
        # behind the step.  The extremes' resident state is primed by one call
        # with k = 1; the timed calls (k = 2, the same values) set no new extreme
        acc = torch.zeros((L.NACC, n), dtype=torch.float64, device=dev)
        frc = torch.as_tensor(rng.normal(size=(L.NFORCING, n)), device=dev).to(dt)
        cases.append(("accumulate", None, lambda: eng.accumulate(diag, frc, acc, 900.0),
                      n * (17 * prec + 2 * 17 * 8)))
        stor = torch.empty(n, dtype=dt, device=dev)
        cases.append(("water_storage", None, lambda: eng.water_storage(so_cs[prec], stor),
                      n * (13 * prec + 8 + prec)))
        for spec in ("T2M,PRCP,TG,SNEQV",
                     "FSH,TRAD,T2M,RUNSRF,RUNSUB,ALBEDO,PRCP,SFCTMP,TG,TV,SNEQV,SNOWH,SMC1,"
                     "SH2O1,STC1,ZWT"):
            ser = xtr.parse([(x, 15) for x in spec.split(",")])
            ns = len(ser)
            kr, masks = xtr.pairs(ser), xtr.masks(ser)
            xval = torch.zeros((2 * ns, n), dtype=dt, device=dev)
            xwhen = torch.zeros((2 * ns, n), dtype=torch.int32, device=dev)
            xout = torch.empty((4 * ns, n), dtype=dt, device=dev)
            st = so_cs[prec].state
            eng.extremes_update(kr, 1, xval, xwhen, diag, frc, st)
            cases += [("extremes_update", f"{ns} series",
                       lambda kr=kr, xval=xval, xwhen=xwhen, st=st: eng.extremes_update(
                           kr, 2, xval, xwhen, diag, frc, st), n * ns * 3 * prec),
                      ("extremes_output", f"{ns} series, 4 stats",
                       lambda masks=masks, xval=xval, xwhen=xwhen, xout=xout: eng.extremes_output(
                           masks, 900.0, xval, xwhen, xout), n * ns * (2 * (prec + 4) + 4 * prec))]
        # interval statistics: half of the items means, half conditions that hold on
        # about half of the columns (the blocks are standard normal; the state's
        # rows have their medians as thresholds); primed by one call with k = 1
        st = so_cs[prec].state
        med = {x: float(st[ist.SOURCES[x][1]].double().median()) for x in
               ("TG", "SNEQV", "SMC1", "STC1")}
        for spec in ("T2M,TG,WARM=SFCTMP@gt0:dur+deg+spell,WET=PRCP@gt0:dur+deg+spell",
                     "FSH,TRAD,T2M,ALBEDO,TG,SNEQV,SMC1,STC1,"
                     + ",".join(f"C{i}={x}@{op}0:dur+deg+spell" for i, (x, op) in enumerate(
                         [("FSH", "gt"), ("RUNSRF", "ge"), ("PRCP", "gt"), ("SFCTMP", "lt")]))
                     + "," + ",".join(f"S{i}={x}@{op}{med[x]!r}:dur+deg+spell" for i, (x, op) in
                                      enumerate([("TG", "gt"), ("SNEQV", "le"), ("SMC1", "lt"),
                                                 ("STC1", "ge")]))):
            items = ist.parse(spec)
            ni, nc = len(items), sum(it.op != L.IST_NONE for it in items)
            tab, thr = ist.table(items), ist.thresholds(items)
            iacc = torch.zeros((ni, n), dtype=torch.float64, device=dev)
            icnt = torch.zeros((3 * ni, n), dtype=torch.int32, device=dev)
            iout = torch.empty((len(ist.row_names(items)), n), dtype=dt, device=dev)
            eng.intstats_update(tab, thr, 1, iacc, icnt, diag, frc, st)
            cases += [("intstats_update", f"{ni} items, {nc} conditioned",
                       lambda tab=tab, thr=thr, iacc=iacc, icnt=icnt: eng.intstats_update(
                           tab, thr, 2, iacc, icnt, diag, frc, st),
                       n * ((ni - nc) * (prec + 16) + nc * (prec + 36))),
                      ("intstats_output", f"{ni} items, every stat",
                       lambda tab=tab, iacc=iacc, icnt=icnt, iout=iout: eng.intstats_output(
                           tab, 12, 900.0, iacc, icnt, iout),
                       n * ((ni - nc) * (8 + prec) + nc * (16 + 3 * prec)))]
        for name, order, fn, nbytes in cases:
            if only and name not in only:
                continue
            ms = timed(fn, a.reps)
            gbs = nbytes / (ms * 1e-3) / 1e9
            r = {"kernel": name, "precision": prec, "ncol": n, "point_order": order,
                 "ms_per_launch": ms, "algorithmic_bytes": nbytes, "achieved_gb_s": gbs,
                 "hbm_frac": gbs / PEAK_GBS}
            print(json.dumps(r), flush=True)
            out.append(r)
        eng.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
