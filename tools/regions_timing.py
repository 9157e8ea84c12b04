#!/usr/bin/env python3
"""What region-aggregated output costs (GPU box): the nmp_region_reduce call
alone against its algorithmic bytes, and the offline driver's ms per step with
and without it, at 1,048,576 columns.

    python tools/regions_timing.py [--out profiles/regions/timing.json]

Kernel.  35 fields (an accumulating run's output block), fp32 and fp64, plans
of 1, 64 and 65,536 equal regions whose members are runs of neighbouring
columns ("coherent": region = column // size, what a basin is in the engine's
coherent column order) or drawn at random over the block ("shuffled": every
lane another cache line).  Time per call (both passes) from HIP events around
`--reps` back-to-back calls on one stream, median of `--repeats`.  Algorithmic
bytes: nfield n sizeof(T) values + 12 B per plan entry + 8 nfield (2 nchunk +
2 nreg) for the partials written and read and the sums and means written; the
HBM fraction is those bytes over the time over 8 TB/s.  nmp_ldasout_grid on the
same 35 fields in column order is timed in the same run as the yardstick (it
moves the same block once more than it reads it).

Driver.  A 1024 x 1024 netCDF case (tools/make_offline_case.py: the
examples/offline_case.nml day, 900-s steps, hourly LDASIN, output every 6
steps), 64 regions of 128 x 128 points weighted by cos(latitude), three
drivers per precision stepping the same case, their blocks of `--block` steps
interleaved in rotating order (host clock around OfflineDriver.run, which ends
in a device synchronise and the writers' flush):

  a  grids only: LDASOUT files, no regions (the path without the option);
  b  grids + regions: LDASOUT and REGIONS files;
  c  regions only (write_grids=False): REGIONS files, no grids.

No threshold: the numbers are written down (DESIGN.md "Region-aggregated
output")."""
import argparse
import glob
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import noahmp_pkg  # noqa: E402,F401
from noahmp_amd import config, driver, layout as L, ncio  # noqa: E402
from noahmp_amd.params import Params  # noqa: E402
from noahmp_amd.regions import RegionPlan  # noqa: E402

PEAK_GBS = 8000.0  # MI355X HBM3E


def timed(fn, reps, repeats):
    import torch
    s = torch.cuda.current_stream()
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(s)
        for _ in range(reps):
            fn()
        b.record(s)
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b) / reps)
    return float(np.median(ms)), [round(x, 5) for x in ms]


def kernel_timing(a):
    import torch
    from noahmp_amd.engine import Engine
    n, nf, dev = a.ncol, a.nfield, "cuda:0"
    rng = np.random.default_rng(0)
    shuffle = rng.permutation(n)
    rows = []
    for prec in (4, 8):
        eng = Engine(Params.builtin(), L.CASE_NML_OPTIONS, device=0, precision=prec)
        dt = torch.float32 if prec == 4 else torch.float64
        fields = torch.as_tensor(rng.normal(size=(nf, n)), device=dev).to(dt).contiguous()
        point = torch.arange(n, dtype=torch.int32, device=dev)
        grids = torch.empty((nf, n), device=dev, dtype=torch.int32 if prec == 4 else torch.int64)
        ms, reps = timed(lambda: eng.ldasout_grid(fields, point, grids, -9999.0), a.reps,
                         a.repeats)
        nbytes = n * nf * prec + n * (nf * prec + 4 + nf * prec)
        yard = {"kernel": "ldasout_grid", "precision": prec, "ncol": n, "nfield": nf,
                "point_order": "identity", "ms_per_call": ms, "ms_repeats": reps,
                "algorithmic_bytes": nbytes, "achieved_gb_s": nbytes / (ms * 1e-3) / 1e9,
                "hbm_frac": nbytes / (ms * 1e-3) / 1e9 / PEAK_GBS}
        print(json.dumps(yard), flush=True)
        rows.append(yard)
        for nreg in (1, 64, 65536):
            base = (np.arange(n) // -(-n // nreg)).astype(np.int64)
            for order in ("coherent", "shuffled"):
                ids = base if order == "coherent" else base[shuffle]
                plan = RegionPlan.from_ids(ids, rng.uniform(0.5, 1.5, n)).to(dev)
                sums = torch.empty((nf, plan.nreg), dtype=torch.float64, device=dev)
                means = torch.empty_like(sums)
                ms, reps = timed(lambda: eng.region_reduce(fields, plan, sums, means), a.reps,
                                 a.repeats)
                nent = plan.nchunk * L.REGION_CHUNK
                nbytes = nf * n * prec + 12 * nent + 8 * nf * (2 * plan.nchunk + 2 * plan.nreg)
                r = {"kernel": "region_reduce", "precision": prec, "ncol": n, "nfield": nf,
                     "nreg": plan.nreg, "nchunk": plan.nchunk, "membership": order,
                     "ms_per_call": ms, "ms_repeats": reps, "algorithmic_bytes": nbytes,
                     "achieved_gb_s": nbytes / (ms * 1e-3) / 1e9,
                     "hbm_frac": nbytes / (ms * 1e-3) / 1e9 / PEAK_GBS,
                     "hbm_frac_over_ldasout_grid": nbytes / (ms * 1e-3) / 1e9 / PEAK_GBS /
                     yard["hbm_frac"]}
                print(json.dumps(r), flush=True)
                rows.append(r)
                del plan
        eng.close()
    return rows


def write_case(d, out_every_s, ny, nx):
    import make_offline_case
    text = open(os.path.join(ROOT, "examples", "offline_case.nml")).read()
    for k in ("geo_em.d01.nc", "init.nc", "ldasin", "ldasout", "restart"):
        text = text.replace(f"'{k}'", f"'{os.path.join(d, k)}'").replace(
            f'"{k}"', f'"{os.path.join(d, k)}"')
    assert "'3 hour'" in text
    text = text.replace("'3 hour'", f"'{out_every_s} second'")
    nml = os.path.join(d, "case.nml")
    with open(nml, "w") as f:
        f.write(text)
    make_offline_case.main([nml, "--ny", str(ny), "--nx", str(nx), "--kind", "mixed"])
    cfg = config.Config(nml)
    grid, _, _ = ncio.read_static(cfg.constfile, Params.builtin().as_dict(), cfg.begdatetime)
    by, bx = max(ny // 8, 1), max(nx // 8, 1)
    reg = (np.arange(ny)[:, None] // by) * 8 + np.arange(nx)[None, :] // bx
    regfile = os.path.join(d, "regions.nc")
    ncio.write_region_map(regfile, grid, reg.astype(np.int32))
    return nml, regfile


def driver_timing(a):
    import torch
    os.makedirs(a.dir, exist_ok=True)
    nml, regfile = write_case(a.dir, a.out_every * 900, a.ny, a.nx)
    variants = {"a": dict(), "b": dict(regions=regfile),
                "c": dict(regions=regfile, write_grids=False)}
    out = []
    for prec in (4, 8):
        ms = {v: [] for v in variants}
        for p in range(a.passes):
            drv = {}
            for v, kw in variants.items():
                cfg = config.Config(nml)
                cfg.outdir = os.path.join(a.dir, f"out_{v}")
                drv[v] = driver.OfflineDriver.from_files(cfg, precision=prec, **kw)
                drv[v].run(nsteps=a.block)  # warm: kernels, pinned buffers, first files
            order = list(variants)
            for r in range((96 - a.block) // a.block):
                k = (r + p) % 3
                for v in order[k:] + order[:k]:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    drv[v].run(nsteps=a.block)
                    ms[v].append((time.perf_counter() - t0) / a.block * 1e3)
            for v in variants:
                drv[v].engine.close()
                for f in glob.glob(os.path.join(a.dir, f"out_{v}", "*_DOMAIN1")):
                    os.remove(f)
            del drv
        med = {v: float(np.median(ms[v])) for v in variants}
        r = {"precision": prec, "ncol": a.ny * a.nx, "out_every": a.out_every,
             "block_steps": a.block, "passes": a.passes, "nreg": 64, "nfield": L.NDIAG_OUT,
             "variants": {"a": "grids only", "b": "grids + regions", "c": "regions only"},
             "ms_per_step_median": med,
             "ms_per_step_min": {v: float(np.min(ms[v])) for v in variants},
             "ms_per_step_blocks": {v: [round(x, 4) for x in ms[v]] for v in variants},
             "b_over_a": med["b"] / med["a"], "c_over_a": med["c"] / med["a"]}
        print(json.dumps({k: r[k] for k in ("precision", "ms_per_step_median", "b_over_a",
                                            "c_over_a")}), flush=True)
        out.append(r)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--ncol", type=int, default=1 << 20)
    ap.add_argument("--nfield", type=int, default=len(L.DIAG_OUT_ACC))
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--ny", type=int, default=1024)
    ap.add_argument("--nx", type=int, default=1024)
    ap.add_argument("--out-every", type=int, default=6)
    ap.add_argument("--block", type=int, default=12, help="steps per timed block")
    ap.add_argument("--passes", type=int, default=3, help="fresh driver triples per precision")
    ap.add_argument("--dir", default=os.path.join(os.environ.get("TMPDIR", "/tmp"),
                                                  "nmp_regions_case"))
    ap.add_argument("--skip-kernel", action="store_true")
    ap.add_argument("--skip-driver", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "regions", "timing.json"))
    a = ap.parse_args(argv)
    import torch
    from noahmp_amd import lib as _nlib
    if not torch.cuda.is_available():
        sys.exit("regions_timing.py: no GPU (a timing is taken on the device or not at all)")
    assert a.block % a.out_every == 0, "whole output intervals per block"
    res = {"what": "nmp_region_reduce per call and the offline driver's ms per step with "
                   "region-aggregated output, variants interleaved on one device",
           "peak_gb_s": PEAK_GBS, "build_hash": _nlib.load().nmp_build_hash().decode()}
    if not a.skip_kernel:
        res["kernel"] = kernel_timing(a)
    if not a.skip_driver:
        res["driver"] = driver_timing(a)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
