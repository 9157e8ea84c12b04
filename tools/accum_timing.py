#!/usr/bin/env python3
"""What accumulated output costs per step, measured at config #3's size and
layout (1,048,576 mixed columns, fp32, two stream ranges, resident forcing,
output every 6 steps) through the engine's Python API.

    python tools/accum_timing.py [--out profiles/accum/timing.json]

Three variants of the same step loop, interleaved in rotating order over
`--rounds` rounds of `--steps` steps each on one device (host clock around
work that ends in a device synchronise):

  a  diagnostics on output steps only (what a run without accumulation does);
  b  every step at NMP_DIAG_OUT (non-output steps write a scratch block);
  c  b plus nmp_accumulate on every step and nmp_water_storage +
     nmp_accum_finish on output steps, on each range's stream after its step.

The accumulate kernel is also timed alone over all columns (device events),
and its achieved bandwidth reported against the bytes it moves: per column
17 reads of the engine's precision and 17 double accumulators read and
written (fp32: 68 B + 272 B).

The columns' physics do not depend on the variant, so the three share one
state, which simply keeps stepping; rotating the order spreads its drift over
the variants.  No threshold: the numbers are written down (DESIGN.md
"Accumulated output")."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import noahmp_pkg  # noqa: E402,F401
from noahmp_amd import cases, layout as L  # noqa: E402
from noahmp_amd.params import Params  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--ncol", type=int, default=1 << 20)
    ap.add_argument("--precision", type=int, default=4, choices=(4, 8))
    ap.add_argument("--steps", type=int, default=96, help="steps per timed block")
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--period", type=int, default=12, help="resident forcing slices (cycled)")
    ap.add_argument("--out-every", type=int, default=6)
    ap.add_argument("--dt", type=float, default=1800.0)
    ap.add_argument("--streams", type=int, default=2)
    ap.add_argument("--kernel-launches", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "accum", "timing.json"))
    a = ap.parse_args(argv)

    import torch
    from noahmp_amd import lib as _nlib
    from noahmp_amd.engine import ColumnState, Engine, StreamShards
    from noahmp_amd.order import coherent_order
    if not torch.cuda.is_available():
        sys.exit("accum_timing.py: no GPU (a timing is taken on the device or not at all)")
    P = Params.builtin("STAS", "USGS")
    julian0, yearlen, seed = 180.0, 366, 1000
    cols = cases.make_columns(a.ncol, "mixed", P.as_dict(), seed=seed, julian=julian0)
    cols = cols.take(coherent_order(cols.lon, cols.static_i, cols.isnow, "lon-snow-type",
                                    band_deg=4.0))
    dev = torch.device("cuda", 0)
    dtype = torch.float32 if a.precision == 4 else torch.float64
    eng = Engine(P, L.CASE_NML_OPTIONS, device=0, precision=a.precision)
    cs = ColumnState.from_host(cols, dev, dtype)
    n = cs.ncol
    F = torch.empty((a.period, L.NFORCING, n), dtype=dtype, device=dev)
    for s in range(a.period):
        F[s].copy_(torch.from_numpy(cases.forcing_step(
            cols, (julian0 + s * a.dt / 86400.0) % yearlen, yearlen, s, seed=seed)))
    del cols
    ranges = StreamShards(eng, cs, a.streams)
    zeros = lambda *shape, dt=dtype: torch.zeros(shape, dtype=dt, device=dev)  # noqa: E731
    out16 = [zeros(L.NDIAG_OUT, n) for _ in range(2)]
    out35 = [zeros(len(L.DIAG_OUT_ACC), n) for _ in range(2)]
    scratch = zeros(L.NDIAG_OUT, n)
    acc = zeros(L.NACC, n, dt=torch.float64)
    stor_beg, stor_end = zeros(n), zeros(n)
    eng.water_storage(cs, stor_beg)
    kstep = [0]  # the shared state's step count (forcing slice, day of year)

    def step(variant):
        k = kstep[0]
        kstep[0] += 1
        out = (k + 1) % a.out_every == 0
        jul = (julian0 + k * a.dt / 86400.0) % yearlen
        f = F[k % a.period]
        d, level, post = None, L.DIAG_NONE, None
        if variant == "a":
            if out:
                d, level = out16[(k // a.out_every) % 2], L.DIAG_OUT_LEVEL
        else:
            blk = out35[(k // a.out_every) % 2]
            d, level = blk[:L.NDIAG_OUT] if out else scratch, L.DIAG_OUT_LEVEL
        if variant == "c":
            def post(st, rng, d=d):
                eng.accumulate(d, f, acc, a.dt, stream=st, cols=rng)
                if out:
                    eng.water_storage(cs, stor_end, stream=st, cols=rng)
                    eng.accum_finish(acc, stor_end, stor_beg, blk[L.NDIAG_OUT:],
                                     a.out_every * a.dt, stream=st, cols=rng)
        ranges.step(f, cases.CASE_NML_ZSOIL, a.dt, jul, yearlen, d, level, post=post)

    def block(variant, steps):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(steps):
            step(variant)
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t0) / steps * 1e3

    variants = ["a", "b", "c"]
    assert a.steps % a.out_every == 0, "whole output intervals per block"
    for v in variants:  # warm every kernel and shape the timed blocks use
        block(v, 2 * a.out_every)
    ms = {v: [] for v in variants}
    for r in range(a.rounds):
        for v in variants[r % 3:] + variants[:r % 3]:
            ms[v].append(block(v, a.steps))

    # the accumulate kernel alone, all columns in one launch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    kern = []
    for _ in range(5):
        for _ in range(10):
            eng.accumulate(scratch, F[0], acc, a.dt)
        torch.cuda.synchronize(dev)
        e0.record()
        for _ in range(a.kernel_launches):
            eng.accumulate(scratch, F[0], acc, a.dt)
        e1.record()
        torch.cuda.synchronize(dev)
        kern.append(e0.elapsed_time(e1) / a.kernel_launches)
    kern_ms = float(np.median(kern))
    nbytes = n * (L.NACC * a.precision + 2 * L.NACC * 8)

    med = {v: float(np.median(ms[v])) for v in variants}
    res = {
        "what": "ms per step of the config #3 loop, variants interleaved on one device",
        "ncol": n, "precision": a.precision, "streams": a.streams, "out_every": a.out_every,
        "dt_s": a.dt, "steps_per_block": a.steps, "rounds": a.rounds,
        "variants": {"a": "diagnostics on output steps only",
                     "b": "NMP_DIAG_OUT every step",
                     "c": "b + accumulate every step, water_storage + finish on output steps"},
        "ms_per_step_median": med,
        "ms_per_step_min": {v: float(np.min(ms[v])) for v in variants},
        "ms_per_step_rounds": {v: [round(x, 5) for x in ms[v]] for v in variants},
        "b_over_a": med["b"] / med["a"], "c_over_a": med["c"] / med["a"],
        "accumulate_kernel": {"ms": kern_ms, "bytes": nbytes,
                              "bytes_per_column": nbytes // max(n, 1),
                              "GBps": nbytes / (kern_ms * 1e-3) / 1e9,
                              "launches": a.kernel_launches, "columns_per_lane": 1,
                              "ms_repeats": [round(x, 5) for x in kern]},
        "status_nonzero_cols": int((cs.status != 0).sum().item()),
        "build_hash": _nlib.load().nmp_build_hash().decode(),
    }
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({k: res[k] for k in ("ms_per_step_median", "b_over_a", "c_over_a",
                                          "accumulate_kernel")}))
    eng.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
