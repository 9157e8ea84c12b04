"""The libm windows of the Newton loops (run by tests/test_gpu_libm_inrange.py in
a child process, once per library).

Under DivFast32 the canopy and bare loops call the in-range cores of
csrc/glibc_math.h behind per-lane windows on MOZ / MOZ2 (sfcdif1) and MOZG
(ragrb); a lane outside one re-runs its loop with DivRef and the full
functions.  Two libraries built by __graft_entry__.build() from the shipped
sources with NMP_COUNT_FALLBACK:

  lib_probe_libm.so   windows narrowed (MOZ, MOZ2 >= -0.2, MOZG >= -0.02):
                      unstable columns leave through them from the second
                      iteration on, after the fast loop has changed
                      TV/TAH/EAH/QSFC       -> `--expect fire`
  lib_count_libm.so   the shipped windows   -> `--expect none`

Inputs: 8,192 "mixed" columns, seeds 31 and 32, one step; both occupancy
variants, diagnostics levels none and full (full runs the 2-m chain: MOZ2).
Every column must equal the C restatement of the reference bit for bit.  With
`fire` each new counter (fb_why bits 32, 33, 34) must be non-zero in every
run; with `none` each must be zero.

    NOAHMP_ENGINE_LIB=.../lib_probe_libm.so python tests/probe_libm.py --expect fire

Prints one JSON line; exit status 0 when every check passed.
"""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import noahmp_pkg  # noqa: E402,F401
from golden_io import bit_equal, load_params  # noqa: E402
from noahmp_amd import cases, layout as L, lib  # noqa: E402
from noahmp_amd.engine import ColumnState, Engine  # noqa: E402
from noahmp_amd.params import Params  # noqa: E402
import port  # noqa: E402  (the oracle: the checker)

# the new fb_why bits (sflx_kernel.hip NMP_DOM)
NEW = {32: "MOZ/MOZ2 window (canopy)", 33: "MOZG window", 34: "MOZ/MOZ2 window (bare)"}


def main():
    expect = sys.argv[sys.argv.index("--expect") + 1]
    assert expect in ("fire", "none")
    raw = lib.load()
    if not hasattr(raw, "nmp_debug_fallback_reasons"):
        print(json.dumps({"error": f"{lib.library_path()} is not a counting build"}))
        return 2
    raw.nmp_debug_fallback_count.restype = C.c_longlong
    raw.nmp_debug_fallback_count.argtypes = [C.c_int, C.c_void_p]
    raw.nmp_debug_fallback_reasons.argtypes = [C.c_void_p]
    P = Params.builtin("STAS", "USGS")
    opts = [L.CASE_NML_OPTIONS[k] for k in L.OPTION_NAMES]
    n, jul, dt, yl = 8192, 180.3, 1800.0, 366
    res = {"ncol": n, "expect": expect, "runs": []}
    ok_all = True
    for seed in (31, 32):
        cols = cases.make_columns(n, "mixed", P.as_dict(), seed=seed, julian=180.0)
        f = cases.forcing_step(cols, jul, yl, 0, seed=seed)
        est, eisn, edg, _ = port.step(load_params(), tuple(opts), cases.CASE_NML_ZSOIL, dt, yl,
                                      jul, cols.state, cols.isnow, cols.static_f, cols.static_i, f)
        for variant in ("small", "full"):
            for level in ("none", "full"):
                eng = Engine(P, L.CASE_NML_OPTIONS, device=0)
                assert eng.launch_variant(variant) == variant
                cs = ColumnState.from_host(cols, "cuda:0")
                raw.nmp_debug_fallback_count(1, None)
                if level == "full":
                    diag = torch.zeros((L.NDIAG_FULL, n), device="cuda:0")
                    eng.step(cs, torch.as_tensor(f, device="cuda:0"), cases.CASE_NML_ZSOIL, dt,
                             jul, yl, diag, L.DIAG_FULL_LEVEL)
                else:
                    eng.step(cs, torch.as_tensor(f, device="cuda:0"), cases.CASE_NML_ZSOIL, dt,
                             jul, yl)
                torch.cuda.synchronize()
                why = np.zeros(64, np.uint32)
                assert raw.nmp_debug_fallback_reasons(why.ctypes.data) == 0
                fb = int(raw.nmp_debug_fallback_count(0, None))
                ok = bit_equal(cs.state.cpu().numpy(), est).all(0) & \
                    (cs.isnow.cpu().numpy() == eisn)
                if level == "full":
                    ok &= bit_equal(diag.cpu().numpy(), edg).all(0)
                eng.close()
                run = {"seed": seed, "variant": variant, "diag": level, "fallbacks": fb,
                       "windows": {NEW[b]: int(why[b]) for b in NEW},
                       "columns_differing": int((~ok).sum())}
                res["runs"].append(run)
                fired = all(why[b] > 0 for b in NEW)
                none = all(why[b] == 0 for b in NEW)
                ok_all = ok_all and bool(ok.all()) and (fired if expect == "fire" else none)
    res["ok"] = ok_all
    print(json.dumps(res))
    return 0 if ok_all else 1


if __name__ == "__main__":
    sys.exit(main())
