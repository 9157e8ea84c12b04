"""The counting evidence for the fix-up-free short divisions (run by
tests/test_gpu_div_nofix.py in a child process, because it loads its own engine
library).

lib_count_libm.so (built by __graft_entry__.build(): the shipped sources with
NMP_COUNT_FALLBACK) forms v_div_fixup_f32's result beside every quotient of
DivFast32::divn (csrc/sflx_math.h) whose lane keeps its loop, and counts per
group of sites (canopy loop with its stomata bisection, bare loop, soil
sub-steps, atanf_ge1) the quotients formed and those whose bits the fix-up
would have changed (nmp_fb_reason 50..57).  The second count must be 0:

  every single-call fixture, one step at diagnostics level full;
  4,096 "mixed" columns (every 7th bare ground) over 8 steps, NONE / OUT;
  the dry-clay set of tests/probe_midloop.py: WDF * DDZ below 2^-102 sends
  soil sub-step divisions to the IEEE arm (counter 25 > 0), which must not
  count as divn quotients.

    NOAHMP_ENGINE_LIB=.../lib_count_libm.so python tests/probe_div_nofix.py

Prints one JSON line; exit status 0 when every check passed.
"""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import noahmp_pkg  # noqa: E402,F401
from golden_io import fixture_tags, load, single_names  # noqa: E402
from noahmp_amd import cases, layout as L, lib  # noqa: E402
from noahmp_amd.engine import ColumnState, Engine  # noqa: E402
from noahmp_amd.params import Params  # noqa: E402

GROUPS = ("canopy", "bare", "soil", "atan")
DEV = "cuda:0"


def main():
    raw = lib.load()
    if not hasattr(raw, "nmp_debug_fallback_reasons"):
        print(json.dumps({"error": f"{lib.library_path()} is not a counting build"}))
        return 2
    raw.nmp_debug_fallback_count.restype = C.c_longlong
    raw.nmp_debug_fallback_count.argtypes = [C.c_int, C.c_void_p]
    raw.nmp_debug_fallback_reasons.argtypes = [C.c_void_p]

    def counters():
        torch.cuda.synchronize()
        why = np.zeros(64, np.uint32)
        assert raw.nmp_debug_fallback_reasons(why.ctypes.data) == 0
        raw.nmp_debug_fallback_count(1, None)
        run = {g: [int(why[50 + 2 * i]), int(why[51 + 2 * i])] for i, g in enumerate(GROUPS)}
        run["soil_ieee_divisions"] = int(why[25])
        return run

    res = {"runs": []}
    tables = {}
    raw.nmp_debug_fallback_count(1, None)
    # ---- the single-call fixtures ----
    for name in single_names():
        g = load(f"single_{name}.npz")
        tags = fixture_tags(g)
        if tags not in tables:
            tables[tags] = Params.builtin(*tags)
        eng = Engine(tables[tags], dict(zip(L.OPTION_NAMES, (int(x) for x in g["options"]))),
                     device=0, precision=4)
        cols = cases.ColumnSet(g["static_f"], g["static_i"], g["state0"], g["isnow0"], *([None] * 7))
        cs = ColumnState.from_host(cols, DEV)
        d = torch.zeros((L.NDIAG_FULL, cs.ncol), device=DEV)
        eng.step(cs, torch.as_tensor(g["forcing"], device=DEV).contiguous(), g["zsoil"],
                 float(g["dt"]), float(g["julian"]), int(g["yearlen"]), d, L.DIAG_FULL_LEVEL)
        run = counters()
        run.update(case=f"single_{name}", option_set=int(eng.option_set()))
        eng.close()
        res["runs"].append(run)
    # ---- 4,096 mixed columns, 8 steps ----
    P = Params.builtin("STAS", "USGS")
    tab = P.as_dict()
    n = 4096
    cols = cases.make_columns(n, "mixed", tab, seed=21, julian=95.0)
    cols.static_i[L.STATIC_I.index("VEGTYP")][::7] = tab["isbarren"]
    eng = Engine(P, L.CASE_NML_OPTIONS, device=0, precision=4)
    assert eng.launch_variant("full") == "full" and eng.option_set() == 1
    cs = ColumnState.from_host(cols, DEV)
    d = torch.zeros((L.NDIAG_OUT, n), device=DEV)
    for s in range(8):
        jul = 95.0 + s / 48.0
        f = torch.as_tensor(cases.forcing_step(cols, jul, 365, s, seed=21), device=DEV)
        out = s % 2 == 1
        eng.step(cs, f, cases.CASE_NML_ZSOIL, 1800.0, jul, 365, d if out else None,
                 L.DIAG_OUT_LEVEL if out else L.DIAG_NONE)
    run = counters()
    run.update(case="mixed 4096 x 8", option_set=1)
    eng.close()
    res["runs"].append(run)
    # ---- dry clay: soil sub-step divisions on the IEEE arm ----
    cols = cases.make_columns(n, "mixed", tab, seed=41, julian=180.0)
    dry = np.arange(n) % 2 == 0
    cols.static_i[L.STATIC_I.index("SOILTYP")][dry] = 12
    for fld in ("SH2O", "SMC"):
        st = cols.state[L.s(fld)]
        st[:, dry] = np.float32(0.001) + np.float32(0.0001) * np.arange(4)[:, None]
    eng = Engine(P, L.CASE_NML_OPTIONS, device=0, precision=4)
    assert eng.option_set() == 1
    cs = ColumnState.from_host(cols, DEV)
    f = torch.as_tensor(cases.forcing_step(cols, 180.3, 366, 0, seed=41), device=DEV)
    eng.step(cs, f, cases.CASE_NML_ZSOIL, 1800.0, 180.3, 366)
    run = counters()
    run.update(case="dry clay", option_set=1)
    eng.close()
    res["runs"].append(run)

    changed = sum(run[g][1] for run in res["runs"] for g in GROUPS)
    formed = {g: sum(run[g][0] for run in res["runs"]) for g in GROUPS}
    res["formed"], res["changed"] = formed, changed
    res["ok"] = bool(changed == 0 and min(formed.values()) > 0
                     and res["runs"][-1]["soil_ieee_divisions"] > 0)
    print(json.dumps(res))
    return 0 if res["ok"] else 1


if __name__ == "__main__":
    sys.exit(main())
