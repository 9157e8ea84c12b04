"""The short division without its fix-up (csrc/sflx_math.h DivFast32::divn).

divn is DivFast32::div minus the closing v_div_fixup_f32.  Inside div's exact
region (|b| in [2^-126, 2^126], a = 0 or |a| >= 2^-102, |a/b| in [2^-126,
2^126]) with finite operands the fix-up changes one case only: a = -0 with
b > 0, where the sequence gives +0 and IEEE gives -0.  tools/div_proof.py
shows the numerators of the sites that call divn never -0.

 (a) divn against the device's IEEE a / b as raw 32-bit patterns over the
     region: every exponent pair times 64 significand pairs times the four
     sign combinations, and significand sweeps at the region's exponent edges.
 (b) the zero numerators, pinned -- the one documented difference included.
 (c) the step kernel with the short divisions against the same kernel with
     IEEE division everywhere (Engine.option_set(0)), compared as uint32
     patterns, so a lost sign of zero shows (golden_io.bit_equal treats -0 and
     +0 as equal and would not notice).
 (d) the counting build: at no divn site of a lane that keeps its loop would
     the fix-up have changed a bit (tests/probe_div_nofix.py, a child process
     because it loads its own engine library).
"""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from golden_io import fixture_tags, load, single_names
from noahmp_amd import cases, layout as L

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
DN_LIB = os.path.join(HERE, "lib", "libnmp_div_nofix.so")
COUNT_LIB = os.path.join(ROOT, "noahmp-1_amd", "lib", "variants", "lib_count_libm.so")
DEV = "cuda:0"
PZ, NZ = 0x00000000, 0x80000000


@pytest.fixture(scope="module")
def dn():
    if not os.path.exists(DN_LIB):
        pytest.fail(f"{DN_LIB} missing: run __graft_entry__.build()")
    lib = C.CDLL(DN_LIB)
    u32 = np.ctypeslib.ndpointer(np.uint32, flags="C_CONTIGUOUS")
    u64p, u32p = C.POINTER(C.c_ulonglong), C.POINTER(C.c_uint)
    lib.dn_exp_pairs.argtypes = [C.c_uint, u32, u32, u64p, u32p]
    lib.dn_edge.argtypes = [C.c_int, C.c_int, C.c_uint, C.c_uint, C.c_uint, C.c_uint, u64p, u32p]
    lib.dn_eval.argtypes = [C.c_uint, u32, u32, u32, u32, u32]
    return lib


def significand_pairs():
    """64 pairs of 23-bit significands: the ends, the alternating patterns and
    their neighbours against each other, then seeded random pairs."""
    top = (1 << 23) - 1
    special = [0, 1, top, top - 1, 0x2AAAAA, 0x555555, 1 << 22, (1 << 22) - 1]
    pairs = [(x, y) for x in special[:6] for y in special[:6]]           # 36
    pairs += [(special[6], special[7]), (special[7], special[6]), (special[6], 0), (0, special[7])]
    rng = np.random.default_rng(20240611)
    while len(pairs) < 64:
        pairs.append(tuple(int(v) for v in rng.integers(0, 1 << 23, 2)))
    sa, sb = (np.array(v, np.uint32) for v in zip(*pairs))
    return sa, sb


# ---- (a) the primitive against IEEE ------------------------------------------
def test_divn_equals_ieee_over_every_exponent_pair(dn):
    """b over [2^-126, 2^126], a over [2^-102, 2^128), the pairs whose IEEE
    quotient lies in [2^-126, 2^126], 64 significand pairs, four sign
    combinations: 0 mismatches against a / b, and against DivFast32::div."""
    sa, sb = significand_pairs()
    assert sa.size == 64
    cnt, first = (C.c_ulonglong * 3)(), (C.c_uint * 2)()
    assert dn.dn_exp_pairs(sa.size, sa, sb, cnt, first) == 0
    print(f"divn over the exponent pairs: {cnt[0]} quotients in the region, {cnt[1]} differ from "
          f"IEEE, {cnt[2]} from div")
    # 253 x 230 exponent pairs; roughly 0.85 of them have an in-range quotient
    assert cnt[0] > 0.5 * 253 * 230 * 64 * 4
    assert cnt[1] == 0, f"first: a = 0x{first[0]:08x}, b = 0x{first[1]:08x}"
    assert cnt[2] == 0


# (ea, eb): a = m 2^ea, b = m' 2^eb at the edges of the region: the smallest
# and largest b, the smallest a, quotients at both ends of [2^-126, 2^126]
EDGES = [(-102, -126), (-102, 0), (-102, 23), (0, 126), (1, 126), (-1, 125), (0, -126), (-1, -126),
         (127, 1), (127, 2), (-126 + 24, 24), (0, 0)]


@pytest.mark.parametrize("ea,eb", EDGES)
def test_divn_equals_ieee_at_region_edges(dn, ea, eb):
    """Per edge: every a significand (signs alternating) against 128 b
    significands (every 65,536th, offset 32,769, both signs), and every b
    significand against 128 a significands: 2.1e9 pairs, less those whose
    quotient leaves the region."""
    tot = [0, 0, 0]
    for sta, oa, stb, ob in ((1, 0, 65536, 32769), (65536, 32769, 1, 0)):
        cnt, first = (C.c_ulonglong * 3)(), (C.c_uint * 2)()
        assert dn.dn_edge(ea, eb, sta, oa, stb, ob, cnt, first) == 0
        assert cnt[1] == 0, f"(2^{ea}, 2^{eb}): {cnt[1]} differ from IEEE, first a = " \
                            f"0x{first[0]:08x}, b = 0x{first[1]:08x}"
        assert cnt[2] == 0
        for i in range(3):
            tot[i] += cnt[i]
    print(f"divn at (2^{ea}, 2^{eb}): {tot[0]} pairs in the region, {tot[1]} differ from IEEE")
    assert tot[0] > 0


# ---- (b) the zero numerators ----------------------------------------------------
def _b_values():
    """Denominators over the region, both signs: the ends, 1, and random ones."""
    rng = np.random.default_rng(7)
    e = np.concatenate([[-126, -126, 126, 0, 0, 1, -1], rng.integers(-126, 126, 249)])
    m = np.concatenate([[0, (1 << 23) - 1, 0, 0, 1, 0x2AAAAA, 0x555555],
                        rng.integers(0, 1 << 23, 249)])
    pos = ((e + 127).astype(np.uint32) << np.uint32(23)) | m.astype(np.uint32)
    return pos, pos | np.uint32(NZ)


def _eval(dn, a, b):
    a, b = np.ascontiguousarray(a, np.uint32), np.ascontiguousarray(b, np.uint32)
    qn, qd, qi = (np.zeros(a.size, np.uint32) for _ in range(3))
    assert dn.dn_eval(a.size, a, b, qn, qd, qi) == 0
    return qn, qd, qi


def test_zero_numerators_pinned(dn):
    bp, bn = _b_values()
    full = lambda v: np.full(bp.size, v, np.uint32)
    # +0 / b: IEEE for both signs of b
    for b, want in ((bp, PZ), (bn, NZ)):
        qn, qd, qi = _eval(dn, full(PZ), b)
        assert (qi == want).all() and (qd == want).all()
        assert (qn == want).all(), "divn(+0, b) is not IEEE's zero"
    # -0 / b, b < 0: +0, as IEEE
    qn, qd, qi = _eval(dn, full(NZ), bn)
    assert (qi == PZ).all() and (qd == PZ).all() and (qn == PZ).all()
    # -0 / b, b > 0: IEEE and div give -0, divn gives +0 -- the documented
    # difference, and the reason a divn site needs a numerator that is never -0
    qn, qd, qi = _eval(dn, full(NZ), bp)
    assert (qi == NZ).all() and (qd == NZ).all()
    assert (qn == PZ).all(), "divn(-0, b > 0) changed: the region in sflx_math.h must follow"


def test_divn_equals_div_on_random_region_pairs(dn):
    """On the same kind of inputs as (a), element by element: wherever the pair
    lies in the region, divn == div == IEEE."""
    rng = np.random.default_rng(11)
    n = 1 << 18
    a = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    b = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    qn, qd, qi = _eval(dn, a, b)
    with np.errstate(all="ignore"):
        af, bf = a.view(np.float32).astype(np.float64), b.view(np.float32).astype(np.float64)
        w = np.abs(af / bf)
        inside = (np.isfinite(af) & np.isfinite(bf) & (np.abs(bf) >= 2.0 ** -126)
                  & (np.abs(bf) <= 2.0 ** 126) & (np.abs(af) >= 2.0 ** -102)
                  & (w >= 2.0 ** -126 * (1 + 2.0 ** -20)) & (w <= 2.0 ** 126 * (1 - 2.0 ** -20)))
    assert inside.sum() > n // 4
    assert (qn[inside] == qi[inside]).all() and (qn[inside] == qd[inside]).all()


# ---- (c) the step kernel, sign of zero included ---------------------------------
# Fields whose zero sign already differs between the short-division kernels and
# the IEEE kernel in the parent build: none (the comparison below, run on the
# parent's library, matched on every field).
PARENT_ZERO_SIGN_DIFFERS = ()
LEVELS = {"none": (L.DIAG_NONE, 0), "out": (L.DIAG_OUT_LEVEL, L.NDIAG_OUT),
          "full": (L.DIAG_FULL_LEVEL, L.NDIAG_FULL)}


@pytest.fixture(scope="module")
def engines(engine_lib):
    from noahmp_amd.engine import Engine
    from noahmp_amd.params import Params
    cache, tables = {}, {}

    def get(options, tags, variant, generic):
        key = (tuple(int(x) for x in options), tuple(tags), variant, generic)
        if key not in cache:
            if tags not in tables:
                tables[tags] = Params.builtin(*tags)
            e = Engine(tables[tags], dict(zip(L.OPTION_NAMES, key[0])), device=0, precision=4)
            assert e.launch_variant(variant) == variant
            if generic:
                assert e.option_set(0) == 0
            cache[key] = e
        return cache[key]
    yield get
    for e in cache.values():
        e.close()


def _column_state(g):
    from noahmp_amd.engine import ColumnState
    cols = cases.ColumnSet(g["static_f"], g["static_i"], g["state0"], g["isnow0"], *([None] * 7))
    return ColumnState.from_host(cols, DEV)


def _same_patterns(x, y, what):
    """x, y: float32 tensors; equal as uint32 patterns except where both are NaN."""
    x, y = x.cpu().numpy(), y.cpu().numpy()
    bad = (x.view(np.uint32) != y.view(np.uint32)) & ~(np.isnan(x) & np.isnan(y))
    if bad.any():
        rows = sorted(set(np.nonzero(bad)[0].tolist())) if bad.ndim > 1 else []
        zero = bool(((x[bad] == 0) & (y[bad] == 0)).all())
        pytest.fail(f"{what}: {int(bad.sum())} elements differ (rows {rows[:12]}); "
                    f"{'all of them zeros of opposite sign' if zero else 'not only zero signs'}")


@pytest.mark.parametrize("variant,level", [("full", "none"), ("full", "full"), ("small", "full")])
@pytest.mark.parametrize("name", single_names())
def test_single_call_short_vs_ieee_division_patterns(engines, name, variant, level):
    g = load(f"single_{name}.npz")
    f = torch.as_tensor(g["forcing"], device=DEV).contiguous()
    lvl, nd = LEVELS[level]
    res = []
    for generic in (False, True):
        eng = engines(g["options"], fixture_tags(g), variant, generic)
        cs = _column_state(g)
        d = torch.zeros((nd, cs.ncol), device=DEV) if nd else None
        eng.step(cs, f, g["zsoil"], float(g["dt"]), float(g["julian"]), int(g["yearlen"]), d, lvl)
        torch.cuda.synchronize()
        res.append((cs, d))
    (a, da), (b, db) = res
    _same_patterns(a.state, b.state, f"{name} state")
    assert torch.equal(a.isnow, b.isnow) and torch.equal(a.status, b.status)
    if nd:
        _same_patterns(da, db, f"{name} diagnostics")


@pytest.mark.parametrize("name", ["casenml", "snow"])
def test_trajectory_short_vs_ieee_division_patterns(engines, name):
    """The reference trajectories stepped NONE, NONE, OUT: state, ISNOW, status
    and the OUT steps' diagnostics after every step."""
    g = load(f"traj_{name}.npz")
    F = torch.as_tensor(g["forcing"], device=DEV).contiguous()
    dt, yl, nstep = float(g["dt"]), int(g["yearlen"]), F.shape[0]
    runs = []
    for generic in (False, True):
        eng = engines(g["options"], ("STAS", "USGS"), "full", generic)
        if not generic:
            assert eng.option_set() == 1
        cs = _column_state(g)
        d = torch.zeros((L.NDIAG_OUT, cs.ncol), device=DEV)
        snaps = []
        for s in range(nstep):
            out = s % 3 == 2
            jul = float(g["julian0"]) + s * dt / 86400.0
            eng.step(cs, F[s], g["zsoil"], dt, jul, yl, d if out else None,
                     L.DIAG_OUT_LEVEL if out else L.DIAG_NONE)
            snaps.append((cs.state.clone(), cs.isnow.clone(), cs.status.clone(),
                          d.clone() if out else None))
        torch.cuda.synchronize()
        runs.append(snaps)
    for s, (x, y) in enumerate(zip(*runs)):
        _same_patterns(x[0], y[0], f"traj_{name} step {s} state")
        assert torch.equal(x[1], y[1]) and torch.equal(x[2], y[2]), f"step {s}"
        if x[3] is not None:
            _same_patterns(x[3], y[3], f"traj_{name} step {s} diagnostics")


# ---- (d) the counting build ---------------------------------------------------------
def test_fixup_would_change_no_quotient_of_a_kept_loop():
    if not os.path.exists(COUNT_LIB):
        pytest.fail(f"counting library missing ({COUNT_LIB}): run __graft_entry__.build()")
    env = dict(os.environ, NOAHMP_ENGINE_LIB=COUNT_LIB)
    r = subprocess.run([sys.executable, os.path.join(HERE, "probe_div_nofix.py")], env=env,
                       capture_output=True, text=True, timeout=110)
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert line, f"probe produced no result (rc {r.returncode}): {r.stderr[-2000:]}"
    res = json.loads(line[-1])
    for run in res["runs"]:
        print(run)
    assert "error" not in res, res
    assert res["changed"] == 0, [run for run in res["runs"]
                                 if any(run[g][1] for g in ("canopy", "bare", "soil", "atan"))]
    # every group of sites formed quotients, and the dry-clay set took the IEEE arm
    assert min(res["formed"].values()) > 0, res["formed"]
    assert res["runs"][-1]["case"] == "dry clay" and res["runs"][-1]["soil_ieee_divisions"] > 0
    assert r.returncode == 0 and res["ok"]
