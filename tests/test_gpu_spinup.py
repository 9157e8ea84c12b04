"""Spin-up on the GPU: nmp_state_drift and nmp_drift_reduce against their numpy
twins (spinup.tracked_host / drift_host / reduce_host, themselves held to a
restatement of the header in tests/test_spinup_host.py) bit for bit, and the
offline driver's spinup(): the state after the loops against a chain of fresh
drivers, the drift history against the twins applied to the chain's end
states, no output during spin-up, the production run afterwards, the early
stop, a run from files with interpolated forcing, the report, the drift map,
the CLI and two ranks.

Every comparison is on bits."""
import ctypes as C
import glob
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

import noahmp_pkg  # noqa: F401  (spawned ranks re-import this module)
from noahmp_amd import cases, config, driver, layout as L, ncio, spinup, timeman
from noahmp_amd.engine import ColumnState, Engine
from noahmp_amd.params import Params
from noahmp_amd.regions import area_weights
from test_spinup_host import NCOLS, check_result, planted
from test_stateout_host import make_columns, same_bits

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NCOL, LD, LD_SNAP, LD_DRIFT = 777, 800, 784, 792       # three blocks plus 9 lanes
RANGES = ((0, 293), (293, 777))
SENTINEL = -31337.0
G = L.DRIFT_GROUPS.index
# the state rows the header names: the kernel reads these and no others
READS = sorted([L.si("SMC") + k for k in range(4)] + [L.si("STC") + k for k in range(3, 7)] +
               [L.si(n) for n in ("SNEQV", "WA", "ZWT", "CANLIQ", "CANICE")] +
               [L.si("ZSNSO") + k for k in range(2, 7)] + [L.si(p) for p in L.CARBON_POOLS])
assert len(READS) == 24


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda:0")


def _engine(precision):
    return Engine(Params.builtin(), L.CASE_NML_OPTIONS, device=0, precision=precision)


def _np(precision):
    return np.float32 if precision == 4 else np.float64


def _raw_drift(eng, state, isnow, static_i, snap, drift, lo, hi, stream=None):
    """nmp_state_drift through the C ABI for columns lo..hi-1 (pointers offset by lo)."""
    s = stream if stream is not None else torch.cuda.current_stream(0)
    p = lambda t: C.c_void_p(t.data_ptr() + lo * t.element_size())  # noqa: E731
    return eng._lib.nmp_state_drift(eng._h, hi - lo, LD, p(state), p(isnow), p(static_i), p(snap),
                                    LD_SNAP, p(drift) if drift is not None else None, LD_DRIFT,
                                    C.c_void_p(s.cuda_stream))


# ---- 1. the per-column kernel ----------------------------------------------------------
@pytest.mark.parametrize("split", [False, True], ids=["whole", "two-ranges"])
@pytest.mark.parametrize("precision", [4, 8])
def test_kernel_equals_the_twin(engine_lib, precision, split):
    eng = _engine(precision)
    dtype = _np(precision)
    s0, isnow, static_i = make_columns(dtype, n=NCOL, ld=LD, seed=precision)
    s1, isnow1, _ = make_columns(dtype, n=NCOL, ld=LD, seed=precision + 10)
    isnow1 = np.roll(isnow1, 1)                              # the snow pack moved, too
    t0 = spinup.tracked_host(s0[:, :NCOL], isnow[:NCOL], static_i[:, :NCOL])
    t1 = spinup.tracked_host(s1[:, :NCOL], isnow1[:NCOL], static_i[:, :NCOL])
    want = spinup.drift_host(t1, t0)
    assert np.isnan(want[G("CARBON")]).any() and (want[G("TWS")] == 0).any()
    sid = _dev(static_i)
    streams = [torch.cuda.Stream(0), torch.cuda.Stream(0)]

    def call(state, isn, snap, drift):
        if split:
            for st, (lo, hi) in zip(streams, RANGES):
                st.wait_stream(torch.cuda.current_stream(0))
                assert _raw_drift(eng, state, isn, sid, snap, drift, lo, hi, st) == 0
                torch.cuda.current_stream(0).wait_stream(st)
        else:
            assert _raw_drift(eng, state, isn, sid, snap, drift, 0, NCOL) == 0
        torch.cuda.synchronize()

    def poisoned(state):     # the rows the header does not name are NaN: a load of one would show
        p = np.full_like(state, np.nan)
        p[READS] = state[READS]
        return p

    for a, b in ((s0, s1), (poisoned(s0), poisoned(s1))):
        snap = torch.full((L.NTRACKED + 2, LD_SNAP), SENTINEL, device="cuda:0",
                          dtype=torch.float32 if precision == 4 else torch.float64)
        drift = torch.full((L.NDRIFT + 2, LD_DRIFT), SENTINEL, dtype=snap.dtype, device="cuda:0")
        # drift = NULL only snapshots (the sentinel in snap is never read)
        call(_dev(a), _dev(isnow), snap, None)
        got = snap.cpu().numpy()
        assert same_bits(got[:L.NTRACKED, :NCOL], t0)
        assert (got[:, NCOL:] == SENTINEL).all() and (got[L.NTRACKED:] == SENTINEL).all()
        assert (drift.cpu().numpy() == SENTINEL).all()
        # one launch measures the loop and arms the next
        call(_dev(b), _dev(isnow1), snap, drift)
        got, gd = snap.cpu().numpy(), drift.cpu().numpy()
        for g, name in enumerate(L.DRIFT_GROUPS):
            assert same_bits(gd[g, :NCOL], want[g]), name
        assert same_bits(got[:L.NTRACKED, :NCOL], t1)
        # tails and rows beyond keep the sentinel
        assert (got[:, NCOL:] == SENTINEL).all() and (got[L.NTRACKED:] == SENTINEL).all()
        assert (gd[:, NCOL:] == SENTINEL).all() and (gd[L.NDRIFT:] == SENTINEL).all()
        # the same state again: no drift, +0.0 (NaN where the tracked value is NaN)
        call(_dev(b), _dev(isnow1), snap, drift)
        assert same_bits(drift.cpu().numpy()[:L.NDRIFT, :NCOL], spinup.drift_host(t1, t1))
    eng.close()


@pytest.mark.parametrize("precision", [4, 8])
def test_front_end(engine_lib, precision):
    eng = _engine(precision)
    dtype = _np(precision)
    state, isnow, static_i = make_columns(dtype, n=NCOL, ld=LD, seed=3)
    sd, idv, sid = _dev(state), _dev(isnow), _dev(static_i)
    snap = torch.full((L.NTRACKED, LD_SNAP), SENTINEL, dtype=sd.dtype, device="cuda:0")
    drift = torch.full((L.NDRIFT, LD_DRIFT), SENTINEL, dtype=sd.dtype, device="cuda:0")
    s = C.c_void_p(torch.cuda.current_stream(0).cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    lib, h = eng._lib, eng._h
    # NMP_E_ARG: a leading dimension below ncol, a NULL array; ncol == 0 is a no-op
    assert lib.nmp_state_drift(h, NCOL, NCOL - 1, p(sd), p(idv), p(sid), p(snap), LD_SNAP,
                               p(drift), LD_DRIFT, s) == -1
    assert lib.nmp_state_drift(h, NCOL, LD, p(sd), p(idv), p(sid), p(snap), NCOL - 1, p(drift),
                               LD_DRIFT, s) == -1
    assert lib.nmp_state_drift(h, NCOL, LD, p(sd), p(idv), p(sid), p(snap), LD_SNAP, p(drift),
                               NCOL - 1, s) == -1
    assert lib.nmp_state_drift(h, NCOL, LD, p(sd), p(idv), p(sid), None, LD_SNAP, p(drift),
                               LD_DRIFT, s) == -1
    assert lib.nmp_state_drift(h, -1, LD, p(sd), p(idv), p(sid), p(snap), LD_SNAP, None, 0, s) == -1
    assert lib.nmp_state_drift(h, 0, LD, p(sd), p(idv), p(sid), p(snap), LD_SNAP, p(drift),
                               LD_DRIFT, s) == 0
    torch.cuda.synchronize()
    assert (snap.cpu().numpy() == SENTINEL).all() and (drift.cpu().numpy() == SENTINEL).all()
    # the binding: its neighbours' shape, dtype and device checks, and a cols range
    cs = ColumnState(_dev(state[:, :NCOL]), _dev(isnow[:NCOL]),
                     torch.zeros((L.NSTATIC_F, NCOL), dtype=sd.dtype, device="cuda:0"),
                     _dev(static_i[:, :NCOL]), torch.zeros(NCOL, dtype=torch.int32, device="cuda:0"))
    sn = torch.full((L.NTRACKED, NCOL), SENTINEL, dtype=sd.dtype, device="cuda:0")
    dr = torch.full((L.NDRIFT, NCOL), SENTINEL, dtype=sd.dtype, device="cuda:0")
    for bad_snap, bad_drift in ((sn[:-1], dr), (sn.cpu(), dr), (sn, dr[:-1]), (sn, dr.cpu()),
                                (sn.to(torch.float16), dr), (sn, dr.to(torch.float16))):
        with pytest.raises(AssertionError):
            eng.state_drift(cs, bad_snap, bad_drift)
    eng.state_drift(cs, sn, cols=(100, 300))
    torch.cuda.synchronize()
    t = spinup.tracked_host(state[:, :NCOL], isnow[:NCOL], static_i[:, :NCOL])
    got = sn.cpu().numpy()
    assert same_bits(got[:, 100:300], t[:, 100:300])
    assert (got[:, :100] == SENTINEL).all() and (got[:, 300:] == SENTINEL).all()
    assert (dr.cpu().numpy() == SENTINEL).all()
    with pytest.raises(AssertionError):
        eng.drift_reduce(dr[:-1], np.zeros(7))
    with pytest.raises(AssertionError):
        eng.drift_reduce(dr, np.zeros(6))
    with pytest.raises(AssertionError):
        eng.drift_reduce(dr, np.zeros(7), weight=torch.ones(NCOL, device="cuda:0"))   # not double
    # nmp_drift_reduce: NMP_E_ARG, and ncol == 0 writes the empty result
    part = torch.zeros(L.DRIFT_SCRATCH * 4, dtype=torch.int64, device="cuda:0")
    out = torch.full((4 * L.NDRIFT + 1,), 7, dtype=torch.int64, device="cuda:0")
    tol = torch.zeros(L.NDRIFT, dtype=torch.float64, device="cuda:0")
    o = lambda k: C.c_void_p(out.data_ptr() + 8 * k * L.NDRIFT)  # noqa: E731
    args = lambda n, ld, d=p(drift), t=p(tol), pt=p(part), o0=o(0): (  # noqa: E731
        h, n, ld, d, None, t, pt, o0, o(1), o(2), o(3), o(4), s)
    assert lib.nmp_drift_reduce(*args(NCOL, NCOL - 1)) == -1
    assert lib.nmp_drift_reduce(*args(-1, LD_DRIFT)) == -1
    for null in ("d", "t", "pt", "o0"):
        assert lib.nmp_drift_reduce(*args(NCOL, LD_DRIFT, **{null: None})) == -1
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 7).all()
    assert lib.nmp_drift_reduce(*args(0, LD_DRIFT)) == 0
    torch.cuda.synchronize()
    g = L.NDRIFT
    want = np.zeros(4 * g + 1, np.int64)
    want[g:2 * g] = -1
    assert np.array_equal(out.cpu().numpy(), want)
    eng.close()


# ---- 2. the reduction ------------------------------------------------------------------
@pytest.mark.parametrize("precision", [4, 8])
def test_reduction_equals_the_twin(engine_lib, precision):
    eng = _engine(precision)
    dtype = _np(precision)
    for n in NCOLS:
        d, w, tol = planted(dtype, n, seed=n)
        dd, wd = _dev(d), _dev(w)
        for weight, wdev in ((w, wd), (None, None)):
            res = eng.drift_reduce(dd, tol, wdev)
            want = spinup.reduce_host(d, tol, weight)
            check_result(res, (want.max, want.arg, want.wsum, want.count, want.wtot))
            assert same_bits(res.mean, want.mean)
        if n >= 63:
            assert res.arg[G("SNEQV")] == 17 and res.arg[G("TWS")] == 9    # (the unweighted call)
        # every column skipped
        res = eng.drift_reduce(dd, tol, torch.zeros_like(wd))
        assert (res.arg == -1).all() and not res.count.any() and res.wtot == 0.0
    # a leading dimension above ncol, through the C ABI: the pad columns hold NaN
    n = NCOL
    d, w, tol = planted(dtype, n, seed=5)
    pad = np.full((L.NDRIFT, LD_DRIFT), np.nan, dtype)
    pad[:, :n] = d
    dd, wd, td = _dev(pad), _dev(w), _dev(tol)
    part = torch.zeros(L.DRIFT_SCRATCH * 4, dtype=torch.int64, device="cuda:0")
    out = torch.zeros(4 * L.NDRIFT + 1, dtype=torch.int64, device="cuda:0")
    p = lambda t, k=0: C.c_void_p(t.data_ptr() + 8 * k)  # noqa: E731
    g = L.NDRIFT
    assert eng._lib.nmp_drift_reduce(eng._h, n, LD_DRIFT, p(dd), p(wd), p(td), p(part), p(out),
                                     p(out, g), p(out, 2 * g), p(out, 3 * g), p(out, 4 * g),
                                     C.c_void_p(torch.cuda.current_stream(0).cuda_stream)) == 0
    torch.cuda.synchronize()
    h = out.cpu().numpy()
    want = spinup.reduce_host(d, tol, w)
    got = spinup.DriftResult(h[:g].view(np.float64), h[g:2 * g], h[2 * g:3 * g].view(np.float64),
                             h[3 * g:4 * g], float(h[4 * g:].view(np.float64)[0]))
    check_result(got, (want.max, want.arg, want.wsum, want.count, want.wtot))
    eng.close()


# ---- 3. the driver, synthetic columns --------------------------------------------------
def _nml(tmp, dt=3600):
    tmp.mkdir(exist_ok=True)
    text = open(os.path.join(ROOT, "examples", "offline_case.nml")).read()
    for k in ("geo_em.d01.nc", "init.nc", "ldasin", "ldasout", "restart"):
        text = text.replace(f"'{k}'", f"'{tmp / k}'").replace(f'"{k}"', f'"{tmp / k}"')
    text = text.replace("interval_seconds = 900", f"interval_seconds = {dt}")
    nml = tmp / "case.nml"
    nml.write_text(text)
    return str(nml)


def _files(outdir):
    return sorted(os.listdir(outdir)) if os.path.isdir(outdir) else []


def _set_state(drv, state, isnow):
    """Start `drv` from (state, isnow): a fresh driver from another's final state."""
    drv.cs.state.copy_(_dev(state))
    drv.cs.isnow.copy_(_dev(isnow))
    if drv.accum is not None:
        drv.accum.restore(None)


def _end(drv):
    return (drv.cs.state.cpu().numpy(), drv.cs.isnow.cpu().numpy(), drv.cs.status.cpu().numpy())


def _history_from_chain(ends, start, static_i, weight, tol=None):
    """The drift history the chain's consecutive end states give, by the twins."""
    tol = np.full(L.NDRIFT, np.inf) if tol is None else tol
    out, prev = [], spinup.tracked_host(start[0], start[1], static_i)
    for st, isn, _ in ends:
        now = spinup.tracked_host(st, isn, static_i)
        out.append(spinup.reduce_host(spinup.drift_host(now, prev), tol, weight))
        prev = now
    return out


def _check_history(history, want, first_loop=1):
    assert [r.loop for r in history] == list(range(first_loop, first_loop + len(want)))
    for r, w in zip(history, want):
        assert same_bits(np.array(r.max), w.max), (r.loop, r.max, w.max)
        assert r.arg == w.arg.tolist() and r.count == w.count.tolist(), r.loop
        assert same_bits(np.array(r.mean), w.mean), r.loop


@pytest.fixture(scope="module", params=[4, 8])
def synth(request, engine_lib, tmp_path_factory):
    """300 mixed columns over one day of hourly steps: a chain of three fresh
    drivers, each from begdatetime and the state the one before left, and one
    driver that spins up three loops and then runs the period with output."""
    precision = request.param
    tmp = tmp_path_factory.mktemp(f"spinup_synth{precision}")
    nml = _nml(tmp)
    cfg = config.Config(nml)
    assert cfg.step_count() == 24
    P = Params.builtin()
    cols = cases.make_columns(300, "mixed", P.as_dict(), seed=5,
                              julian=timeman.julian(cfg.begdatetime))
    kw = dict(params=P, precision=precision)
    start = (cols.state.astype(_np(precision)), cols.isnow.copy())
    ends, prev = [], None
    for _ in range(3):
        d = driver.OfflineDriver(config.Config(nml), cols, write=False, **kw)
        if prev is not None:
            _set_state(d, prev[0], prev[1])
        d.run()
        assert d.step_index == 24 and d.t == cfg.enddatetime
        prev = _end(d)
        ends.append(prev)
        d.engine.close()
    cfg_a = config.Config(nml)
    cfg_a.outdir, cfg_a.resdir = str(tmp / "out_a"), str(tmp / "res_a")
    a = driver.OfflineDriver(cfg_a, cols, accumulate=True, state_out="all", **kw)
    a.spinup(loops=3)
    out = dict(nml=nml, cols=cols, kw=kw, precision=precision, start=start, ends=ends, tmp=tmp,
               weight=area_weights(np.asarray(cols.static_f[L.STATIC_F.index("LAT")], np.float64)),
               spun=_end(a), history=list(a.spinup_history), stop=a.spinup_stop,
               files_after_spinup=_files(cfg_a.outdir) + _files(cfg_a.resdir),
               written_after_spinup=list(a.written), at=(a.t, a.step_index), cfg_a=cfg_a)
    a.run()
    out["written"] = list(a.written)
    a.engine.close()
    return out


def test_spinup_equals_the_chain(synth):
    st, isn, status = synth["spun"]
    assert same_bits(st, synth["ends"][2][0]) and np.array_equal(isn, synth["ends"][2][1])
    assert not same_bits(st, synth["ends"][1][0])           # the third loop did move the state
    # status keeps OR-ing over the loops
    assert np.array_equal(status, synth["ends"][0][2] | synth["ends"][1][2] | synth["ends"][2][2])
    cfg = synth["cfg_a"]
    assert synth["at"] == (cfg.begdatetime, 0) and synth["stop"] == "ran all 3 loops"


def test_spinup_history_equals_the_twins(synth):
    want = _history_from_chain(synth["ends"], synth["start"], synth["cols"].static_i,
                               synth["weight"])
    assert len(synth["history"]) == 3
    _check_history(synth["history"], want)
    for r in synth["history"]:
        assert r.tol == [np.inf] * 7 and r.converged
        print(f"fp{8 * synth['precision']} loop {r.loop}: max {r.max}")
    assert any(m > 0 for m in synth["history"][0].max)


def test_spinup_writes_nothing_but_its_report(synth):
    assert synth["files_after_spinup"] == ["SPINUP.json"] and synth["written_after_spinup"] == []
    rep = json.load(open(os.path.join(synth["cfg_a"].outdir, "SPINUP.json")))
    assert rep["groups"] == L.DRIFT_GROUPS and rep["stop"] == "ran all 3 loops"
    assert rep["tol"] == ["inf"] * 7 and len(rep["units"]) == 7
    assert rep["history"] == [r.as_json() for r in synth["history"]]


def test_production_run_after_spinup(synth):
    """run() after spinup() writes what a fresh driver started from the
    spun-up state writes: the fluxes, the first interval's budget, the state."""
    cfg_b = config.Config(synth["nml"])
    cfg_b.outdir = str(synth["tmp"] / "out_b")
    b = driver.OfflineDriver(cfg_b, synth["cols"], accumulate=True, state_out="all", **synth["kw"])
    _set_state(b, synth["spun"][0], synth["spun"][1])
    b.run()
    fa = [f for f in synth["written"]]
    fb = list(b.written)
    assert len(fa) == len(fb) == 8
    for x, y in zip(fa, fb):
        assert os.path.basename(x) == os.path.basename(y)
        with np.load(x) as zx, np.load(y) as zy:
            assert str(zx["fields"]) == str(zy["fields"]) and str(zx["time"]) == str(zy["time"])
            assert zx["diag"].shape[0] == 35 + L.NXROWS
            assert same_bits(zx["diag"], zy["diag"]), x
    b.engine.close()


def test_early_stop_and_refusal(synth):
    h2 = synth["history"][1]
    assert all(np.isfinite(h2.max))
    tol = dict(zip(L.DRIFT_GROUPS, h2.max))
    tol_arr = spinup.parse_tol(tol)
    want = _history_from_chain(synth["ends"], synth["start"], synth["cols"].static_i,
                               synth["weight"], tol_arr)
    assert want[0].count.any() and not want[1].count.any()
    c = driver.OfflineDriver(config.Config(synth["nml"]), synth["cols"], write=False,
                             **synth["kw"])
    c.spinup(loops=3, tol=tol, report=False)
    assert len(c.spinup_history) == 2 and c.spinup_stop == "converged after loop 2"
    _check_history(c.spinup_history, want[:2])
    assert c.spinup_history[1].tol == tol_arr.tolist()
    assert same_bits(c.cs.state.cpu().numpy(), synth["ends"][1][0])
    assert (c.t, c.step_index) == (c.cfg.begdatetime, 0)
    # refused once a step has run, with a drift map off a grid, and with bad arguments
    c.run(nsteps=1)
    with pytest.raises(RuntimeError):
        c.spinup(loops=1)
    c.engine.close()
    d = driver.OfflineDriver(config.Config(synth["nml"]), synth["cols"], write=False,
                             **synth["kw"])
    for kw in (dict(loops=0), dict(loops=1, min_loops=0), dict(loops=1, drift_map=True),
               dict(loops=1, tol="NOPE=1"), dict(loops=1, tol="SOIL_M=-1")):
        with pytest.raises(ValueError):
            d.spinup(**kw)
    assert d.spinup_history == [] and (d.t, d.step_index) == (d.cfg.begdatetime, 0)
    # min_loops = 3 holds the loop past the pass that met the tolerances
    d.spinup(loops=3, tol=tol, min_loops=3, report=False)
    assert len(d.spinup_history) == 3
    _check_history(d.spinup_history, want)
    assert same_bits(d.cs.state.cpu().numpy(), synth["ends"][2][0])
    d.engine.close()


# ---- 4. the driver, from files ---------------------------------------------------------
@pytest.fixture(scope="module")
def files(engine_lib, tmp_path_factory):
    """make_offline_case's 4 x 8 grid, one day at 900 s with 3-hourly files and
    the closing file, forcing interpolated in time: a chain of two drivers and
    a two-loop spin-up with the report and the drift map."""
    from test_gpu_tinterp import _case
    tmp = tmp_path_factory.mktemp("spinup_files")
    cfg = _case(tmp / "case")
    nml = str(tmp / "case" / "case.nml")
    ends, prev, start = [], None, None
    for _ in range(2):
        d = driver.OfflineDriver.from_files(config.Config(nml), interp=True, write=False)
        if prev is None:
            start = _end(d)[:2]
        else:
            _set_state(d, prev[0], prev[1])
        d.run()
        assert d.step_index == 96 and d.interp_held == []
        prev = _end(d)
        ends.append(prev)
        perm, static_i = d.perm.copy(), d.cs.static_i.cpu().numpy()
        lat = d._lat.copy()
        d.engine.close()
    cfg_s = config.Config(nml)
    cfg_s.outdir = str(tmp / "out_s")
    s = driver.OfflineDriver.from_files(cfg_s, interp=True)
    s.spinup(loops=2, drift_map=True)
    out = dict(nml=nml, cfg=cfg, tmp=tmp, ends=ends, start=start, perm=perm, static_i=static_i,
               weight=area_weights(lat), grid=s.grid, spun=_end(s), history=list(s.spinup_history),
               held=list(s.interp_held), outdir=cfg_s.outdir, files=_files(cfg_s.outdir),
               same_perm=np.array_equal(s.perm, perm), blocks=s.feed.up.count)
    s.engine.close()
    return out


def test_files_spinup_equals_the_chain(files):
    assert files["same_perm"] and files["held"] == []
    assert same_bits(files["spun"][0], files["ends"][1][0])
    assert np.array_equal(files["spun"][1], files["ends"][1][1])
    # feed.reset(): every loop formed its nine blocks again
    assert files["blocks"] == 18
    want = _history_from_chain(files["ends"], files["start"], files["static_i"], files["weight"])
    _check_history(files["history"], want)
    assert any(m > 0 for m in files["history"][1].max)


def test_files_report_and_drift_map(files):
    assert files["files"] == ["SPINUP.json", "SPINUP_DRIFT_DOMAIN1"]
    rep = json.load(open(os.path.join(files["outdir"], "SPINUP.json")))
    assert rep["history"] == [r.as_json() for r in files["history"]] and len(rep["history"]) == 2
    assert rep["groups"] == L.DRIFT_GROUPS and rep["stop"] == "ran all 2 loops"
    names = [f"DRIFT_{g}" for g in L.DRIFT_GROUPS]
    got = ncio.read_ldasout(os.path.join(files["outdir"], "SPINUP_DRIFT_DOMAIN1"), files["grid"],
                            names)[:, files["perm"]]
    t = [spinup.tracked_host(st, isn, files["static_i"]) for st, isn, _ in files["ends"]]
    assert same_bits(got, spinup.drift_host(t[1], t[0]))
    raw = ncio.read_ldasin(os.path.join(files["outdir"], "SPINUP_DRIFT_DOMAIN1"))
    assert sorted(raw) == sorted(names)
    assert (raw["DRIFT_TWS"][~files["grid"].mask] == ncio.FILL).all()


# ---- 5. the CLI ------------------------------------------------------------------------
def _cli():
    spec = importlib.util.spec_from_file_location("noahmp_offline",
                                                  os.path.join(ROOT, "noahmp_offline.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    return cli


def test_offline_cli_spinup(files, capsys):
    cli, cfg = _cli(), files["cfg"]
    assert cli.main([files["nml"], "--interp", "--spinup-loops", "2", "--spinup-restart"]) == 0
    text = capsys.readouterr().out
    assert "spin-up loop 1:" in text and "spin-up loop 2:" in text and "ran all 2 loops" in text
    assert len(glob.glob(os.path.join(cfg.outdir, "*.LDASOUT_DOMAIN1"))) == 8
    stamp = cfg.begdatetime.strftime("%Y%m%d%H")
    path = os.path.join(cfg.resdir, f"RESTART.{stamp}_DOMAIN1.spinup.nc")
    st, isn, t, step = ncio.read_state(path, files["grid"])
    assert (t, step) == (cfg.begdatetime, 0)
    assert same_bits(st[:, files["perm"]], files["ends"][1][0])
    assert np.array_equal(isn[files["perm"]], files["ends"][1][1])
    for bad in (["--spinup-tol", "SOIL_M=1"], ["--spinup-min-loops", "2"], ["--spinup-map"],
                ["--spinup-restart"], ["--spinup-loops", "0"],
                ["--spinup-loops", "2", "--spinup-tol", "NOPE=1"],
                ["--spinup-loops", "2", "--spinup-min-loops", "0"]):
        with pytest.raises(SystemExit):
            cli.main([files["nml"]] + bad)


# ---- 6. two ranks ----------------------------------------------------------------------
def _spin_rank(rank, world, port, nml, tol, out):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    drv = driver.OfflineDriver.from_files(config.Config(nml), interp=True, write=False)
    drv.spinup(loops=3, tol=tol, report=False)
    with open(f"{out}.r{rank}.json", "w") as f:
        json.dump(dict(stop=drv.spinup_stop, history=[r.as_json() for r in drv.spinup_history]), f)
    with pytest.raises(ValueError):
        drv.spinup(loops=1, drift_map=True)      # the drift map is a single rank's
    dist.barrier()
    drv.engine.close()
    dist.destroy_process_group()


def test_two_ranks_decide_as_one(files):
    import socket
    import torch.multiprocessing as mp
    # stops after loop 2 on a single rank: its loop-2 maxima as the tolerances
    tol = dict(zip(L.DRIFT_GROUPS, files["history"][1].max))
    single = driver.OfflineDriver.from_files(config.Config(files["nml"]), interp=True,
                                             write=False)
    single.spinup(loops=3, tol=tol, report=False)
    assert single.spinup_stop == "converged after loop 2"
    want = [r.as_json() for r in single.spinup_history]
    single.engine.close()
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    out = str(files["tmp"] / "ranks")
    mp.start_processes(_spin_rank, args=(2, port, files["nml"], tol, out), nprocs=2,
                       start_method="spawn")
    for rank in range(2):
        got = json.load(open(f"{out}.r{rank}.json"))
        assert got["stop"] == "converged after loop 2" and len(got["history"]) == 2
        for g, w in zip(got["history"], want):
            assert g["loop"] == w["loop"] and g["tol"] == w["tol"]
            assert g["max"] == w["max"] and g["arg"] == w["arg"] and g["count"] == w["count"]
            assert np.allclose(g["mean"], w["mean"], rtol=1e-12)   # its last bits may differ
