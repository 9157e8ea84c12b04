"""Interval statistics on the GPU: nmp_intstats_update / nmp_intstats_output
against their numpy restatement (intstats.update_host / output_host), and the
offline driver with interval_stats=... against values formed in numpy from the
reference's own trajectory (traj_casenml fixture), bit for bit: beside
accumulation, state output and regions, through restart files, after a spin-up
and on two ranks.

Bounds: every comparison is on bits.  The kernels do one double add per step
and item, and at output one double division or product and one conversion,
which numpy forms the same way."""
import datetime
import glob
import os

import numpy as np
import pytest
import torch

import noahmp_pkg  # noqa: F401  (spawned ranks re-import this module)
from golden_io import bit_equal, load
from noahmp_amd import cases, config, driver, intstats as IS, layout as L, ncio, timeman
from noahmp_amd.engine import ColumnState, Engine
from noahmp_amd.params import Params
from test_gpu_accum import ACC_SHAPES

pytestmark = pytest.mark.gpu

NAN, INF = float("nan"), float("inf")
DIAG, FORC, STATE = L.EXT_SRC_DIAG, L.EXT_SRC_FORCING, L.EXT_SRC_STATE
SPEC = ("T2M,SMC1,TG,SNEQV,FROST=SFCTMP@lt273.15:dur+spell+deg,WET=PRCP@gt0:dur+spell,"
        "LEAFWET=CANLIQ@gt0,HEAT=FSH@gt0:deg")
ITEMS = IS.parse(SPEC)
NAMES = IS.row_names(ITEMS)
NIST = len(NAMES)
assert NAMES == ["T2M_MEAN", "SMC1_MEAN", "TG_MEAN", "SNEQV_MEAN", "FROST_DUR", "FROST_DEG",
                 "FROST_SPELL", "WET_DUR", "WET_SPELL", "LEAFWET_DUR", "HEAT_DEG"]
# beside accumulation, whose rows have a T2M_MEAN of their own, the item takes a label
SPEC_ACC = SPEC.replace("T2M,", "T2AVG=T2M,", 1)
NAMES_ACC = ["T2AVG_MEAN"] + NAMES[1:]


def ibits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize])


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(ibits(a), ibits(b))


def first_diff(got, want):
    """Where two arrays first differ in bits, for an assertion's message."""
    got, want = np.asarray(got), np.asarray(want)
    at = np.argwhere(ibits(got) != ibits(want))
    if not len(at):
        return "equal"
    i = tuple(at[0])
    return f"{len(at)} differ, first at {i}: got {got[i]!r} ({ibits(got)[i]:#x}), " \
           f"want {want[i]!r} ({ibits(want)[i]:#x})"


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda:0")


def _engine(precision):
    return Engine(Params.builtin(), L.CASE_NML_OPTIONS, device=0, precision=precision)


# ---- 1. the kernels against the restatement ---------------------------------------------
# items of all three kinds, all four operators and every stat, against a
# threshold of 2 and of 0; the planted columns' values go into every item's
# source row
M, U, G, S = L.IST_MEAN, L.IST_DUR, L.IST_DEG, L.IST_SPELL
K_ITEMS = [(DIAG, 3, L.IST_NONE, M), (FORC, 8, L.IST_GT, U | G | S), (STATE, 29, L.IST_GE, U),
           (DIAG, 15, L.IST_LT, G | S), (STATE, 55, L.IST_LE, U | S), (FORC, 0, L.IST_NONE, M),
           (STATE, 29, L.IST_NONE, M), (FORC, 8, L.IST_GT, G), (DIAG, 3, L.IST_GE, U | S),
           (STATE, 55, L.IST_LT, U), (FORC, 0, L.IST_LE, U | G | S)]
K_THR = [0.0, 2.0, 2.0, 2.0, 2.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0]
NSTEP = 7
PLANTED = {
    "equal_to_2": [2, 2, 2, 2, 2, 2, 2],
    "signed_zeros": [-0.0, 0.0, -0.0, 0.0, -0.0, 0.0, -0.0],
    "nan_inside_a_spell": [3, 3, NAN, 3, 3, 1, 3],
    "plus_inf": [INF, 3, INF, 1, INF, INF, 3],
    "minus_inf": [-INF, 1, -INF, 3, -INF, -INF, -1],
    "both_inf": [INF, -INF, 3, INF, 1, -INF, 2],
    "alternating": [3, 1, 3, 1, 3, 1, 3],
    "two_equal_spells": [3, 3, 1, 3, 3, 1, 1],
    "all_above": [5, 5, 5, 5, 5, 5, 5],
    "all_below": [-5, -5, -5, -5, -5, -5, -5],
}


def _run_kernels(eng, dtype, items, thr, ld, lo, hi, nstep, seed, planted=True):
    rng = np.random.default_rng(seed)
    ni = len(items)
    nrow = sum(bin(it[3]).count("1") for it in items)
    acc0 = np.full((ni, ld), NAN)                     # k == 1 must not read them
    cnt0 = rng.integers(-9, 99, size=(3 * ni, ld)).astype(np.int32)
    acc, cnt = _dev(acc0), _dev(cnt0)
    want_a, want_c = acc0.copy(), cnt0.copy()
    mean_rows = [3 * i + j for i, it in enumerate(items) if it[2] == L.IST_NONE for j in range(3)]
    out0 = rng.normal(size=(nrow + 3, ld)).astype(dtype)     # a block: the rows are 1..nrow
    col = {name: lo + j for j, name in enumerate(PLANTED) if lo + j < hi} if planted else {}
    assert not planted or len(col) == len(PLANTED) or hi - lo == 1
    for k in range(1, nstep + 1):
        diag = rng.normal(1.0, 2.0, size=(16, ld)).astype(dtype)
        forcing = rng.normal(1.0, 2.0, size=(12, ld)).astype(dtype)
        state = rng.normal(1.0, 2.0, size=(56, ld)).astype(dtype)
        blocks = {DIAG: diag, FORC: forcing, STATE: state}
        for kind, row, _, _ in items:
            for name, c in col.items():
                blocks[kind][row, c] = PLANTED[name][k - 1]
        d, f, s = _dev(diag), _dev(forcing), _dev(state)
        eng.intstats_update(items, thr, k, acc, cnt, d, f, s, cols=(lo, hi))
        IS.update_host(want_a[:, lo:hi], want_c[:, lo:hi], k, items, thr, diag[:, lo:hi],
                       forcing[:, lo:hi], state[:, lo:hi])
        torch.cuda.synchronize()
        before = acc.cpu().numpy(), cnt.cpu().numpy()
        block = _dev(out0)
        eng.intstats_output(items, k, 900.0, acc, cnt, block[1:1 + nrow], cols=(lo, hi))
        torch.cuda.synchronize()
        got_a, got_c, got_o = acc.cpu().numpy(), cnt.cpu().numpy(), block.cpu().numpy()
        assert same_bits(got_a[:, lo:hi], want_a[:, lo:hi]), \
            (k, first_diff(got_a[:, lo:hi], want_a[:, lo:hi]))
        assert np.array_equal(got_c[:, lo:hi], want_c[:, lo:hi]), \
            (k, first_diff(got_c[:, lo:hi], want_c[:, lo:hi]))
        # the output call changed neither array; outside the range nothing moved; a
        # mean item's cnt rows (rows no item names) are as they were
        assert same_bits(got_a, before[0]) and np.array_equal(got_c, before[1])
        assert same_bits(got_a[:, :lo], acc0[:, :lo]) and same_bits(got_a[:, hi:], acc0[:, hi:])
        assert np.array_equal(got_c[:, :lo], cnt0[:, :lo])
        assert np.array_equal(got_c[:, hi:], cnt0[:, hi:])
        assert np.array_equal(got_c[mean_rows], cnt0[mean_rows])
        want_o = IS.output_host(want_a[:, lo:hi], want_c[:, lo:hi], items, k, 900.0, dtype)
        assert same_bits(got_o[1:1 + nrow, lo:hi], want_o), \
            (k, first_diff(got_o[1:1 + nrow, lo:hi], want_o))
        assert same_bits(got_o[0], out0[0]) and same_bits(got_o[1 + nrow:], out0[1 + nrow:])
        assert same_bits(got_o[:, :lo], out0[:, :lo]) and same_bits(got_o[:, hi:], out0[:, hi:])
        # the inputs are read only
        assert same_bits(d.cpu().numpy(), diag) and same_bits(f.cpu().numpy(), forcing)
        assert same_bits(s.cpu().numpy(), state)
    return want_a, want_c, col


@pytest.mark.parametrize("ld,lo,hi", ACC_SHAPES + [(1, 0, 1), (70, 69, 70)])
@pytest.mark.parametrize("precision", [4, 8])
def test_kernels_equal_the_restatement(engine_lib, precision, ld, lo, hi):
    eng = _engine(precision)
    dtype = np.float32 if precision == 4 else np.float64
    a, n, col = _run_kernels(eng, dtype, K_ITEMS, K_THR, ld, lo, hi, NSTEP, 100 * precision + ld)
    eng.close()
    assert not np.isnan(a[:, lo:hi][[1, 2, 3, 4, 7, 8, 9, 10]]).any()   # k == 1 ignored the NaN
    if len(col) < len(PLANTED):
        return
    # the restatement itself, on the planted columns: (count, run, longest) of an item
    cnt = lambda i, name: n[3 * i:3 * i + 3, col[name]].tolist()  # noqa: E731
    assert cnt(1, "equal_to_2") == [0, 0, 0] and cnt(2, "equal_to_2") == [7, 7, 7]    # gt, ge 2
    assert cnt(3, "equal_to_2") == [0, 0, 0] and cnt(4, "equal_to_2") == [7, 7, 7]    # lt, le 2
    assert cnt(7, "signed_zeros") == [0, 0, 0] and cnt(8, "signed_zeros") == [7, 7, 7]   # gt, ge 0
    assert cnt(9, "signed_zeros") == [0, 0, 0] and cnt(10, "signed_zeros") == [7, 7, 7]  # lt, le 0
    assert ibits(a[[7, 8, 9, 10], col["signed_zeros"]]).tolist() == [0, 0, 0, 0]
    assert cnt(1, "nan_inside_a_spell") == [5, 1, 2]       # not counted, and it broke the spell
    assert a[1, col["nan_inside_a_spell"]] == 5.0 and np.isnan(a[0, col["nan_inside_a_spell"]])
    assert cnt(1, "plus_inf") == [6, 3, 3] and a[1, col["plus_inf"]] == INF
    assert cnt(3, "minus_inf") == [6, 3, 3] and a[3, col["minus_inf"]] == INF
    assert cnt(1, "minus_inf") == [1, 0, 1] and a[1, col["minus_inf"]] == 1.0
    assert a[0, col["plus_inf"]] == INF and a[5, col["minus_inf"]] == -INF
    assert np.isnan(a[0, col["both_inf"]]) and cnt(1, "both_inf") == [3, 0, 2]
    assert cnt(1, "alternating") == [4, 1, 1] and cnt(3, "alternating") == [3, 0, 1]
    assert cnt(1, "two_equal_spells") == [4, 0, 2] and a[1, col["two_equal_spells"]] == 4.0
    assert cnt(1, "all_above") == [7, 7, 7] and cnt(3, "all_above") == [0, 0, 0]
    assert cnt(1, "all_below") == [0, 0, 0] and cnt(3, "all_below") == [7, 7, 7]
    assert a[1, col["all_above"]] == 21.0 and a[3, col["all_below"]] == 49.0
    assert a[0, col["all_above"]] == 35.0 and a[1, col["all_below"]] == 0.0


@pytest.mark.parametrize("precision", [4, 8])
def test_thirty_two_items_in_one_call(engine_lib, precision):
    srcs = sorted(IS.SOURCES.values())
    items, thr = [], []
    for i in range(32):
        kind, row = srcs[(7 * i) % len(srcs)]
        op = i % 5
        items.append((kind, row, op, M if op == 0 else (U, G, S, U | G | S)[i % 4]))
        thr.append([0.0, 2.0, 1.0, -0.5][i % 4])
    assert {it[0] for it in items} == {0, 1, 2} and {it[2] for it in items} == {0, 1, 2, 3, 4}
    eng = _engine(precision)
    _run_kernels(eng, np.float32 if precision == 4 else np.float64, items, thr, 334, 38, 301, 3,
                 7 + precision, planted=False)
    eng.close()


# ---- 2. blocks no item names may be NULL; the refusals' order -------------------------------
def test_blocks_no_item_names_may_be_null(engine_lib):
    eng = _engine(4)
    rng = np.random.default_rng(5)
    n = 130
    state = rng.normal(size=(56, n)).astype(np.float32)
    forcing = rng.normal(size=(12, n)).astype(np.float32)
    acc = torch.full((2, n), NAN, dtype=torch.float64, device="cuda:0")
    cnt = torch.full((6, n), 5, dtype=torch.int32, device="cuda:0")
    items, thr = [(STATE, 37, L.IST_NONE, M), (FORC, 8, L.IST_GT, U)], [0.0, 0.0]
    eng.intstats_update(items, thr, 1, acc, cnt, None, _dev(forcing), _dev(state))
    torch.cuda.synchronize()
    want = np.stack([state[37].astype(np.float64), np.where(forcing[8] > 0, forcing[8], 0.0)])
    assert same_bits(acc.cpu().numpy(), want)
    h = (forcing[8] > 0).astype(np.int32)
    assert np.array_equal(cnt.cpu().numpy(), np.stack([h * 0 + 5] * 3 + [h] * 3))
    # mean items alone need no cnt at all (the wrapper wants a tensor: the library call itself)
    import ctypes as C
    i32 = (C.c_int32 * 4)(STATE, 37, L.IST_NONE, M)
    f64 = (C.c_double * 1)(0.0)
    sd, one = _dev(state), torch.zeros((1, n), dtype=torch.float64, device="cuda:0")
    null = C.c_void_p(0)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert engine_lib.nmp_intstats_update(eng._h, n, n, 1, i32, f64, null, null,
                                          C.c_void_p(sd.data_ptr()), 1,
                                          C.c_void_p(one.data_ptr()), null, n, st) == 0
    torch.cuda.synchronize()
    assert same_bits(one.cpu().numpy()[0], state[37].astype(np.float64))
    # refused with nothing enqueued: a missing block an item names, k < 1, a bad item
    from noahmp_amd.lib import NmpError
    before = acc.cpu().numpy(), cnt.cpu().numpy()
    bad_items = ([(3, 0, 0, M), items[1]], [(STATE, 56, 0, M), items[1]],
                 [(STATE, 37, 5, U), items[1]], [(STATE, 37, 0, U), items[1]],
                 [items[0], (FORC, 8, L.IST_GT, M)], [items[0], (FORC, 8, L.IST_GT, 0)])
    for kw in [dict(state=None), dict(forcing=None), dict(k=0), dict(thr=[0.0, NAN]),
               dict(thr=[0.0, INF])] + [dict(items=b) for b in bad_items]:
        a = dict(items=items, thr=thr, k=2, forcing=_dev(forcing + 1), state=_dev(state + 1))
        a.update(kw)
        with pytest.raises(NmpError) as e:
            eng.intstats_update(a["items"], a["thr"], a["k"], acc, cnt, None, a["forcing"],
                                a["state"])
        assert e.value.code == -1
    out = torch.zeros((2, n), device="cuda:0")
    for kw in [dict(k=0), dict(dt=0.0), dict(dt=NAN), dict(dt=INF)] + \
            [dict(items=b) for b in bad_items[:5]]:
        a = dict(items=items, k=2, dt=900.0)
        a.update(kw)
        with pytest.raises(NmpError) as e:
            eng.intstats_output(a["items"], a["k"], a["dt"], acc, cnt, out)
        assert e.value.code == -1
    # the order: a bad item is refused in an empty call too; an empty call with valid
    # items is NMP_OK whatever the pointers; NULL pointers are refused after that
    with pytest.raises(NmpError):
        eng.intstats_update(bad_items[0], thr, 3, acc, cnt, None, _dev(forcing), _dev(state),
                            cols=(7, 7))
    i32 = (C.c_int32 * 8)(STATE, 37, L.IST_NONE, M, FORC, 8, L.IST_GT, U)
    f64 = (C.c_double * 2)(0.0, 0.0)
    assert engine_lib.nmp_intstats_update(eng._h, 0, n, 2, i32, f64, null, null, null, 3, null,
                                          null, n, st) == 0
    assert engine_lib.nmp_intstats_update(eng._h, n, n, 2, i32, f64, null, null, null, 3, null,
                                          null, n, st) == -1
    assert engine_lib.nmp_intstats_output(eng._h, 0, 2, i32, 3, 900.0, null, null, n, null, n,
                                          st) == 0
    assert engine_lib.nmp_intstats_output(eng._h, n, 2, i32, 3, 900.0, null, null, n, null, n,
                                          st) == -1
    eng.intstats_update(items, thr, 3, acc, cnt, None, _dev(forcing), _dev(state), cols=(7, 7))
    torch.cuda.synchronize()
    assert same_bits(acc.cpu().numpy(), before[0]) and np.array_equal(cnt.cpu().numpy(), before[1])
    assert not out.cpu().numpy().any()
    eng.close()


# ---- the driver: shared runs ---------------------------------------------------------------
def _cols(g, state=None, isnow=None):
    return cases.ColumnSet(g["static_f"], g["static_i"], g["state0"] if state is None else state,
                           g["isnow0"] if isnow is None else isnow, *([None] * 7))


def _cfg(tmp_path, sub="out"):
    from test_config import write_case
    cfg = config.Config(write_case(tmp_path))
    cfg.outdir = str(tmp_path / sub)
    return cfg


def _npz_files(outdir):
    return sorted(glob.glob(os.path.join(outdir, "*.LDASOUT.npz")))


def _npz_members(path):
    with np.load(path, allow_pickle=False) as z:
        return {k: (z[k].dtype.str, z[k].shape, z[k].tobytes()) for k in z.files}


def _netcdf_files(outdir):
    return sorted(glob.glob(os.path.join(outdir, "*.LDASOUT_DOMAIN1")))


def _regions_files(outdir):
    return sorted(glob.glob(os.path.join(outdir, "*.REGIONS_DOMAIN1")))


@pytest.fixture(scope="module")
def traj():
    return load("traj_casenml.npz")


def _twin(g, precision, nsteps, state=None, isnow=None):
    """A plain engine run of the fixture's columns: per step the 16 output
    fluxes and the state the step left."""
    eng = _engine(precision)
    dt = torch.float32 if precision == 4 else torch.float64
    cs = ColumnState.from_host(_cols(g, state, isnow), "cuda:0", dt)
    diag = torch.zeros((16, 32), device="cuda:0", dtype=dt)
    t, diags, states = datetime.datetime(2000, 1, 1), [], []
    for k in range(nsteps):
        f = _dev(g["forcing"][k]).to(dt)
        eng.step(cs, f, cases.CASE_NML_ZSOIL, 900.0, timeman.julian(t), timeman.yearlen(t.year),
                 diag, L.DIAG_OUT_LEVEL)
        diags.append(diag.cpu().numpy().copy())
        states.append(cs.state.cpu().numpy().copy())
        t = t + datetime.timedelta(seconds=900)
    eng.close()
    return diags, states


@pytest.fixture(scope="module")
def twin32(engine_lib, traj):
    diags, states = _twin(traj, 4, 96)
    assert bit_equal(states[-1], traj["states"][-1]).all()
    return diags, states


def _ref_step(g, twin32, k):
    """(diag16, forcing, state) of step k from the reference's trajectory, T2M
    (which the reference's argument list does not have) from the twin run."""
    diag = np.stack([twin32[0][k][i] if n == "T2M" else g["diags"][k][L.DIAG_FULL.index(n)]
                     for i, n in enumerate(L.DIAG_OUT)])
    return diag, g["forcing"][k], g["states"][k]


def _want_rows(steps, items=ITEMS, dtype=np.float32):
    """The statistics rows of an interval from its steps' (diag, forcing, state)."""
    n = steps[0][0].shape[1]
    acc, cnt = np.full((len(items), n), NAN), np.full((3 * len(items), n), -3, np.int32)
    for k, (d, f, s) in enumerate(steps, 1):
        IS.update_host(acc, cnt, k, IS.table(items), IS.thresholds(items), d, f, s)
    return IS.output_host(acc, cnt, IS.table(items), len(steps), 900.0, dtype)


@pytest.fixture(scope="module")
def ist_run(engine_lib, traj, tmp_path_factory):
    """The uninterrupted run of the trajectory's 96 steps with SPEC (npz
    output, two ranges of 16 columns) and the same run without the option."""
    tmp = tmp_path_factory.mktemp("ist_run")
    res = {}
    for key, kw in (("ist", dict(interval_stats=SPEC)), ("plain", dict())):
        cfg = _cfg(tmp, key)
        drv = driver.OfflineDriver(cfg, _cols(traj), forcing=lambda step, t: traj["forcing"][step],
                                   **kw)
        assert [hi - lo for lo, hi in drv.ranges.ranges] == [16, 16]
        drv.run()
        assert drv.step_index == 96
        files = _npz_files(cfg.outdir)
        assert len(files) == 8
        res[key] = dict(files=files, state=drv.cs.state.cpu().numpy(),
                        isnow=drv.cs.isnow.cpu().numpy(), names=list(drv.out_names))
        drv.engine.close()
    return res


# ---- 3. the reference's own trajectory shows the feature ------------------------------------
def _item_steps(g, twin32, it, j):
    """(12, 32) values of item `it`'s series over interval j, from the reference's data."""
    blocks = [_ref_step(g, twin32, k) for k in range(12 * j, 12 * j + 12)]
    return np.stack([b[it.kind][it.row] for b in blocks])


def _longest(h):
    """The longest run of True down each column of h (steps, n)."""
    run, best = np.zeros(h.shape[1], int), np.zeros(h.shape[1], int)
    for row in h:
        run = np.where(row, run + 1, 0)
        best = np.maximum(best, run)
    return best


def test_reference_data_shows_the_feature(traj, twin32):
    """Column-intervals (of 8 x 32) where the condition holds on some but not
    all of the 12 steps, and of those the ones whose longest spell is shorter
    than the duration: counted on the fixture, asserted as lower bounds."""
    assert not any(np.isnan(traj[k]).any() for k in ("diags", "forcing", "states"))
    bounds = {"PRCP@gt0": (198, 116), "SFCTMP@lt273.15": (25, 6), "CANLIQ@gt0": (47, 11)}
    for cond, (some, broken) in bounds.items():
        (it,) = IS.parse(f"X={cond}:dur+spell")
        ct = np.float32(it.c)
        part = short = 0
        for j in range(8):
            v = _item_steps(traj, twin32, it, j)
            h = v > ct if it.op == L.IST_GT else v < ct
            p = (h.sum(0) > 0) & (h.sum(0) < 12)
            part += int(p.sum())
            short += int((p & (_longest(h) < h.sum(0))).sum())
        print(f"{cond}: partly held in {part} of 256 column-intervals, broken spells in {short}")
        assert part >= some and short >= broken, cond


# ---- 4. the driver against the reference trajectory ------------------------------------------
def test_driver_rows_equal_reference_trajectory(ist_run, twin32, traj):
    g = traj
    assert ist_run["ist"]["names"] == L.DIAG_OUT + NAMES
    assert bit_equal(ist_run["ist"]["state"], g["states"][-1]).all()
    assert np.array_equal(ist_run["ist"]["isnow"], g["isnows"][-1])
    assert same_bits(ist_run["ist"]["state"], ist_run["plain"]["state"])
    for j, (fe, fp) in enumerate(zip(ist_run["ist"]["files"], ist_run["plain"]["files"])):
        assert os.path.basename(fe) == os.path.basename(fp)
        with np.load(fe, allow_pickle=False) as z:
            d, fields = z["diag"], str(z["fields"]).split(",")
        with np.load(fp, allow_pickle=False) as z:
            d16 = z["diag"]
        assert fields == L.DIAG_OUT + NAMES and d.shape == (16 + NIST, 32)
        assert d.dtype == np.float32
        assert same_bits(d[:16], d16), f"file {j}: the output step's fluxes changed"
        steps = [_ref_step(g, twin32, k) for k in range(12 * j, 12 * j + 12)]
        want = _want_rows(steps)
        for i, name in enumerate(NAMES):
            assert same_bits(d[16 + i], want[i]), (j, name)
        # independently: a step-ordered double sum, and numpy counts
        for it in ITEMS:
            v = _item_steps(g, twin32, it, j)
            if it.stats & L.IST_MEAN:
                s = np.zeros(32)
                for row in v:
                    s = s + row.astype(np.float64)
                assert same_bits(d[fields.index(f"{it.label}_MEAN")],
                                 (s / 12.0).astype(np.float32)), (j, it.label)
            if it.stats & L.IST_DUR:
                ct = np.float32(it.c)
                h = v > ct if it.op == L.IST_GT else v < ct
                assert np.array_equal(d[fields.index(f"{it.label}_DUR")],
                                      (900.0 * h.sum(0)).astype(np.float32)), (j, it.label)
                if it.stats & L.IST_SPELL:
                    assert np.array_equal(d[fields.index(f"{it.label}_SPELL")],
                                          (900.0 * _longest(h)).astype(np.float32)), (j, it.label)


# ---- 5. beside accumulation, state output and regions ------------------------------------------
@pytest.fixture(scope="module")
def case(engine_lib, traj, tmp_path_factory):
    """The trajectory's netCDF case with a region file, run with accumulate,
    state_out and regions, with and without interval statistics."""
    from test_gpu_driver import _write_netcdf_case
    tmp = tmp_path_factory.mktemp("ist_case")
    nml, grid = _write_netcdf_case(tmp, traj)
    ny, nx = grid.shape
    rng = np.random.default_rng(21)
    reg = rng.integers(0, 3, size=(ny, nx)).astype(np.int32) * 4 + 2
    reg.reshape(-1)[grid.index[rng.choice(grid.n, 5, replace=False)]] = -1
    area = rng.uniform(0.5, 2.0, size=(ny, nx))
    regfile = str(tmp / "regions.nc")
    ncio.write_region_map(regfile, grid, reg, area)
    out = dict(nml=str(nml), grid=grid, regfile=regfile, tmp=tmp,
               ids=reg.reshape(-1)[grid.index].astype(np.int64), w=area.reshape(-1)[grid.index])
    common = dict(accumulate=True, state_out="SOIL_M,SNOW_T", regions=regfile,
                  extremes="TG,PRCP:max+tmax")
    for key, kw in (("with", dict(common, interval_stats=SPEC_ACC)), ("without", common),
                    ("only", dict(interval_stats=SPEC))):
        cfg = config.Config(str(nml))
        cfg.outdir = str(tmp / key)
        drv = driver.OfflineDriver.from_files(cfg, **kw).run()
        assert drv.step_index == 96
        out[key] = dict(outdir=cfg.outdir, perm=drv.perm.copy(), names=list(drv.out_names))
        drv.engine.close()
    return out


def test_composition_rows_and_regions(case, ist_run):
    from noahmp_amd import stateout
    from noahmp_amd.regions import RegionPlan
    grid, perm = case["grid"], case["with"]["perm"]
    srows = stateout.row_names(stateout.parse_groups("SOIL_M,SNOW_T"))
    xrows = ["TG_MAX", "TG_MIN", "PRCP_MAX", "PRCP_TMAX"]
    names = case["with"]["names"]
    # row order: fluxes, budget rows, extremes rows, statistics rows, state rows
    assert names == L.DIAG_OUT + L.BUDGET + xrows + NAMES_ACC + srows
    assert case["without"]["names"] == L.DIAG_OUT + L.BUDGET + xrows + srows
    a, b = _netcdf_files(case["with"]["outdir"]), _netcdf_files(case["without"]["outdir"])
    assert len(a) == len(b) == 8
    plan = RegionPlan.from_ids(case["ids"][perm], case["w"][perm])
    nred = 39 + NIST + 4
    ra, rb = _regions_files(case["with"]["outdir"]), _regions_files(case["without"]["outdir"])
    assert len(ra) == len(rb) == 8
    for j, (x, y) in enumerate(zip(a, b)):
        dx = ncio.read_ldasout(x, grid, names)
        dy = ncio.read_ldasout(y, grid, case["without"]["names"])
        assert same_bits(dx[:39], dy[:39]), x                  # fluxes, budget and extremes rows
        assert same_bits(dx[39 + NIST:], dy[39:]), x           # state rows
        # the statistics rows are the npz run's, in grid order
        with np.load(ist_run["ist"]["files"][j], allow_pickle=False) as z:
            assert same_bits(dx[39:39 + NIST], z["diag"][16:]), x
        # the run's own T2M_MEAN (a float sum) is not the statistics' (a double sum)
        rx, ry = ncio.read_ldasin(x), ncio.read_ldasin(y)
        assert list(rx) == L.DIAG_OUT + L.BUDGET + xrows + NAMES_ACC + ["SOIL_M", "SNOW_T"]
        for name in ry:
            assert np.asarray(rx[name]).tobytes() == np.asarray(ry[name]).tobytes(), (x, name)
        # REGIONS: the statistics rows ride along, the fill-capable SNOW_T rows do not
        r, r0 = ncio.read_regions(ra[j]), ncio.read_regions(rb[j])
        assert r["names"] == names[:nred] and r0["names"] == case["without"]["names"][:43]
        want = plan.reduce_host(dx[:nred, perm])[1]
        assert same_bits(r["means"], want), ra[j]
        assert same_bits(r["means"][:39], r0["means"][:39])
        assert same_bits(r["means"][39 + NIST:], r0["means"][39:])
    # statistics alone on the grid: the same rows after the 16 fluxes
    c = _netcdf_files(case["only"]["outdir"])
    assert case["only"]["names"] == L.DIAG_OUT + NAMES and len(c) == 8
    for j, x in enumerate(c):
        with np.load(ist_run["ist"]["files"][j], allow_pickle=False) as z:
            assert same_bits(ncio.read_ldasout(x, grid, case["only"]["names"]), z["diag"]), x


def test_a_colliding_row_name_is_refused(engine_lib, traj, tmp_path):
    with pytest.raises(ValueError, match="T2M_MEAN"):
        driver.OfflineDriver(_cfg(tmp_path), _cols(traj), accumulate=True, interval_stats=SPEC)


def _record_steps(drv):
    """Every ranges.step call's (diag_level, the diag block's address)."""
    calls, step = [], drv.ranges.step

    def spy(forcing, zsoil, dt, julian, yearlen, diag=None, diag_level=L.DIAG_NONE, **kw):
        calls.append((diag_level, None if diag is None else diag.data_ptr()))
        return step(forcing, zsoil, dt, julian, yearlen, diag, diag_level, **kw)
    drv.ranges.step = spy
    return calls


def test_steps_between_outputs_keep_their_diag_level(engine_lib, traj, tmp_path):
    ff = lambda step, t: traj["forcing"][step]  # noqa: E731
    # state and forcing items only: the steps between output steps write no fluxes
    drv = driver.OfflineDriver(_cfg(tmp_path, "sf"), _cols(traj), forcing=ff,
                               interval_stats="TG,SMC1,WET=PRCP@gt0:dur+spell")
    assert drv.block.scratch is None and not drv.intstats.needs_fluxes
    calls = _record_steps(drv)
    drv.run(nsteps=25)
    drv.engine.close()
    assert [c[0] for c in calls] == ([L.DIAG_NONE] * 11 + [L.DIAG_OUT_LEVEL]) * 2 + [L.DIAG_NONE]
    assert all(c[1] is None for c in calls if c[0] == L.DIAG_NONE)
    # a flux item: every step writes its fluxes, between output steps into one scratch block
    drv = driver.OfflineDriver(_cfg(tmp_path, "d"), _cols(traj), forcing=ff,
                               interval_stats="T2M,HEAT=FSH@gt0:deg")
    calls = _record_steps(drv)
    drv.run(nsteps=25)
    scratch, block = drv.block.scratch.data_ptr(), drv.diag.data_ptr()
    drv.engine.close()
    assert [c[0] for c in calls] == [L.DIAG_OUT_LEVEL] * 25
    assert [c[1] for c in calls] == ([scratch] * 11 + [block]) * 2 + [scratch]
    # the option off: as ever, and nothing is allocated
    drv = driver.OfflineDriver(_cfg(tmp_path, "off"), _cols(traj), forcing=ff)
    assert drv.intstats is None and drv.block.intstats is None
    calls = _record_steps(drv)
    drv.run(nsteps=13)
    drv.engine.close()
    assert [c[0] for c in calls] == [L.DIAG_NONE] * 11 + [L.DIAG_OUT_LEVEL] + [L.DIAG_NONE]


# ---- restart inside an interval ---------------------------------------------------------
def test_restart_mid_interval_npz(ist_run, twin32, traj, tmp_path):
    g = traj
    ff = lambda step, t: g["forcing"][step]  # noqa: E731
    a = driver.OfflineDriver(_cfg(tmp_path, "first"), _cols(g), forcing=ff, interval_stats=SPEC)
    a.run(nsteps=40)
    assert a.intstats.k == 4
    path = str(tmp_path / "r.npz")
    a.save_restart(path)
    a.engine.close()
    with np.load(path) as z:
        assert str(z["ist_spec"]) == IS.spec_string(ITEMS) and int(z["ist_steps"]) == 4
        assert z["ist_acc"].shape == (len(ITEMS), 32) and z["ist_acc"].dtype == np.float64
        assert z["ist_cnt"].shape == (3 * len(ITEMS), 32) and z["ist_cnt"].dtype == np.int32
    cfg = _cfg(tmp_path, "second")
    b = driver.OfflineDriver(cfg, _cols(g), forcing=ff, interval_stats=SPEC)
    b.load_restart(path)
    assert b.step_index == 40 and b.intstats.k == 4
    b.run()
    assert bit_equal(b.cs.state.cpu().numpy(), g["states"][-1]).all()
    b.engine.close()
    files = _npz_files(cfg.outdir)
    assert [os.path.basename(f) for f in files] == \
        [os.path.basename(f) for f in ist_run["ist"]["files"][3:]]
    for got, want in zip(files, ist_run["ist"]["files"][3:]):
        assert _npz_members(got) == _npz_members(want), got
    # a restart without the arrays, and one taken under another spec, start a fresh interval
    plain = driver.OfflineDriver(_cfg(tmp_path, "p"), _cols(g), forcing=ff, write=False)
    plain.run(nsteps=40)
    p2 = str(tmp_path / "plain.npz")
    plain.save_restart(p2)
    plain.engine.close()
    assert "ist_acc" not in np.load(p2).files
    other = driver.OfflineDriver(_cfg(tmp_path, "o"), _cols(g), forcing=ff,
                                 interval_stats=SPEC.replace("273.15", "273.16"))
    other.run(nsteps=40)
    p3 = str(tmp_path / "other.npz")
    other.save_restart(p3)
    other.engine.close()
    steps = [_ref_step(g, twin32, k) for k in range(40, 48)]
    want = _want_rows(steps)
    for sub, rpath in (("third", p2), ("fourth", p3)):
        cfg = _cfg(tmp_path, sub)
        c = driver.OfflineDriver(cfg, _cols(g), forcing=ff, interval_stats=SPEC)
        c.load_restart(rpath)
        assert c.step_index == 40 and c.intstats.k == 0
        c.run(nsteps=8)
        c.engine.close()
        with np.load(_npz_files(cfg.outdir)[0], allow_pickle=False) as z:
            d = z["diag"]
        for i, name in enumerate(NAMES):
            assert same_bits(d[16 + i], want[i]), (sub, name)
        # the durations count from the restart: at most 8 steps
        assert (d[16 + NAMES.index("WET_DUR")] <= 8 * 900.0).all()


def test_restart_mid_interval_netcdf(case, twin32, traj, tmp_path):
    grid = case["grid"]
    cfg = config.Config(case["nml"])
    cfg.outdir = str(tmp_path / "first")
    a = driver.OfflineDriver.from_files(cfg, interval_stats=SPEC).run(nsteps=40)
    path = str(tmp_path / "RESTART.nc")
    a.save_restart(path)
    a.engine.close()
    got = ncio.read_intstats(path, grid)
    assert got is not None and got[2] == 4 and got[3] == IS.spec_string(ITEMS)
    assert got[0].dtype == np.float64 and got[1].dtype == np.int32
    cfg.outdir = str(tmp_path / "second")
    b = driver.OfflineDriver.from_files(cfg, init=path, interval_stats=SPEC)
    assert b.step_index == 40 and b.intstats.k == 4
    b.run()
    b.engine.close()
    files, want = _netcdf_files(cfg.outdir), _netcdf_files(case["only"]["outdir"])
    assert [os.path.basename(f) for f in files] == [os.path.basename(f) for f in want[3:]]
    for x, y in zip(files, want[3:]):
        assert open(x, "rb").read() == open(y, "rb").read(), x
    # load_restart of the same file into a constructed driver resumes it as well
    cfg.outdir = str(tmp_path / "third")
    c = driver.OfflineDriver.from_files(cfg, interval_stats=SPEC)
    c.load_restart(path)
    assert c.step_index == 40 and c.intstats.k == 4
    c.run(nsteps=8)
    c.engine.close()
    x = _netcdf_files(cfg.outdir)
    assert len(x) == 1 and open(x[0], "rb").read() == open(want[3], "rb").read()
    # a run without the option ignores the restart's extra variables
    cfg.outdir = str(tmp_path / "plain")
    p = driver.OfflineDriver.from_files(cfg, init=path, write=False).run()
    assert bit_equal(p.to_grid_order(p.cs.state.cpu().numpy()), traj["states"][-1]).all()
    p.engine.close()
    # a netCDF restart without the variables starts a fresh interval there
    p = driver.OfflineDriver.from_files(cfg, write=False).run(nsteps=40)
    bare = str(tmp_path / "BARE.nc")
    p.save_restart(bare)
    p.engine.close()
    assert ncio.read_intstats(bare, grid) is None
    cfg.outdir = str(tmp_path / "fourth")
    d = driver.OfflineDriver.from_files(cfg, init=bare, interval_stats=SPEC)
    assert d.step_index == 40 and d.intstats.k == 0
    d.run(nsteps=8)
    d.engine.close()
    x = _netcdf_files(cfg.outdir)
    assert len(x) == 1
    got = ncio.read_ldasout(x[0], grid, L.DIAG_OUT + NAMES)
    want_rows = _want_rows([_ref_step(traj, twin32, k) for k in range(40, 48)])
    for i, name in enumerate(NAMES):
        assert same_bits(got[16 + i], want_rows[i]), name


# ---- spin-up, then the run ---------------------------------------------------------------
def test_spinup_then_run_starts_a_fresh_interval(engine_lib, traj, tmp_path):
    g = traj
    ff = lambda step, t: g["forcing"][step]  # noqa: E731
    a = driver.OfflineDriver(_cfg(tmp_path, "spun"), _cols(g), forcing=ff, interval_stats=SPEC)
    a.spinup(2, report=False)
    assert a.intstats.k == 0 and a.step_index == 0
    state, isnow = a.cs.state.cpu().numpy(), a.cs.isnow.cpu().numpy()
    assert not bit_equal(state, g["state0"]).all()
    a.run(nsteps=12)
    a.engine.close()
    cfg = _cfg(tmp_path, "fresh")
    b = driver.OfflineDriver(cfg, _cols(g, state, isnow), forcing=ff, interval_stats=SPEC)
    b.run(nsteps=12)
    b.engine.close()
    fa, fb = _npz_files(str(tmp_path / "spun")), _npz_files(cfg.outdir)
    assert len(fa) == len(fb) == 1
    assert _npz_members(fa[0]) == _npz_members(fb[0])
    # and they are the restatement's on a twin run from the spun-up state
    diags, states = _twin(g, 4, 12, state, isnow)
    want = _want_rows([(diags[k], g["forcing"][k], states[k]) for k in range(12)])
    with np.load(fa[0], allow_pickle=False) as z:
        assert same_bits(z["diag"][16:], want)


# ---- two ranks ---------------------------------------------------------------------------
def _intstats_rank(rank, world, port, nml):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    drv = driver.OfflineDriver.from_files(config.Config(nml), interval_stats=SPEC)
    assert drv.gather.nfield == 16 + NIST
    drv.run()
    dist.barrier()
    drv.engine.close()
    dist.destroy_process_group()


def test_two_ranks_write_the_single_rank_files(case):
    import socket
    import torch.multiprocessing as mp
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    mp.start_processes(_intstats_rank, args=(2, port, case["nml"]), nprocs=2, start_method="spawn")
    multi = _netcdf_files(config.Config(case["nml"]).outdir)
    single = _netcdf_files(case["only"]["outdir"])
    assert len(multi) == len(single) == 8
    for a, b in zip(multi, single):
        assert os.path.basename(a) == os.path.basename(b)
        assert open(a, "rb").read() == open(b, "rb").read(), a


# ---- fp64 ---------------------------------------------------------------------------------
def test_fp64_driver_equals_the_restatement(engine_lib, traj, tmp_path):
    g = traj
    cfg = _cfg(tmp_path)
    drv = driver.OfflineDriver(cfg, _cols(g), forcing=lambda step, t: g["forcing"][step],
                               precision=8, interval_stats=SPEC)
    drv.run(nsteps=12)
    drv.engine.close()
    files = _npz_files(cfg.outdir)
    assert len(files) == 1
    with np.load(files[0], allow_pickle=False) as z:
        d = z["diag"]
    assert d.dtype == np.float64 and d.shape == (16 + NIST, 32)
    diags, states = _twin(g, 8, 12)
    assert same_bits(d[:16], diags[11])
    steps = [(diags[k], g["forcing"][k].astype(np.float64), states[k]) for k in range(12)]
    want = _want_rows(steps, dtype=np.float64)
    for i, name in enumerate(NAMES):
        assert same_bits(d[16 + i], want[i]), name
    # the means are fp64 values of their own, not widened fp32 ones
    tg = d[16 + NAMES.index("TG_MEAN")]
    assert (tg.astype(np.float32).astype(np.float64) != tg).any()
