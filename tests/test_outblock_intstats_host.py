"""The output block's plan with interval statistics, on the host (no GPU, no
library): output.OutputBlock driven with a recording stand-in for the engine
(the idea of test_outblock_host.py) and a column state of CPU tensors.  For
statistics alone and beside each of accumulate, extremes and state_out: the
rows, the regions' rows, the one scratch block, the kernels each range's stream
is handed and their order for a step between output steps and an output step,
the counter's reset, and the interval's way through both restart formats.

The expectations are written out below; nothing of them is computed by
output.py."""
import datetime
import types

import numpy as np
import pytest
import torch

from noahmp_amd import extremes as X, intstats as IS, layout as L, ncio, output, stateout

NCOL, DT, RANGES = 8, 900.0, ((0, 4), (4, 8))
IST_STATE = "TG,SMC1,FROST=SFCTMP@lt273.15:dur+spell+deg,SNOWCOV=SNEQV@gt1"   # no flux item
IST_FLUX = "TAVG=T2M,HEAT=FSH@gt0:deg"                                        # flux items
ROWS = {IST_STATE: ["TG_MEAN", "SMC1_MEAN", "FROST_DUR", "FROST_DEG", "FROST_SPELL",
                    "SNOWCOV_DUR"],
        IST_FLUX: ["TAVG_MEAN", "HEAT_DEG"]}
EXT = "PRCP:max+tmax,TG"          # forcing and state series: 4 rows, no flux series
EXT_FLUX = "FSH"                  # a flux series: 2 rows
N = (NCOL,)
FLUX, FORC, STATE, ACC, BUD = (16, NCOL), (12, NCOL), (L.NSTATE, NCOL), (L.NACC, NCOL), (19, NCOL)


class Recorder:
    """Stands in for Engine: any method call is noted as (name, the shapes of
    its tensor arguments, cols)."""

    def __init__(self):
        self.calls, self.args = [], []

    def __getattr__(self, name):
        def method(*args, stream=None, cols=None, **kw):
            tensors = [a for a in args if isinstance(a, torch.Tensor)]
            self.calls.append((name, tuple(tuple(t.shape) for t in tensors), cols))
            self.args.append((name, args, stream))
        return method


def make_cs(n=NCOL, dtype=torch.float32):
    st = torch.arange(L.NSTATE * n, dtype=dtype).reshape(L.NSTATE, n)
    return types.SimpleNamespace(ncol=n, state=st)


def make_block(ist, acc=False, ext=None, state=None, cs=None):
    eng = Recorder()
    blk = output.OutputBlock(eng, cs or make_cs(), DT, acc, None if ext is None else X.parse(ext),
                             0 if state is None else stateout.parse_groups(state),
                             stat_items=None if ist is None else IS.parse(ist))
    return eng, blk


ACC_STEP = [("accumulate", (FLUX, FORC, ACC))]
ACC_OUT = ACC_STEP + [("water_storage", (N,)), ("accum_finish", (ACC, N, N, BUD))]
X_STEP = [("extremes_update", ((4, NCOL), (4, NCOL), FORC, STATE))]
X_OUT = X_STEP + [("extremes_output", ((4, NCOL), (4, NCOL), (4, NCOL)))]
XF_STEP = [("extremes_update", ((2, NCOL), (2, NCOL), FLUX))]
XF_OUT = XF_STEP + [("extremes_output", ((2, NCOL), (2, NCOL), (2, NCOL)))]
# IST_STATE: 4 items (acc of 4 rows, cnt of 12), reads the forcing and the state; 6 output rows
IS_STEP = [("intstats_update", ((4, NCOL), (12, NCOL), FORC, STATE))]
IS_OUT = IS_STEP + [("intstats_output", ((4, NCOL), (12, NCOL), (6, NCOL)))]
# IST_FLUX: 2 items (2 rows, 6 rows), reads the fluxes only; 2 output rows
IF_STEP = [("intstats_update", ((2, NCOL), (6, NCOL), FLUX))]
IF_OUT = IF_STEP + [("intstats_output", ((2, NCOL), (6, NCOL), (2, NCOL)))]
NSTATE_ROWS = len(stateout.row_names(stateout.ALL))
ST_OUT = [("state_output", ((NSTATE_ROWS, NCOL),))]

# (interval_stats, accumulate, extremes, state_out) -> does a producer read the
# fluxes every step, the calls of a step between output steps, of an output step
EXPECT = {
    (IST_STATE, False, None, None):     (False, IS_STEP, IS_OUT),
    (IST_FLUX, False, None, None):      (True, IF_STEP, IF_OUT),
    (IST_STATE, True, None, None):      (True, ACC_STEP + IS_STEP, ACC_OUT + IS_OUT),
    (IST_FLUX, True, None, None):       (True, ACC_STEP + IF_STEP, ACC_OUT + IF_OUT),
    (IST_STATE, False, EXT, None):      (False, X_STEP + IS_STEP, X_OUT + IS_OUT),
    (IST_STATE, False, EXT_FLUX, None): (True, XF_STEP + IS_STEP, XF_OUT + IS_OUT),
    (IST_FLUX, False, EXT, None):       (True, X_STEP + IF_STEP, X_OUT + IF_OUT),
    (IST_STATE, False, None, "all"):    (False, IS_STEP, IS_OUT + ST_OUT),
    (IST_FLUX, False, None, "all"):     (True, IF_STEP, IF_OUT + ST_OUT),
    (IST_FLUX, True, EXT, "all"):       (True, ACC_STEP + X_STEP + IF_STEP,
                                         ACC_OUT + X_OUT + IF_OUT + ST_OUT),
}


def run_post(eng, post):
    """The calls `post` records for each range on its stream."""
    got = []
    for i, rng in enumerate(RANGES):
        eng.calls.clear(), eng.args.clear()
        post(f"stream{i}", rng)
        assert all(a[2] == f"stream{i}" for a in eng.args)
        got.append(list(eng.calls))
    return got


@pytest.mark.parametrize("ist,acc,ext,state", list(EXPECT))
def test_plan_of_every_run(ist, acc, ext, state):
    needs, between, at_output = EXPECT[(ist, acc, ext, state)]
    eng, blk = make_block(ist, acc, ext, state)
    # construction: an accumulating run forms the interval's beginning storage, nothing else
    assert [c[0] for c in eng.calls] == (["water_storage"] if acc else [])
    # 1. the rows: fluxes, budget rows, extremes rows, statistics rows, state rows
    nflux = 35 if acc else 16
    xrows = {None: [], EXT: ["PRCP_MAX", "PRCP_TMAX", "TG_MAX", "TG_MIN"],
             EXT_FLUX: ["FSH_MAX", "FSH_MIN"]}[ext]
    names = list(L.DIAG_OUT_ACC if acc else L.DIAG_OUT) + xrows + ROWS[ist]
    if state is not None:
        names += stateout.row_names(stateout.ALL)
    assert blk.names == names
    assert tuple(blk.diag.shape) == (len(names), NCOL) and blk.diag.dtype == torch.float32
    # 2. the regions' rows: the statistics rows cannot hold the fill value
    first_state = nflux + len(xrows) + len(ROWS[ist])
    if state is None:
        assert blk.region_rows is None
    else:
        assert blk.region_rows == first_state + stateout.nofill_rows(stateout.ALL)
    # 3. one scratch block, if and only if a flux item or another flux reader is present
    assert (blk.scratch is not None) == needs
    assert blk.intstats.needs_fluxes == (ist == IST_FLUX)
    if needs:
        assert tuple(blk.scratch.shape) == (16, NCOL)
    assert not hasattr(blk.intstats, "scratch")
    assert blk.carried == [p for p in (blk.accum, blk.extremes, blk.intstats) if p is not None]
    assert blk.producers[-1 if state is None else -2] is blk.intstats
    # the resident state: doubles and int32 whatever the engine's precision
    assert blk.intstats.acc.dtype == torch.float64 and blk.intstats.cnt.dtype == torch.int32
    f = torch.zeros(FORC)
    # ---- a step between output steps
    dstep, level, post = blk.plan(f, blk.diag, False)
    if needs:
        assert level == L.DIAG_OUT_LEVEL and dstep.data_ptr() == blk.scratch.data_ptr()
    else:
        assert level == L.DIAG_NONE and dstep is None
    assert blk.intstats.k == 1
    for rng, got in zip(RANGES, run_post(eng, post)):
        assert got == [(n, s, rng) for n, s in between]
    _check_update_args(eng, blk, dstep, f, ist, 1)
    # ---- an output step, into a block of its own (a gather buffer under a process group)
    diag = torch.zeros_like(blk.diag)
    dstep, level, post = blk.plan(f, diag, True)
    assert level == L.DIAG_OUT_LEVEL and dstep.data_ptr() == diag.data_ptr()
    assert blk.intstats.k == 0                   # the counter's reset
    for rng, got in zip(RANGES, run_post(eng, post)):
        assert got == [(n, s, rng) for n, s in at_output]
    _check_update_args(eng, blk, dstep, f, ist, 2)
    # each producer's rows are its own slice of the block, in row order
    row0 = {"accum_finish": 16, "extremes_output": nflux, "intstats_output": nflux + len(xrows),
            "state_output": first_state}
    itemsize = diag.element_size() * NCOL
    seen = set()
    for name, args, _ in eng.args:
        if name in row0:
            rows = [a for a in args if isinstance(a, torch.Tensor)][-1]
            assert rows.data_ptr() == diag.data_ptr() + row0[name] * itemsize, name
            seen.add(name)
        if name == "intstats_output":    # (table, k, dt, acc, cnt, rows): the driver's count
            assert np.array_equal(args[0], IS.table(IS.parse(ist)))
            assert args[1:3] == (2, DT)
            assert args[3] is blk.intstats.acc and args[4] is blk.intstats.cnt
    assert "intstats_output" in seen
    # the next interval counts from 1 again
    blk.plan(f, blk.diag, False)
    assert blk.intstats.k == 1


def _check_update_args(eng, blk, dstep, f, ist, k):
    """intstats_update(table, thresholds, k, acc, cnt, fluxes, forcing, state):
    a flux item reads the block the step wrote; a block no item names is None."""
    items = IS.parse(ist)
    (args,) = [a for n, a, _ in eng.args if n == "intstats_update"]
    assert np.array_equal(args[0], IS.table(items)) and args[0].dtype == np.int32
    assert np.array_equal(args[1], IS.thresholds(items)) and args[1].dtype == np.float64
    assert args[2] == k and args[3] is blk.intstats.acc and args[4] is blk.intstats.cnt
    if ist == IST_FLUX:
        assert args[5].data_ptr() == dstep.data_ptr() and args[6] is None and args[7] is None
    else:
        assert args[5] is None and args[6] is f and args[7] is blk.intstats.cs.state
    for name, a, _ in eng.args:
        if name == "accumulate":
            assert a[0].data_ptr() == dstep.data_ptr()


def test_off_is_the_block_as_it_was():
    """The trailing argument defaults to None: no producer, nothing allocated."""
    eng = Recorder()
    blk = output.OutputBlock(eng, make_cs(), DT, True, X.parse(EXT), stateout.ALL)
    assert blk.intstats is None and blk.carried == [blk.accum, blk.extremes]
    assert len(blk.producers) == 4
    assert blk.names == L.DIAG_OUT_ACC + X.row_names(X.parse(EXT)) + \
        stateout.row_names(stateout.ALL)
    _, _, post = blk.plan(torch.zeros(FORC), blk.diag, True)
    eng.calls.clear()
    post("s", (0, NCOL))
    assert [c[0] for c in eng.calls] == ["accumulate", "water_storage", "accum_finish",
                                         "extremes_update", "extremes_output", "state_output"]


def test_enqueue_order_and_region_rows_of_the_full_run():
    eng, blk = make_block(IST_FLUX, True, "FSH,TG,PRCP:max+tmax", "all")
    assert blk.names[:35] == L.DIAG_OUT_ACC
    assert blk.names[35:41] == ["FSH_MAX", "FSH_MIN", "TG_MAX", "TG_MIN", "PRCP_MAX", "PRCP_TMAX"]
    assert blk.names[41:43] == ["TAVG_MEAN", "HEAT_DEG"]
    assert blk.names[43:] == stateout.row_names(stateout.ALL)
    assert blk.region_rows == 35 + 6 + 2 + 32 == 75
    _, _, post = blk.plan(torch.zeros(FORC), blk.diag, True)
    eng.calls.clear()
    post("s", (0, NCOL))
    assert [c[0] for c in eng.calls] == ["accumulate", "water_storage", "accum_finish",
                                         "extremes_update", "extremes_output",
                                         "intstats_update", "intstats_output", "state_output"]


def test_a_row_name_that_occurs_twice_is_refused():
    # accumulation's T2M_MEAN and FSH_MEAN: the default label of a flux's mean collides
    for spec in ("T2M", "FSH,TG", "X=TG@gt1,T2M=TG"):
        with pytest.raises(ValueError, match="occur twice"):
            make_block(spec, acc=True)
        make_block(spec, acc=False)
    make_block("TAVG=T2M", acc=True)
    # (a statistics row ends in _MEAN, _DUR, _DEG or _SPELL: no flux, extremes or
    # state-output row does, so with those any label passes)
    make_block("TG_MAX=TG@gt1,SOIL_M=SMC1,LAI=LAI", ext="TG", state="all")


# ---- the interval's way through the restart formats ------------------------------------------
def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same_state(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        if isinstance(x, np.ndarray):
            assert x.dtype == y.dtype and x.shape == y.shape and np.array_equal(bits(x), bits(y))
        else:
            assert x == y and type(x) is type(y)


def fill_interval(blk, seed):
    """Part way through an interval: arbitrary sums and counters."""
    g = torch.Generator().manual_seed(seed)
    p = blk.intstats
    p.acc.copy_(torch.randn(p.acc.shape, generator=g, dtype=torch.float64))
    p.acc[0, 0], p.acc[1, 1], p.acc[2, 2] = -0.0, float("nan"), float("inf")
    p.cnt.copy_(torch.randint(0, 6, p.cnt.shape, generator=g, dtype=torch.int32))
    p.k = 5
    if blk.accum is not None:
        blk.accum.acc.copy_(torch.randn(blk.accum.acc.shape, generator=g, dtype=torch.float64))
        blk.accum.steps = 5


def test_payload_names():
    _, blk = make_block(IST_STATE)
    assert blk.intstats.npz == ("ist_acc", "ist_cnt", "ist_steps", "ist_spec")
    assert blk.intstats.nc == ("intstats", ncio.read_intstats)
    assert blk.intstats.spec == ("TG:mean,SMC1:mean,FROST=SFCTMP@lt273.15:dur+deg+spell,"
                                 "SNOWCOV=SNEQV@gt1.0:dur")


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_interval_round_trips_through_both_formats(tmp_path, dtype):
    _, a = make_block(IST_STATE, acc=True, cs=make_cs(dtype=dtype))
    fill_interval(a, 1)
    want = [p.state() for p in a.carried]
    assert want[1][0].dtype == np.float64 and want[1][0].shape == (4, NCOL)
    assert want[1][1].dtype == np.int32 and want[1][1].shape == (12, NCOL)
    assert want[1][2:] == (5, a.intstats.spec)
    # npz: the items as a restart stores them
    path = str(tmp_path / "r.npz")
    np.savez(path, **{k: np.int64(v) if isinstance(v, int) else np.asarray(v)
                      for p, st in zip(a.carried, want) for k, v in zip(p.npz, st)})
    eng, b = make_block(IST_STATE, acc=True, cs=make_cs(dtype=dtype))
    eng.calls.clear()
    with np.load(path, allow_pickle=False) as z:
        assert z.files == ["acc", "stor_beg", "acc_steps", "ist_acc", "ist_cnt", "ist_steps",
                           "ist_spec"]
        for p in b.carried:
            p.restore(tuple(z[k] for k in p.npz))
    assert eng.calls == []
    for p, w in zip(b.carried, want):
        same_state(p.state(), w)
    # netCDF: a 4 x 4 grid with 8 land points, the columns in another order than the grid's
    mask = np.array([[1, 0, 1, 0], [0, 1, 1, 0], [0, 0, 1, 1], [1, 0, 0, 1]], bool)
    grid = ncio.Grid(np.zeros((4, 4)), np.zeros((4, 4)), mask)
    assert grid.n == NCOL
    perm = np.array([5, 2, 7, 0, 3, 6, 1, 4])

    def to_grid_order(v):
        out = np.empty_like(v)
        out[..., perm] = v
        return out
    kw = {p.nc[0]: tuple(to_grid_order(v) if isinstance(v, np.ndarray) else v for v in st)
          for p, st in zip(a.carried, want)}
    assert sorted(kw) == ["accum", "intstats"]
    path = str(tmp_path / "r.nc")
    npdt = np.float32 if dtype == torch.float32 else np.float64
    ncio.write_state(path, grid, np.zeros((L.NSTATE, NCOL), npdt), np.zeros(NCOL, np.int32),
                     datetime.datetime(2000, 1, 1, 10), 40, **kw)
    eng, c = make_block(IST_STATE, acc=True, cs=make_cs(dtype=dtype))
    eng.calls.clear()
    for p in c.carried:
        p.restore(p.nc[1](path, grid), perm)
    assert eng.calls == []
    for p, w in zip(c.carried, want):
        same_state(p.state(), w)
    # a file without the interval: both read None
    ncio.write_state(path, grid, np.zeros((L.NSTATE, NCOL), npdt), np.zeros(NCOL, np.int32),
                     datetime.datetime(2000, 1, 1, 10), 40)
    assert [p.nc[1](path, grid) for p in c.carried] == [None, None]


def test_restore_none_and_another_spec_start_fresh():
    eng, blk = make_block(IST_STATE)
    fill_interval(blk, 2)
    carried = blk.intstats.state()
    eng.calls.clear()
    blk.intstats.restore(None)
    # no launch: the next step is the interval's first and reads no old sum
    assert eng.calls == [] and blk.intstats.k == 0
    # under another spec (another threshold is enough) the carried interval does not apply
    _, other = make_block(IST_STATE.replace("273.15", "273.16"))
    before = other.intstats.state()
    other.intstats.restore(carried)
    assert other.intstats.k == 0
    same_state(other.intstats.state(), before)
    # under the same spec it does
    _, same = make_block(IST_STATE, acc=True)
    same.intstats.restore(carried)
    same_state(same.intstats.state(), carried)
    assert same.intstats.k == 5
