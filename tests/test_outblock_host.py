"""The output block's plan, on the host (no GPU, no library): output.OutputBlock
and its producers driven with a recording stand-in for the engine and a column
state of CPU tensors.  Per run of the option matrix, for a step between output
steps and an output step: the rows, the regions' rows, where the step writes its
fluxes and at which level, the one scratch block, the kernels each range's
stream is handed and their order, the interval counters, and the interval's way
through both restart formats.

The expectations are written out below; nothing of them is computed by
output.py."""
import datetime
import types

import numpy as np
import pytest
import torch

from noahmp_amd import extremes as X, layout as L, ncio, output, stateout

NCOL, DT, RANGES = 8, 900.0, ((0, 4), (4, 8))
EXT_STATE = "PRCP:max+tmax,TG,SMC1"   # forcing and state series: no flux series
EXT_FLUX = "FSH,TG"                   # a flux series
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


def make_block(acc, ext, state, cs=None):
    eng = Recorder()
    blk = output.OutputBlock(eng, cs or make_cs(), DT, acc, None if ext is None else X.parse(ext),
                             0 if state is None else stateout.parse_groups(state))
    return eng, blk


# what each producer enqueues for one range: (name, shapes of the tensor arguments)
ACC_STEP = [("accumulate", (FLUX, FORC, ACC))]
ACC_OUT = ACC_STEP + [("water_storage", (N,)), ("accum_finish", (ACC, N, N, BUD))]
# EXT_STATE: 3 series (val, when of 6 rows), reads the forcing and the state; 6 output rows
XS_STEP = [("extremes_update", ((6, NCOL), (6, NCOL), FORC, STATE))]
XS_OUT = XS_STEP + [("extremes_output", ((6, NCOL), (6, NCOL), (6, NCOL)))]
# EXT_FLUX: 2 series (4 rows), reads the fluxes and the state; 4 output rows
XF_STEP = [("extremes_update", ((4, NCOL), (4, NCOL), FLUX, STATE))]
XF_OUT = XF_STEP + [("extremes_output", ((4, NCOL), (4, NCOL), (4, NCOL)))]
NSTATE_ROWS = len(stateout.row_names(stateout.ALL))
ST_OUT = [("state_output", ((NSTATE_ROWS, NCOL),))]

# (accumulate, extremes, state_out) -> does a producer read the fluxes every step,
# the calls of a step between output steps, the calls of an output step
EXPECT = {
    (False, None, None):       (False, [], []),
    (False, None, "all"):      (False, [], ST_OUT),
    (False, EXT_STATE, None):  (False, XS_STEP, XS_OUT),
    (False, EXT_STATE, "all"): (False, XS_STEP, XS_OUT + ST_OUT),
    (False, EXT_FLUX, None):   (True, XF_STEP, XF_OUT),
    (False, EXT_FLUX, "all"):  (True, XF_STEP, XF_OUT + ST_OUT),
    (True, None, None):        (True, ACC_STEP, ACC_OUT),
    (True, None, "all"):       (True, ACC_STEP, ACC_OUT + ST_OUT),
    (True, EXT_STATE, None):   (True, ACC_STEP + XS_STEP, ACC_OUT + XS_OUT),
    (True, EXT_STATE, "all"):  (True, ACC_STEP + XS_STEP, ACC_OUT + XS_OUT + ST_OUT),
    (True, EXT_FLUX, None):    (True, ACC_STEP + XF_STEP, ACC_OUT + XF_OUT),
    (True, EXT_FLUX, "all"):   (True, ACC_STEP + XF_STEP, ACC_OUT + XF_OUT + ST_OUT),
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


@pytest.mark.parametrize("acc,ext,state", list(EXPECT))
def test_plan_of_every_run(acc, ext, state):
    needs, between, at_output = EXPECT[(acc, ext, state)]
    eng, blk = make_block(acc, ext, state)
    # construction: an accumulating run forms the interval's beginning storage, nothing else
    assert [c[0] for c in eng.calls] == (["water_storage"] if acc else [])
    # 1. the rows
    next_ = 0 if ext is None else len(X.row_names(X.parse(ext)))
    assert next_ == {None: 0, EXT_STATE: 6, EXT_FLUX: 4}[ext]
    names = list(L.DIAG_OUT_ACC if acc else L.DIAG_OUT)
    nflux = 35 if acc else 16
    assert len(names) == nflux
    if ext is not None:
        names += X.row_names(X.parse(ext))
    if state is not None:
        names += stateout.row_names(stateout.ALL)
    assert blk.names == names
    assert tuple(blk.diag.shape) == (len(names), NCOL) and blk.diag.dtype == torch.float32
    # 2. the regions' rows
    if state is None:
        assert blk.region_rows is None
    else:
        assert blk.region_rows == nflux + next_ + stateout.nofill_rows(stateout.ALL)
    # 4. one scratch block, if and only if a producer reads the fluxes
    assert (blk.scratch is not None) == needs
    assert any(p.needs_fluxes for p in blk.producers) == needs
    if needs:
        assert tuple(blk.scratch.shape) == (16, NCOL) and blk.scratch.dtype == torch.float32
    assert not hasattr(blk.accum, "acc_diag") and not hasattr(blk.extremes, "scratch")
    assert (blk.accum is not None) == acc and (blk.extremes is not None) == (ext is not None)
    assert blk.carried == [p for p in (blk.accum, blk.extremes) if p is not None]
    f = torch.zeros(FORC)
    # ---- a step between output steps
    dstep, level, post = blk.plan(f, blk.diag, False)
    if needs:   # 3. level and destination
        assert level == L.DIAG_OUT_LEVEL and dstep.data_ptr() == blk.scratch.data_ptr()
        assert tuple(dstep.shape) == (16, NCOL)
    else:
        assert level == L.DIAG_NONE and dstep is None
    if acc:     # 6. the counters
        assert blk.accum.steps == 1
    if ext is not None:
        assert blk.extremes.k == 1
    if not between:   # 5. the enqueue order
        assert post is None
    else:
        for rng, got in zip(RANGES, run_post(eng, post)):
            assert got == [(n, s, rng) for n, s in between]
        _check_flux_reader(eng, dstep, ext)
    # ---- an output step, into a block of its own (a gather buffer under a process group)
    diag = torch.zeros_like(blk.diag)
    dstep, level, post = blk.plan(f, diag, True)
    assert level == L.DIAG_OUT_LEVEL and dstep.data_ptr() == diag.data_ptr()
    assert tuple(dstep.shape) == (16, NCOL) and dstep.stride() == diag.stride()
    if acc:
        assert blk.accum.steps == 0
    if ext is not None:
        assert blk.extremes.k == 0
    if not at_output:
        assert post is None
        return
    for rng, got in zip(RANGES, run_post(eng, post)):
        assert got == [(n, s, rng) for n, s in at_output]
    _check_flux_reader(eng, dstep, ext)
    # each producer's rows are its own slice of the block, in row order
    row0 = {"accum_finish": 16, "extremes_output": nflux, "state_output": nflux + next_}
    itemsize = diag.element_size() * NCOL
    for name, args, _ in eng.args:
        if name in row0:
            rows = [a for a in args if isinstance(a, torch.Tensor)][-1]
            assert rows.data_ptr() == diag.data_ptr() + row0[name] * itemsize, name
    # the interval's span and the step of the interval reach the kernels
    for name, args, _ in eng.args:
        if name == "accum_finish":
            assert args[-1] == 2 * DT
        if name == "extremes_update":
            assert args[1] == 2
    if state is not None:
        name, args, _ = eng.args[-1]
        assert name == "state_output" and args[1] == stateout.ALL and args[3] == float(ncio.FILL)


def _check_flux_reader(eng, dstep, ext):
    """accumulate and a flux series' extremes_update read the block the step wrote."""
    for name, args, _ in eng.args:
        if name == "accumulate":
            assert args[0].data_ptr() == dstep.data_ptr()
        if name == "extremes_update":
            assert (args[4] is None) == (ext != EXT_FLUX)
            if ext == EXT_FLUX:
                assert args[4].data_ptr() == dstep.data_ptr()


def test_region_rows_of_the_full_run():
    """35 flux and budget rows, the 6 extremes rows of the three series, and the
    32 state rows that cannot hold the fill value."""
    _, blk = make_block(True, "FSH,TG,PRCP:max+tmax", "all")
    assert blk.names[:35] == L.DIAG_OUT_ACC
    assert blk.names[35:41] == ["FSH_MAX", "FSH_MIN", "TG_MAX", "TG_MIN", "PRCP_MAX", "PRCP_TMAX"]
    assert blk.names[41:] == stateout.row_names(stateout.ALL)
    assert stateout.nofill_rows(stateout.ALL) == 32
    assert blk.region_rows == 35 + 6 + 32 == 73


def test_enqueue_order_of_the_two_carried_producers():
    eng, blk = make_block(True, EXT_FLUX, None)
    _, _, post = blk.plan(torch.zeros(FORC), blk.diag, True)
    post("s", (0, NCOL))
    assert [c[0] for c in eng.calls] == ["water_storage", "accumulate", "water_storage",
                                         "accum_finish", "extremes_update", "extremes_output"]


def test_chain():
    assert output.chain([]) is None and output.chain([None, None]) is None
    seen = []
    a = lambda st, rng: seen.append(("a", st, rng))  # noqa: E731
    b = lambda st, rng: seen.append(("b", st, rng))  # noqa: E731
    assert output.chain([None, a]) is a and output.chain((b, None)) is b
    output.chain([a, None, b])("s", (0, 4))
    assert seen == [("a", "s", (0, 4)), ("b", "s", (0, 4))]


# ---- 7. the interval's way through the restart formats --------------------------------------
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
    """Part way through an interval: arbitrary accumulators and extremes."""
    g = torch.Generator().manual_seed(seed)
    for p in blk.carried:
        if p is blk.accum:
            p.acc.copy_(torch.randn(p.acc.shape, generator=g, dtype=torch.float64))
            p.stor_beg.copy_(torch.randn(p.stor_beg.shape, generator=g))
            p.steps = 5
        else:
            p.val.copy_(torch.randn(p.val.shape, generator=g))
            p.val[0, 0], p.val[1, 1] = -0.0, float("nan")
            p.when.copy_(torch.randint(1, 6, p.when.shape, generator=g, dtype=torch.int32))
            p.k = 5


def test_payload_names():
    _, blk = make_block(True, EXT_FLUX, None)
    assert blk.accum.npz == ("acc", "stor_beg", "acc_steps")
    assert blk.extremes.npz == ("ext_val", "ext_when", "ext_steps", "ext_spec")
    assert blk.accum.nc == ("accum", ncio.read_accum)
    assert blk.extremes.nc == ("extremes", ncio.read_extremes)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_interval_round_trips_through_both_formats(tmp_path, dtype):
    _, a = make_block(True, EXT_STATE, None, make_cs(dtype=dtype))
    fill_interval(a, 1)
    want = [p.state() for p in a.carried]
    assert want[0][2] == 5 and want[1][2:] == (5, "PRCP:max+tmax,TG:max+min,SMC1:max+min")
    # npz: the items as a restart stores them
    path = str(tmp_path / "r.npz")
    np.savez(path, **{k: np.int64(v) if isinstance(v, int) else np.asarray(v)
                      for p, st in zip(a.carried, want) for k, v in zip(p.npz, st)})
    eng, b = make_block(True, EXT_STATE, None, make_cs(dtype=dtype))
    eng.calls.clear()
    with np.load(path, allow_pickle=False) as z:
        assert z.files == ["acc", "stor_beg", "acc_steps", "ext_val", "ext_when", "ext_steps",
                           "ext_spec"]
        for p in b.carried:
            p.restore(tuple(z[k] for k in p.npz))
    assert eng.calls == []          # a resumed interval keeps its beginning storage
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
    assert sorted(kw) == ["accum", "extremes"]
    path = str(tmp_path / "r.nc")
    npdt = np.float32 if dtype == torch.float32 else np.float64
    ncio.write_state(path, grid, np.zeros((L.NSTATE, NCOL), npdt), np.zeros(NCOL, np.int32),
                     datetime.datetime(2000, 1, 1, 10), 40, **kw)
    eng, c = make_block(True, EXT_STATE, None, make_cs(dtype=dtype))
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
    eng, blk = make_block(True, EXT_STATE, None)
    fill_interval(blk, 2)
    carried = [p.state() for p in blk.carried]
    eng.calls.clear()
    for p in blk.carried:
        p.restore(None)
    # accumulation: zero accumulators, the beginning storage formed anew from the state
    assert eng.calls == [("water_storage", (N,), None)]
    assert blk.accum.steps == 0 and not blk.accum.acc.any()
    # extremes: the next step is the interval's first (k = 1 takes any value)
    assert blk.extremes.k == 0
    # under another spec the carried extremes do not apply; accumulation has no spec
    _, other = make_block(True, "PRCP:max+tmax,TG,SMC2", None)
    before = other.extremes.state()
    other.extremes.restore(carried[1])
    assert other.extremes.k == 0
    same_state(other.extremes.state(), before)
    other.accum.restore(carried[0])
    same_state(other.accum.state(), carried[0])
    # under the same spec they do
    _, same = make_block(False, EXT_STATE, None)
    same.extremes.restore(carried[1])
    same_state(same.extremes.state(), carried[1])
