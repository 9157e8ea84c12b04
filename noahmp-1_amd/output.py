"""The output side of the offline driver (driver.OfflineDriver).

An output file's rows come from producers with one interface, as the forcing
comes from feeds (feeds._Feed): `Fluxes`, `Accumulation`, `Extremes`, `IntervalStats`,
`StateRows`.
A producer has `names` (its rows), `needs_fluxes` (does it read the step's 16
fluxes on every step) and `step(f, fluxes, rows)`: one more step with the
forcing `f`, its fluxes in `fluxes` (None unless `needs_fluxes`) and, at an
output step, `rows`, the producer's slice of the output block (else None).  It
returns the hook `hook(stream, (lo, hi))` that enqueues the producer's kernels
for a column range after the step, or None.  One that carries an interval also
has `state()`, `restore(state | None, idx)`, `npz` (its npz items, in state()'s
order) and `nc` (ncio.write_state's keyword, the function that reads it back).

`OutputBlock` composes a run's producers: the rows' layout, the one scratch
block and each step's plan.  `OutputWriter` stages an output step's block and
writes its files on background threads."""
from __future__ import annotations

import datetime
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import extremes as X, intstats as IS, layout as L, ncio, stateout


def chain(hooks):
    """One StreamShards hook `hook(stream, (lo, hi))` from several, None among
    them: none is None, one is itself, more are called in order."""
    hooks = [h for h in hooks if h is not None]
    if len(hooks) < 2:
        return hooks[0] if hooks else None

    def hook(st, rng):
        for h in hooks:
            h(st, rng)
    return hook


class OutputWriter:
    """LDASOUT (and REGIONS) files of the output steps, written while the loop
    goes on stepping.  A single rank's output is laid on the file's grids
    (nmp_ldasout_grid) and copied on a stream of its own and written by writer
    threads (ncio.write_ldasout_grids).

    block: the run's OutputBlock -- the rows' names, and `region_rows`, the
    leading rows the regions reduce (None: all of them; a run with state
    output leaves out its trailing rows, which can hold the fill value).
    `stage` (the rank that writes, in a run that writes output) allocates the
    staging buffers up front: a page-locked allocation of the whole set's
    fluxes costs tens of ms inside the time loop (the file's grids in its byte
    order when the run has a grid; none for a regions-only run).  perm: the
    land point of each engine column (None = grid order)."""
    # output files in flight at once (writer threads) and staging buffers: a
    # file's write is a memory copy into the page cache on its own thread
    OUT_WRITERS, OUT_BUFFERS = 2, 3

    def __init__(self, engine, cfg, grid, block, ncol_total: int, dtype, dev, stage: bool,
                 region_plan=None, write_grids: bool = True, perm=None):
        self.engine, self.cfg, self.grid, self.out_names = engine, cfg, grid, block.names
        self.dev, self.region_plan, self.write_grids, self.perm = dev, region_plan, write_grids, perm
        self.written, self.regions_written = [], []
        nout = len(self.out_names)
        self.region_rows = nout if block.region_rows is None else block.region_rows
        self._writer = ThreadPoolExecutor(self.OUT_WRITERS)
        self._out_host = [None] * self.OUT_BUFFERS
        if stage and write_grids:
            shape = (nout, ncol_total)
            if grid is not None:
                shape = (nout, grid.shape[0] * grid.shape[1])
                dtype = torch.int32 if dtype == torch.float32 else torch.int64
            self._out_host = [torch.empty(shape, dtype=dtype, pin_memory=True)
                              for _ in range(self.OUT_BUFFERS)]
        self._out_fut, self._n_out_w = [None] * self.OUT_BUFFERS, 0
        # the columns' grid points and the device grids, from their first use on
        self._out_point, self._out_dev = None, None
        self._reg_dev, self._reg_host = None, [None] * self.OUT_BUFFERS
        if region_plan is not None:
            # sums and means of an output step, and their pinned staging buffers
            self._reg_dev = torch.zeros((2, self.region_rows, region_plan.nreg),
                                        dtype=torch.float64, device=dev)
            self._reg_host = [torch.empty((2, self.region_rows, region_plan.nreg),
                                          dtype=torch.float64,
                                          pin_memory=True) for _ in range(self.OUT_BUFFERS)]

    def point(self) -> torch.Tensor:
        """The grid point of every engine column (int32, on the device)."""
        if self._out_point is None:
            idx = np.asarray(self.grid.index)
            self._out_point = torch.as_tensor(
                (idx if self.perm is None else idx[self.perm]).astype(np.int32), device=self.dev)
        return self._out_point

    def _grids(self, d: torch.Tensor, stream) -> torch.Tensor:
        """d laid on the file's grids in its byte order, on `stream`."""
        point = self.point()
        if self._out_dev is None:
            npts = self.grid.shape[0] * self.grid.shape[1]
            self._out_dev = torch.empty((d.shape[0], npts), device=self.dev,
                                        dtype=torch.int32 if d.dtype == torch.float32
                                        else torch.int64)
        # (nmp_ldasout_grid takes at most NDIAG_FULL rows a call)
        for r in range(0, d.shape[0], L.NDIAG_FULL):
            self.engine.ldasout_grid(d[r:r + L.NDIAG_FULL], point,
                                     self._out_dev[r:r + L.NDIAG_FULL], float(ncio.FILL),
                                     stream=stream)
        return self._out_dev

    def write(self, d: torch.Tensor, path: str, t1: datetime.datetime, stream):
        """One output step's (16, n) fluxes (35 fields with accumulation),
        written on a background thread:
        on `stream` (after the step that produced them) the engine lays them
        on the file's grids in its byte order (nmp_ldasout_grid)
        and they are copied into the next of OUT_BUFFERS pinned host buffers;
        a writer thread (OUT_WRITERS of them) waits for the copy and writes
        the header and the bytes (ncio.write_ldasout_grids) while the loop
        goes on stepping.  A buffer is reused once its previous file is
        written.  Returns the event after which `d` has been read.
        With regions the block is also reduced to the regions' sums and means
        on `stream` (nmp_region_reduce), which go to a small pinned buffer of
        the same slot; the same writer job writes the REGIONS file.  The event
        covers the reduce.  write_grids=False leaves only that."""
        src = None
        if self.write_grids:
            src = d if self.grid is None else self._grids(d, stream)
            self.written.append(path)
        k = self._n_out_w % self.OUT_BUFFERS
        self._n_out_w += 1
        if self._out_fut[k] is not None:
            self._out_fut[k].result()
        h, rh, rpath = self._out_host[k], None, None
        if self.region_plan is not None:
            rh, rpath = self._reg_host[k], ncio.regions_path(self.cfg.outdir, t1)
            self.engine.region_reduce(d[:self.region_rows], self.region_plan, self._reg_dev[0],
                                      self._reg_dev[1], stream=stream)
            self.regions_written.append(rpath)
        with torch.cuda.stream(stream):
            if src is not None:
                h.copy_(src, non_blocking=True)
            if rh is not None:
                rh.copy_(self._reg_dev, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(stream)
        self._out_fut[k] = self._writer.submit(self._job, ev, None if src is None else h, path,
                                               rh, rpath, t1)
        return ev

    def _job(self, ev, h, path, rh, rpath, t1):
        """A writer thread's part: the files of one output step, once its copies have landed."""
        ev.synchronize()
        if rh is not None:
            plan = self.region_plan
            ncio.write_regions(rpath, plan.region_id, plan.ncolumns, plan.wsum, rh.numpy()[1], t1,
                               self.out_names[:self.region_rows])
        if h is None:
            return
        a = h.numpy()
        if self.grid is not None:
            ncio.write_ldasout_grids(path, self.grid, a.view(">f4" if a.itemsize == 4 else ">f8"),
                                     t1, self.out_names)
        else:
            np.savez(path, time=np.array(t1.isoformat()), fields=np.array(",".join(self.out_names)),
                     diag=a)

    def flush(self):
        """Wait until every output file issued so far is written (raises a
        writer's error)."""
        for f in self._out_fut:
            if f is not None:
                f.result()


class Fluxes:
    """The output step's 16 surface fluxes: the step kernel writes them into
    their rows itself, so there is nothing to enqueue after it."""
    names, needs_fluxes = L.DIAG_OUT, False

    def step(self, f, fluxes, rows):
        return None


class Accumulation:
    """An output interval's accumulated output (layout.BUDGET), on the device:
    the accumulators `acc` (every step's fluxes are added up), the water storage
    at the interval's beginning and end, and `steps`, the steps added up so far."""
    names, needs_fluxes = L.BUDGET, True
    npz, nc = ("acc", "stor_beg", "acc_steps"), ("accum", ncio.read_accum)

    def __init__(self, engine, cs, dt: float):
        self.engine, self.cs, self.dt = engine, cs, dt
        n, dev, dtype = cs.ncol, cs.state.device, cs.state.dtype
        self.acc = torch.zeros((L.NACC, n), dtype=torch.float64, device=dev)
        self.stor_beg = torch.zeros(n, dtype=dtype, device=dev)
        self.stor_end = torch.zeros(n, dtype=dtype, device=dev)
        self.restore(None)

    def state(self):
        """(acc, stor_beg, steps) of the interval so far, on the host: what a restart carries."""
        return self.acc.cpu().numpy(), self.stor_beg.cpu().numpy(), self.steps

    def restore(self, state, idx=slice(None)):
        """`state` (state(), of the columns `idx` picks) resumes its interval;
        None starts a fresh one: zero accumulators, the beginning storage from
        the model state as it is (nmp_water_storage, on the current stream)."""
        if state is None:
            self.steps = 0
            self.acc.zero_()
            self.engine.water_storage(self.cs, self.stor_beg)
            return
        dev = self.acc.device
        self.acc.copy_(torch.as_tensor(np.ascontiguousarray(state[0][:, idx], np.float64),
                                       device=dev))
        self.stor_beg.copy_(torch.as_tensor(np.ascontiguousarray(state[1][idx]), device=dev))
        self.steps = int(state[2])

    def step(self, f, fluxes, rows):
        """Add the step's fluxes and precipitation to the accumulators; at an
        output step (rows: the output block's budget rows) also close the
        interval, and the next step begins a new one."""
        self.steps += 1
        span_s = self.steps * self.dt
        if rows is not None:
            self.steps = 0

        def hook(st, rng):
            self.engine.accumulate(fluxes, f, self.acc, self.dt, stream=st, cols=rng)
            if rows is not None:
                self.engine.water_storage(self.cs, self.stor_end, stream=st, cols=rng)
                self.engine.accum_finish(self.acc, self.stor_end, self.stor_beg, rows, span_s,
                                         stream=st, cols=rng)
        return hook


class Extremes:
    """An output interval's extremes (extremes.py), on the device: the running
    maxima and minima `val` of the selected series, `when` (the step of the
    interval that set each) and `k`, the steps taken so far.  Only a series of
    the output fluxes makes every step write them (`need_diag`)."""
    npz, nc = ("ext_val", "ext_when", "ext_steps", "ext_spec"), ("extremes", ncio.read_extremes)

    def __init__(self, engine, cs, series, dt: float):
        self.engine, self.cs, self.dt, self.series = engine, cs, dt, list(series)
        self.spec = X.spec_string(self.series)
        self.kind_rows, self.stats = X.pairs(self.series), X.masks(self.series)
        self.names = X.row_names(self.series)
        self.needs_fluxes = self.need_diag = X.has_diag(self.series)
        self.need_state = any(s.kind == L.EXT_SRC_STATE for s in self.series)
        self.need_forcing = any(s.kind == L.EXT_SRC_FORCING for s in self.series)
        n, dev, dtype = cs.ncol, cs.state.device, cs.state.dtype
        self.val = torch.zeros((2 * len(self.series), n), dtype=dtype, device=dev)
        self.when = torch.zeros((2 * len(self.series), n), dtype=torch.int32, device=dev)
        self.k = 0

    def state(self):
        """(val, when, k, spec) of the interval so far, on the host: what a restart carries."""
        return self.val.cpu().numpy(), self.when.cpu().numpy(), self.k, self.spec

    def restore(self, state, idx=slice(None)):
        """`state` (state(), of the columns `idx` picks) resumes its interval
        if it was taken with this run's spec; None, or another spec, starts a
        fresh one: the next step is the interval's first and takes any value."""
        self.k = 0
        if state is None or str(state[3]) != self.spec:
            return
        dev = self.val.device
        dt = np.float32 if self.val.dtype == torch.float32 else np.float64
        self.val.copy_(torch.as_tensor(np.ascontiguousarray(state[0][:, idx], dt), device=dev))
        self.when.copy_(torch.as_tensor(np.ascontiguousarray(state[1][:, idx], np.int32),
                                        device=dev))
        self.k = int(state[2])

    def step(self, f, fluxes, rows):
        """Fold this step into the running extremes from its fluxes (None
        without a flux series), its forcing `f` and the state it left; at an
        output step (rows: the output block's extremes rows) also form the
        interval's rows, and the next step begins a new interval."""
        self.k += 1
        k = self.k
        if rows is not None:
            self.k = 0
        state = self.cs.state if self.need_state else None
        forcing = f if self.need_forcing else None

        def hook(st, rng):
            self.engine.extremes_update(self.kind_rows, k, self.val, self.when, fluxes, forcing,
                                        state, stream=st, cols=rng)
            if rows is not None:
                self.engine.extremes_output(self.stats, self.dt, self.val, self.when, rows,
                                            stream=st, cols=rng)
        return hook


class IntervalStats:
    """An output interval's statistics (intstats.py), on the device: the running
    sums `acc` of the selected items, their counters `cnt` (the steps a
    condition held, its current and its longest run) and `k`, the steps taken
    so far.  Only an item of the output fluxes makes every step write them."""
    npz, nc = ("ist_acc", "ist_cnt", "ist_steps", "ist_spec"), ("intstats", ncio.read_intstats)

    def __init__(self, engine, cs, items, dt: float):
        self.engine, self.cs, self.dt, self.items = engine, cs, dt, list(items)
        self.spec = IS.spec_string(self.items)
        self.table, self.thresholds = IS.table(self.items), IS.thresholds(self.items)
        self.names = IS.row_names(self.items)
        self.needs_fluxes = IS.has_diag(self.items)
        self.need_state = any(it.kind == L.EXT_SRC_STATE for it in self.items)
        self.need_forcing = any(it.kind == L.EXT_SRC_FORCING for it in self.items)
        n, dev = cs.ncol, cs.state.device
        self.acc = torch.zeros((len(self.items), n), dtype=torch.float64, device=dev)
        self.cnt = torch.zeros((3 * len(self.items), n), dtype=torch.int32, device=dev)
        self.k = 0

    def state(self):
        """(acc, cnt, k, spec) of the interval so far, on the host: what a restart carries."""
        return self.acc.cpu().numpy(), self.cnt.cpu().numpy(), self.k, self.spec

    def restore(self, state, idx=slice(None)):
        """`state` (state(), of the columns `idx` picks) resumes its interval
        if it was taken with this run's spec; None, or another spec, starts a
        fresh one: the next step is the interval's first and reads no old sum."""
        self.k = 0
        if state is None or str(state[3]) != self.spec:
            return
        dev = self.acc.device
        self.acc.copy_(torch.as_tensor(np.ascontiguousarray(state[0][:, idx], np.float64),
                                       device=dev))
        self.cnt.copy_(torch.as_tensor(np.ascontiguousarray(state[1][:, idx], np.int32),
                                       device=dev))
        self.k = int(state[2])

    def step(self, f, fluxes, rows):
        """Fold this step into the running sums and counters from its fluxes
        (None without a flux item), its forcing `f` and the state it left; at
        an output step (rows: the output block's statistics rows) also form
        the interval's rows, and the next step begins a new interval."""
        self.k += 1
        k = self.k
        if rows is not None:
            self.k = 0
        state = self.cs.state if self.need_state else None
        forcing = f if self.need_forcing else None

        def hook(st, rng):
            self.engine.intstats_update(self.table, self.thresholds, k, self.acc, self.cnt, fluxes,
                                        forcing, state, stream=st, cols=rng)
            if rows is not None:
                self.engine.intstats_output(self.table, k, self.dt, self.acc, self.cnt, rows,
                                            stream=st, cols=rng)
        return hook


class StateRows:
    """The selected groups of the land state (layout.STATE_OUT), formed at
    output steps from the state the step left (nmp_state_output), the groups
    that can hold the fill value last: `nofill_rows` come before them."""
    needs_fluxes = False

    def __init__(self, engine, cs, mask: int):
        self.engine, self.cs, self.mask = engine, cs, mask
        self.names, self.nofill_rows = stateout.row_names(mask), stateout.nofill_rows(mask)

    def step(self, f, fluxes, rows):
        if rows is None:
            return None

        def hook(st, rng):
            self.engine.state_output(self.cs, self.mask, rows, float(ncio.FILL), stream=st,
                                     cols=rng)
        return hook


class OutputBlock:
    """A run's producers in row order (fluxes, budget rows, extremes rows,
    interval-statistics rows, state rows) and what each step owes them.  `diag` is the (rows, ncol) block,
    `region_rows` the leading rows the regions reduce (None = all; state output
    ends them before the groups that can hold the fill value), `scratch` the one
    block the steps between output steps write their fluxes to (None unless a
    producer reads them), `carried` the producers a restart carries."""

    def __init__(self, engine, cs, dt: float, accumulate: bool, ext_series, state_mask: int,
                 stat_items=None):
        self.accum = Accumulation(engine, cs, dt) if accumulate else None
        self.extremes = Extremes(engine, cs, ext_series, dt) if ext_series is not None else None
        self.intstats = IntervalStats(engine, cs, stat_items, dt) if stat_items is not None \
            else None
        state = StateRows(engine, cs, state_mask) if state_mask else None
        self.producers = [p for p in (Fluxes(), self.accum, self.extremes, self.intstats, state)
                          if p is not None]
        self.carried = [p for p in (self.accum, self.extremes, self.intstats) if p is not None]
        self.names, self.slices = [], []
        for p in self.producers:
            self.slices.append(slice(len(self.names), len(self.names) + len(p.names)))
            self.names += p.names
        if self.intstats is not None and len(set(self.names)) != len(self.names):
            twice = sorted({n for n in self.names if self.names.count(n) > 1})
            raise ValueError(f"interval_stats: the row names {twice} occur twice in this run's "
                             "output (choose another label)")
        self.region_rows = None if state is None else self.slices[-1].start + state.nofill_rows
        n, dev, dtype = cs.ncol, cs.state.device, cs.state.dtype
        self.diag = torch.zeros((len(self.names), n), dtype=dtype, device=dev)
        self.scratch = torch.zeros((L.NDIAG_OUT, n), dtype=dtype, device=dev) \
            if any(p.needs_fluxes for p in self.producers) else None

    def plan(self, f, diag, out: bool):
        """One more step with the forcing `f`: (where it writes its fluxes, its
        diag_level, StreamShards.step's `post`).  An output step (`out`) writes
        them into rows 0..15 of `diag` (the block, or a process group's gather
        buffer), another into the scratch block, or nowhere (DIAG_NONE)."""
        fluxes, level = None, L.DIAG_NONE
        if out:
            fluxes, level = diag[:L.NDIAG_OUT], L.DIAG_OUT_LEVEL
        elif self.scratch is not None:
            fluxes, level = self.scratch, L.DIAG_OUT_LEVEL
        return fluxes, level, chain(
            p.step(f, fluxes if p.needs_fluxes else None, diag[s] if out else None)
            for p, s in zip(self.producers, self.slices))
