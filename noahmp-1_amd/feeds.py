"""Forcing feeds: how each step's 12 forcing fields reach the engine.

`ForcingUpload` carries host arrays to the GPU: pinned, double-buffered host
buffers copied on a copy stream, so the host builds step t+1's forcing while
the GPU steps t.  A feed is one forcing path of the offline driver
(driver.OfflineDriver); `feed_kind` chooses it from the provider and the
driver's arguments, and the driver's loop calls, every step,

* `read(t0)`: the input file's header (LDASIN files only), timed apart;
* `step(k, t0, cur) -> FeedStep(f, pre, after, upload, slot)`: the device
  buffer `f` the step reads, the work `pre(stream, (lo, hi))` that forms it
  on each range's stream, the streams and events the ranges wait for, and
  the `ForcingUpload` slot whose reuse the step's launches guard;
* `launched(t0, producers)`: after the step's launches are enqueued;

and `reset()` when the run's time jumps (a restart loaded into the driver).

From LDASIN files (cosz="device", ingest=True, the defaults) a file's bytes
go up as stored, once per input interval (ncio.LdasinForcing.grid_raw, read
ahead on a thread), and the engine forms the block in its column order
(nmp_ldasin_ingest) on the upload stream, beside the steps of the previous
file; the block stays resident while each range forms the 12 forcing fields,
COSZ included, on its own stream right before its launch
(nmp_forcing_from_ldasin_geo), waiting only on that block's event.  Files on
a coarser grid of their own (from_files forcing_grid) take the same path with
nmp_ldasin_regrid in nmp_ldasin_ingest's place, and downscale=True adds
nmp_ldasin_downscale on the upload stream before the block's event.
ingest=False builds the block on the host (ncio.LdasinForcing.block);
cosz="host" uploads the variables plus the host's COSZ every step
(ncio.LdasinForcing.raw, nmp_forcing_from_ldasin); the 12-field host form
(48 B per column, 96 in fp64) remains for providers that supply all of them,
and for the steps of an input file that carries CO2AIR / O2AIR of its own.
interp=True (LdasinInterpFeed) keeps the blocks of both ends of the input
interval resident and each range forms its fields between them
(nmp_forcing_from_ldasin_interp, tinterp.py) instead of holding the earlier
file's values.
"""
from __future__ import annotations

import datetime
from collections import namedtuple

import numpy as np
import torch

from . import cases, layout as L, timeman


class SyntheticForcing:
    """Seeded diurnal forcing for a ColumnSet (cases.forcing_step), per step."""

    def __init__(self, cols: cases.ColumnSet, seed: int = 0):
        self.cols, self.seed = cols, seed

    def __call__(self, step: int, t: datetime.datetime) -> np.ndarray:
        return cases.forcing_step(self.cols, timeman.julian(t), timeman.yearlen(t.year), step,
                                  seed=self.seed)


class ForcingUpload:
    """Pinned, double-buffered host->device forcing uploads on a copy stream.

    `put(f)` copies the (12, n) host array into pinned buffer b, enqueues its
    upload to device buffer b on the copy stream and returns that device
    buffer; the caller's launches wait on `stream`.  Buffer b is reused two
    puts later: the host side waits for b's previous upload to land, the copy
    stream for the launches that read it (`consumed_by`)."""

    def __init__(self, n: int, dtype, device, nbuf: int = 2, nfield: int = L.NFORCING):
        dev = torch.device(device)
        self.host = [torch.empty((nfield, n), dtype=dtype, pin_memory=True)
                     for _ in range(nbuf)]
        self.dev = [torch.empty((nfield, n), dtype=dtype, device=dev) for _ in range(nbuf)]
        self.stream = torch.cuda.Stream(dev)
        self.uploaded = [None] * nbuf
        self.consumed = [()] * nbuf
        self.count = 0

    def put(self, f: np.ndarray | None = None, fill=None, prefilled: bool = False) -> torch.Tensor:
        """Upload f, or whatever fill(host_array) writes into the pinned buffer
        (a provider filling it in place saves a host copy), or -- prefilled --
        what a completed prefetch() left there."""
        b = self.count % len(self.host)
        self.count += 1
        if prefilled:
            pass  # prefetch() waited for the buffer's previous upload and filled it
        else:
            if self.uploaded[b] is not None:
                self.uploaded[b].synchronize()  # pinned buffer b is free again
            if fill is not None:
                fill(self.host[b].numpy())
            else:
                self.host[b].numpy()[...] = f
        for e in self.consumed[b]:
            self.stream.wait_event(e)
        with torch.cuda.stream(self.stream):
            self.dev[b].copy_(self.host[b], non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(self.stream)
        self.uploaded[b], self.consumed[b] = ev, ()
        self._last = b
        return self.dev[b]

    def prefetch(self, fill, executor):
        """Fill the pinned buffer the next put() will use on `executor`, once
        its previous upload has landed; the caller then calls put(prefilled=
        True) after the returned future has completed without error."""
        b = self.count % len(self.host)
        ev, h = self.uploaded[b], self.host[b].numpy()

        def job():
            if ev is not None:
                ev.synchronize()
            fill(h)
        return executor.submit(job)

    @property
    def last_slot(self) -> int:
        """The buffer slot of the last put (its device buffer and whatever the
        caller keeps per slot are guarded by the same events)."""
        return self._last

    def consumed_by(self, streams, slot: int | None = None):
        """The last put's device buffer (or slot `slot`'s) is read by launches
        on `streams`."""
        evs = []
        for s in streams:
            e = torch.cuda.Event()
            e.record(s)
            evs.append(e)
        self.consumed[self._last if slot is None else slot] = tuple(evs)


class DeviceSyntheticForcing:
    """Synthetic forcing generated on the device each step (nmp_forcing_synth):
    no host generation, no upload -- the long-run path for synthetic cases
    (a year of hourly forcing for 1 M columns would be 0.4-0.8 TB from the
    host).  climate: (NCLIM, n) records of this rank's columns
    (cases.climate); first_col: their global index (stateless draws)."""
    on_device = True

    def __init__(self, climate: np.ndarray, seed: int = 0, first_col: int = 0):
        self.climate, self.seed, self.first_col = climate, seed, first_col


# ---- feeds --------------------------------------------------------------------------
def feed_kind(forcing, ldasin_upload: bool = True, cosz: str = "device", ingest: bool = True,
              downscale: bool = False, interp: bool = False) -> str:
    """The forcing path of a run, from the driver's `forcing` argument (a
    provider, "device" or None) and its arguments: "host" (12 fields from the
    host), "device-synth", "ldasin-step" (the LDASIN block with the host's
    COSZ every step), or a resident block per input file, built on the host
    ("ldasin-block") or from the file's bytes on the device ("ldasin-ingest";
    "ldasin-regrid" for files on a grid of their own).  interp: the steps
    between two input times interpolate between their resident blocks
    ("ldasin-interp" wherever one of the three block kinds would have been
    returned; any other path is refused).  The one place that asks the
    provider what it can do; no device work."""
    if cosz not in ("device", "host"):
        raise ValueError(f"cosz must be 'device' or 'host', not {cosz!r}")
    files = ldasin_upload and hasattr(forcing, "raw")
    if interp and not (files and cosz == "device"):
        raise ValueError("interp needs LDASIN files uploaded as resident blocks with COSZ formed "
                         "on the device (a file provider, ldasin_upload=True, cosz='device')")
    if downscale:
        if not (files and cosz == "device"):
            raise ValueError("downscale needs LDASIN files uploaded as resident blocks "
                             "(ldasin_upload=True, cosz='device')")
        if not hasattr(forcing, "dz"):
            raise ValueError("downscale needs LDASIN files on a forcing grid")
    if (isinstance(forcing, str) and forcing == "device") or getattr(forcing, "on_device", False):
        return "device-synth"
    if not files:
        return "host"
    if cosz == "host":
        return "ldasin-step"
    if interp:
        return "ldasin-interp"
    if not (ingest and hasattr(forcing, "grid_raw")):
        return "ldasin-block"
    return "ldasin-ingest" if getattr(forcing, "plan", None) is None else "ldasin-regrid"


FeedStep = namedtuple("FeedStep", "f pre after upload slot")


class _Feed:
    """What the driver reads of every feed; `last` is the last step's FeedStep."""
    raw_upload = raw_fbuf = geo = ingest = point = regrid_plan = dz = None
    last = None

    def read(self, t0):
        return None

    def launched(self, t0, producers):
        if self.last.upload is not None:
            self.last.upload.consumed_by(producers, self.last.slot)

    def reset(self):
        pass


class HostFeed(_Feed):
    """12 fields from the host through `upload`: the provider's array, or --
    a provider with `variables` (LDASIN files) -- the fields built in place in
    the pinned buffer.  Every run has one: the LDASIN feeds hand it the steps
    of a file that carries CO2AIR / O2AIR."""
    kind = "host"

    def __init__(self, forcing, ncol: int, dtype, dev, downscale: bool = False):
        self.forcing, self.downscale = forcing, downscale
        self.variables = getattr(forcing, "variables", None)
        self.upload = ForcingUpload(ncol, dtype, dev)
        self.info = None

    def read(self, t0):
        """The input file's variable names (header only, once per input time)."""
        if self.variables is not None:
            self.info = self.variables(t0)
        return self.info

    def step(self, k, t0, cur):
        if self.info is None:
            f = self.upload.put(self.forcing(k, t0))
        else:  # LDASIN files, the 12-field form
            if self.downscale:
                raise ValueError(f"downscale: the input file of {t0.isoformat()} carries its "
                                 "own CO2AIR / O2AIR and takes the 12-field host form")
            f = self.upload.put(fill=lambda h: self.forcing(k, t0, out=h))
        self.last = FeedStep(f, None, (cur, self.upload.stream), self.upload, None)
        return self.last


class DeviceSynthFeed(_Feed):
    """nmp_forcing_synth on each range's stream right before that range's
    launch, into buffer k % 2 (stream order: reuse safe); no upload."""
    kind = "device-synth"

    def __init__(self, forcing, engine, ncol: int, dtype, dev):
        self.forcing, self.engine = forcing, engine
        self.climate = torch.as_tensor(forcing.climate, device=dev).to(dtype).contiguous()
        self.fbuf = torch.empty((2, L.NFORCING, ncol), dtype=dtype, device=dev)

    def step(self, k, t0, cur):
        f, fr = self.fbuf[k % 2], self.forcing
        jul, yl = timeman.julian(t0), timeman.yearlen(t0.year)
        pre = lambda st, rng: self.engine.forcing_synth(  # noqa: E731
            self.climate, jul, yl, fr.seed, k, f, fr.first_col, stream=st, cols=rng)
        self.last = FeedStep(f, pre, (cur,), None, None)
        return self.last


class LdasinStepFeed(_Feed):
    """cosz="host": the LDASIN block (the file's variables and the host's
    COSZ) straight into a pinned buffer and up every step; each range forms
    its 12 fields on its own stream before its launch (nmp_forcing_from_ldasin)
    into buffer k % 2."""
    kind = "ldasin-step"

    def __init__(self, host: HostFeed, engine, ncol: int, dtype, dev):
        self.host, self.forcing, self.engine = host, host.forcing, engine
        self.raw_upload = ForcingUpload(ncol, torch.float32, dev, nfield=L.NLDASIN)
        self.raw_fbuf = torch.empty((2, L.NFORCING, ncol), dtype=dtype, device=dev)

    def read(self, t0):
        self.info = self.host.read(t0)
        return self.info

    def step(self, k, t0, cur):
        if {"CO2AIR", "O2AIR"} & self.info:
            self.last = self.host.step(k, t0, cur)
            return self.last
        raw, ready, upload, slot = self._block(k, t0)
        geo = solar = None
        if self.geo is not None and "COSZ" not in self.info:
            geo = self.geo
            solar = timeman.solar_terms(timeman.julian(t0), timeman.yearlen(t0.year))
        f = self.raw_fbuf[k % 2]
        pre = lambda st, rng: self.engine.forcing_from_ldasin(  # noqa: E731
            raw, f, stream=st, cols=rng, geo=geo, solar=solar)
        self.last = FeedStep(f, pre, (cur, ready), upload, slot)
        return self.last

    def _block(self, k, t0):
        """The step's device block, what the ranges wait for before they
        read it, and the ForcingUpload and slot that hold it."""
        up = self.raw_upload
        raw = up.put(fill=lambda h: self.forcing.raw(k, t0, out=h))
        return raw, up.stream, up, None


class LdasinBlockFeed(LdasinStepFeed):
    """cosz="device": the file's variables go up once per input interval and
    stay resident (`blocks`, by input time); COSZ is formed on the device
    every step from `geo` and the step's solar terms -- the file's own COSZ
    where it has one.  The ranges wait only for their own block's event, so
    the next file's upload (enqueued as soon as its bytes are read) runs
    beside the steps instead of before one.  kind "ldasin-block" builds the
    block on the host, "ldasin-ingest" / "ldasin-regrid" from the file's
    bytes on the device, with the next file read ahead."""

    def __init__(self, kind: str, host: HostFeed, engine, ncol: int, dtype, dev,
                 lapse_rate: float = 0.0065, dz_host=None):
        super().__init__(host, engine, ncol, dtype, dev)
        self.kind, self.blocks, self.lapse_rate = kind, {}, lapse_rate
        if dz_host is not None:  # downscale
            self.dz = torch.as_tensor(dz_host, device=dev).contiguous()
        self._prefetch, self._prefetch_pool = None, None
        self.geo = torch.as_tensor(self.forcing.geo(), device=dev).contiguous()
        if kind == "ldasin-block":
            return
        # (files on their own grid: the source grid's points, and the
        # columns' regrid plan instead of a point each)
        fr, regrid = self.forcing, kind == "ldasin-regrid"
        npts = fr.plan.npts if regrid else fr.grid.shape[0] * fr.grid.shape[1]
        self.ingest = ForcingUpload(npts, torch.int32, dev, nfield=L.NLDASIN - 1)
        self.ingest_blk = torch.zeros((2, L.NLDASIN, ncol), dtype=torch.float32, device=dev)
        if regrid:
            self.regrid_plan = fr.plan.to(dev)
        else:
            self.point = torch.as_tensor(fr.point(), device=dev)

    def _block(self, k, t0):
        ti = self.forcing.input_time(t0)
        if ti not in self.blocks:
            self.blocks[ti] = self._put_block(t0, "COSZ" in self.info)
        for old in [b for b in self.blocks if b < ti]:
            del self.blocks[old]
        return self.blocks[ti]

    def launched(self, t0, producers):
        super().launched(t0, producers)
        if self.ingest is not None:
            self._put_next_block(t0)

    def reset(self):
        """The resident blocks and the read-ahead belong to the old time: a
        block kept across a jump could sit in a slot the next upload reuses."""
        self.blocks.clear()
        if self._prefetch is not None:
            self._prefetch[1].exception()  # a running read-ahead finishes with its buffer
        self._prefetch = None

    def _put_block(self, t: datetime.datetime, file_cosz: bool):
        """Upload the LDASIN block of t's input file once; returns the device
        block, its event and the ForcingUpload whose stream and slot guard it.
        With `ingest` (and no COSZ in the file) the file's bytes go up as
        stored and the engine forms the block's rows (nmp_ldasin_ingest, or
        nmp_ldasin_regrid for files on their own grid, on the upload's
        stream); otherwise the host builds the block (ncio block).  With
        downscale either block is then corrected for elevation on the same
        stream (nmp_ldasin_downscale), before its event."""
        fr = self.forcing
        if self.ingest is None or file_cosz or not fr.ingestible(t):
            up = self.raw_upload
            blk = up.put(fill=lambda h: fr.block(t, out=h))
        else:
            up, ti = self.ingest, fr.input_time(t)
            ready = False
            if self._prefetch is not None and self._prefetch[0] == ti:
                # the file's bytes were read while the previous file's steps ran
                ready = self._prefetch[1].exception() is None
            self._prefetch = None
            g = up.put(fill=lambda h: fr.grid_raw(t, out=h), prefilled=ready)
            blk = self.ingest_blk[up.last_slot]
            if self.regrid_plan is not None:
                self.engine.ldasin_regrid(g, self.regrid_plan, blk, fr.nearest_mask,
                                          stream=up.stream)
            else:
                self.engine.ldasin_ingest(g, self.point, blk, stream=up.stream)
        if self.dz is not None:
            self.engine.ldasin_downscale(blk, self.dz, self.lapse_rate, stream=up.stream)
        if up is self.ingest:
            # read the next input file's bytes ahead (a missing or non-fp32 file
            # fails only the prefetch; its step then takes the plain path)
            nxt = ti + fr.every
            if self._prefetch_pool is None:
                from concurrent.futures import ThreadPoolExecutor
                self._prefetch_pool = ThreadPoolExecutor(1)
            self._prefetch = (nxt, up.prefetch(lambda h: fr.grid_raw(nxt, out=h),
                                               self._prefetch_pool))
        ev = torch.cuda.Event()
        ev.record(up.stream)
        return blk, ev, up, up.last_slot

    def _put_next_block(self, t: datetime.datetime):
        """Once the next input file's bytes have been read ahead, upload and
        ingest them (on the upload stream, beside the steps of this
        interval) -- when that file takes the ingest path.  Only the interval
        right after t's: the one after that would take the slot this
        interval's remaining steps still read (two slots)."""
        pf, fr = self._prefetch, self.forcing
        if pf is None or pf[0] in self.blocks or not pf[1].done() or \
                pf[0] != fr.input_time(t) + fr.every:
            return
        nxt = pf[0]
        if pf[1].exception() is not None:
            return  # the boundary step reads it itself (and raises if it must)
        if {"CO2AIR", "O2AIR", "COSZ"} & fr.variables(nxt) or not fr.ingestible(nxt):
            return
        self.blocks[nxt] = self._put_block(nxt, False)


class LdasinInterpFeed(_Feed):
    """Interpolation between input times (tinterp.py; nmp_forcing_from_ldasin_interp):
    the steps of the input interval [ti, ti + every) read the resident blocks
    of both its ends.  A block is formed per file exactly as LdasinBlockFeed
    forms it, on the upload stream -- ingest or regrid from the file's bytes
    (or the host's block, ingest=False), nmp_ldasin_downscale if asked, then
    nmp_ldasin_cosz (COSZ at the file's own time, for the zenith-weighted
    SWDOWN), then the block's event -- and each range forms its 12 fields on
    its own stream before its launch, waiting on both blocks' events.

    Three slots: the interval's two blocks are in use while the block after
    them is read ahead (a thread fills the pinned slot; `launched` uploads it
    once the bytes are there).  A device slot is overwritten only after the
    events of the launches that read it, a pinned slot only after its upload's
    (ForcingUpload); a read-ahead that is not used is waited for before its
    slot is filled again.  prefetch=False forms every block at the step that
    first needs it instead.

    The interval whose closing file does not exist runs held (w1 = 0) when it
    ends at or after the run's end (`end`), noted in `interp_held`; a missing
    file anywhere else is a FileNotFoundError at the step that needs it."""
    kind = "ldasin-interp"
    NSLOT = 3

    def __init__(self, host: HostFeed, engine, ncol: int, dtype, dev, lapse_rate: float = 0.0065,
                 dz_host=None, ingest: bool = True, hold=("RAINRATE",), sw_zenith: bool = True,
                 cosz_floor: float = 0.05, end: datetime.datetime | None = None,
                 prefetch: bool = True):
        from . import tinterp
        self.host, self.forcing, self.engine = host, host.forcing, engine
        self.hold_mask = tinterp.hold_mask(hold)
        self.sw_zenith, self.cosz_floor = bool(sw_zenith), float(cosz_floor)
        tinterp.check_args(0.0, self.hold_mask, self.sw_zenith, self.cosz_floor)
        self.end, self.prefetch, self.lapse_rate = end, bool(prefetch), lapse_rate
        self.blocks, self.interp_held = {}, []
        self.read_ahead = 0  # blocks formed beside the steps, ahead of the one that needs them
        self._prefetch, self._prefetch_pool = None, None
        fr = self.forcing
        if dz_host is not None:  # downscale
            self.dz = torch.as_tensor(dz_host, device=dev).contiguous()
        self.geo = torch.as_tensor(fr.geo(), device=dev).contiguous()
        self.fbuf = torch.empty((2, L.NFORCING, ncol), dtype=dtype, device=dev)
        if ingest and hasattr(fr, "grid_raw"):
            regrid = getattr(fr, "plan", None) is not None
            npts = fr.plan.npts if regrid else fr.grid.shape[0] * fr.grid.shape[1]
            self.ingest = ForcingUpload(npts, torch.int32, dev, nbuf=self.NSLOT,
                                        nfield=L.NLDASIN - 1)
            self.ingest_blk = torch.zeros((self.NSLOT, L.NLDASIN, ncol), dtype=torch.float32,
                                          device=dev)
            if regrid:
                self.regrid_plan = fr.plan.to(dev)
            else:
                self.point = torch.as_tensor(fr.point(), device=dev)
            self.up = self.ingest
        else:  # the host builds each block; the upload's device buffers are the slots
            self.raw_upload = ForcingUpload(ncol, torch.float32, dev, nbuf=self.NSLOT,
                                            nfield=L.NLDASIN)
            self.up = self.raw_upload

    # ---- files ---------------------------------------------------------------------
    def _path(self, ti):
        from .ncio import ldasin_path
        return ldasin_path(self.forcing.indir, ti)

    def _check_file(self, ti):
        """The input file of ti can become a resident block (FileNotFoundError
        naming it when it does not exist)."""
        fr = self.forcing
        own = {"COSZ", "CO2AIR", "O2AIR"} & fr.variables(ti)
        if own:
            raise ValueError(f"interp: {self._path(ti)} carries {', '.join(sorted(own))} of its "
                             "own; interpolation between input times takes files with the 8 "
                             "LDASIN variables only")
        if not fr.ingestible(ti):
            raise ValueError(f"interp: {self._path(ti)} does not hold the 8 LDASIN variables as "
                             "fp32 grids of the forcing's shape; interpolation needs resident "
                             "blocks")

    def read(self, t0):
        """The headers of the interval's files (cached per input time)."""
        import os
        fr = self.forcing
        ti = fr.input_time(t0)
        self._check_file(ti)
        if t0 != ti and os.path.isfile(self._path(ti + fr.every)):
            self._check_file(ti + fr.every)
        return None

    # ---- blocks --------------------------------------------------------------------
    def _drop_prefetch(self):
        """A read-ahead nobody takes finishes before its pinned slot is filled again."""
        if self._prefetch is not None:
            self._prefetch[1].exception()
        self._prefetch = None

    def _put_block(self, ti):
        """Upload and form the block of input time ti in the next slot; returns
        (device block, its event, its slot)."""
        fr, up = self.forcing, self.up
        self._check_file(ti)
        if self.ingest is not None:
            ready = False
            if self._prefetch is not None and self._prefetch[0] == ti:
                ready = self._prefetch[1].exception() is None
                self._prefetch = None
            else:
                self._drop_prefetch()
            g = up.put(fill=lambda h: fr.grid_raw(ti, out=h), prefilled=ready)
            blk = self.ingest_blk[up.last_slot]
            if self.regrid_plan is not None:
                self.engine.ldasin_regrid(g, self.regrid_plan, blk, fr.nearest_mask,
                                          stream=up.stream)
            else:
                self.engine.ldasin_ingest(g, self.point, blk, stream=up.stream)
        else:
            blk = up.put(fill=lambda h: fr.block(ti, out=h))
        if self.dz is not None:
            self.engine.ldasin_downscale(blk, self.dz, self.lapse_rate, stream=up.stream)
        solar = timeman.solar_terms(timeman.julian(ti), timeman.yearlen(ti.year))
        self.engine.ldasin_cosz(blk, self.geo, solar, stream=up.stream)
        ev = torch.cuda.Event()
        ev.record(up.stream)
        return blk, ev, up.last_slot

    def _block(self, ti):
        if ti not in self.blocks:
            self.blocks[ti] = self._put_block(ti)
        return self.blocks[ti]

    def step(self, k, t0, cur):
        import os
        from . import tinterp
        fr = self.forcing
        ti = fr.input_time(t0)
        tn = ti + fr.every
        for old in [b for b in self.blocks if b < ti]:
            del self.blocks[old]
        w1 = tinterp.weights(t0, ti, fr.every)[1]
        b0, e0, s0 = self._block(ti)
        b1, e1, s1 = None, None, None
        if w1 != 0.0 and tn not in self.blocks and not os.path.isfile(self._path(tn)):
            if self.end is None or tn < self.end:
                raise FileNotFoundError(self._path(tn))
            if ti not in self.interp_held:  # the closing interval runs held
                self.interp_held.append(ti)
            w1 = 0.0
        if w1 != 0.0:
            b1, e1, s1 = self._block(tn)
        solar = timeman.solar_terms(timeman.julian(t0), timeman.yearlen(t0.year))
        f = self.fbuf[k % 2]
        pre = lambda st, rng: self.engine.forcing_from_ldasin_interp(  # noqa: E731
            b0, b1, w1, f, self.geo, solar, self.hold_mask, self.sw_zenith, self.cosz_floor,
            stream=st, cols=rng)
        self._slots = (s0,) if s1 is None else (s0, s1)
        self.last = FeedStep(f, pre, (cur, e0) if e1 is None else (cur, e0, e1), None, None)
        return self.last

    def launched(self, t0, producers):
        """The step's launches read its blocks' slots; then the read-ahead."""
        evs = []
        for s in producers:
            e = torch.cuda.Event()
            e.record(s)
            evs.append(e)
        for slot in self._slots:
            self.up.consumed[slot] = tuple(evs)
        if self.prefetch:
            self._read_ahead(t0)

    def _read_ahead(self, t0):
        """The first block after t0's that is not resident yet, among this
        interval's closing block and the one after it (the third slot): start
        reading its bytes, or -- once they are there -- upload and form it
        beside the steps.  A file that is missing or cannot become a block is
        left to the step that needs it."""
        import os
        fr = self.forcing
        tn = fr.input_time(t0) + fr.every
        nxt = tn if tn not in self.blocks else tn + fr.every
        if nxt in self.blocks:
            return
        if self.ingest is None:
            try:
                if os.path.isfile(self._path(nxt)):
                    self.blocks[nxt] = self._put_block(nxt)
                    self.read_ahead += 1
            except ValueError:
                pass
            return
        pf = self._prefetch
        if pf is None:
            if os.path.isfile(self._path(nxt)):
                try:
                    self._check_file(nxt)
                except ValueError:
                    return
                if self._prefetch_pool is None:
                    from concurrent.futures import ThreadPoolExecutor
                    self._prefetch_pool = ThreadPoolExecutor(1)
                self._prefetch = (nxt, self.up.prefetch(lambda h: fr.grid_raw(nxt, out=h),
                                                        self._prefetch_pool))
            return
        if not pf[1].done():
            return
        if pf[0] != nxt or pf[1].exception() is not None:
            self._prefetch = None  # (finished: its slot is free for the next read)
            return
        try:
            self.blocks[nxt] = self._put_block(nxt)
            self.read_ahead += 1
        except ValueError:
            self._prefetch = None  # (done: nothing to wait for)

    def reset(self):
        """The resident blocks and the read-ahead belong to the old time; the
        restart's interval rebuilds both its blocks (the weights depend on
        time alone)."""
        self.blocks.clear()
        self._drop_prefetch()


def make_feed(kind: str, host: HostFeed, engine, ncol: int, dtype, dev, lapse_rate: float = 0.0065,
              dz_host=None, interp: dict | None = None):
    """The feed of `kind` (feed_kind) around the run's HostFeed; interp: the
    LdasinInterpFeed's own arguments."""
    if kind == "host":
        return host
    if kind == "ldasin-interp":
        return LdasinInterpFeed(host, engine, ncol, dtype, dev, lapse_rate, dz_host,
                                **(interp or {}))
    if kind == "device-synth":
        return DeviceSynthFeed(host.forcing, engine, ncol, dtype, dev)
    if kind == "ldasin-step":
        return LdasinStepFeed(host, engine, ncol, dtype, dev)
    return LdasinBlockFeed(kind, host, engine, ncol, dtype, dev, lapse_rate, dz_host)
