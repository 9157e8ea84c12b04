"""Python front end of the HIP column engine (drop-in for core/module_noahmp_engine.f90).

`Engine` owns the engine handle (tables on the device + options); column data
are caller-owned torch tensors on the engine's GPU in field-major SoA layout
(see layout.py / include/noahmp_engine.h).  `ColumnState` bundles the arrays
of one column set.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass

import numpy as np
import torch

from . import layout as L
from . import lib as _lib
from .params import Params

MATH_REF, MATH_FAST = 0, 1
# nmp_set_launch_variant: occupancy instantiation of the step kernel
LAUNCH_VARIANTS = {"auto": 0, "small": 1, "full": 2}


def _ptr(t, off: int = 0):
    """Device pointer of t, `off` elements in (a column offset into a field-major array)."""
    return C.c_void_p(t.data_ptr() + off * t.element_size()) if t is not None else C.c_void_p(0)


@dataclass
class ColumnState:
    """Device-resident SoA arrays for ncol columns (leading dimension ncol)."""
    state: torch.Tensor     # (56, n) real
    isnow: torch.Tensor     # (n,) int32
    static_f: torch.Tensor  # (6, n) real
    static_i: torch.Tensor  # (6, n) int32
    status: torch.Tensor    # (n,) int32

    @property
    def ncol(self) -> int:
        return int(self.isnow.shape[0])

    @classmethod
    def from_host(cls, cols, device, dtype=torch.float32) -> "ColumnState":
        """From a cases.ColumnSet (numpy SoA)."""
        dev = torch.device(device)
        return cls(
            state=torch.as_tensor(np.ascontiguousarray(cols.state), device=dev).to(dtype).contiguous(),
            isnow=torch.as_tensor(np.ascontiguousarray(cols.isnow, np.int32), device=dev),
            static_f=torch.as_tensor(np.ascontiguousarray(cols.static_f), device=dev).to(dtype).contiguous(),
            static_i=torch.as_tensor(np.ascontiguousarray(cols.static_i, np.int32), device=dev),
            status=torch.zeros(cols.isnow.shape[0], dtype=torch.int32, device=dev),
        )

    def narrow(self, start: int, length: int) -> "ColumnState":
        """A contiguous copy of a column range (for sharding)."""
        return ColumnState(self.state[:, start:start + length].contiguous(),
                           self.isnow[start:start + length].contiguous(),
                           self.static_f[:, start:start + length].contiguous(),
                           self.static_i[:, start:start + length].contiguous(),
                           self.status[start:start + length].contiguous())


class Engine:
    """One engine per device: noahmp_init + *_readptable + noahmp_set_options."""

    def __init__(self, params: Params | None = None, options: dict | None = None,
                 device: int = 0, precision: int = 4, math: int | str = MATH_REF):
        self._lib = _lib.load()
        self.params = params if params is not None else Params.builtin()
        opts = dict(L.CASE_NML_OPTIONS)
        if options:
            opts.update(options)
        self.options = opts
        self.device = int(device)
        self.precision = int(precision)
        self.dtype = torch.float32 if precision == 4 else torch.float64
        o = _lib.NmpOptions(*[int(opts[k]) for k in _lib.NMP_OPTION_FIELDS])
        h = C.c_void_p()
        _lib.check(self._lib.nmp_init(C.byref(self.params.struct), C.byref(o), self.device,
                                      self.precision, C.byref(h)), "nmp_init")
        self._h = h
        if isinstance(math, str):
            math = MATH_FAST if math == "fast" else MATH_REF
        self.set_math(math)

    def set_cols_per_wave(self, cpw: int):
        """nmp_set_cols_per_wave: 8..64 columns per wave, 0 = 64 (default)."""
        _lib.check(self._lib.nmp_set_cols_per_wave(self._h, int(cpw)), "nmp_set_cols_per_wave")

    def option_set(self, request: int = -1) -> int:
        """nmp_option_set: the compiled option set the kernel runs (0 = the
        run-time-options kernel); request 0 forces set 0, 1 picks the match."""
        rc = self._lib.nmp_option_set(self._h, int(request))
        _lib.check(min(rc, 0), "nmp_option_set")
        return rc

    def launch_variant(self, variant: str | int | None = None) -> str:
        """nmp_set_launch_variant: "small" / "full" force the half- / full-
        occupancy kernel for every launch, "auto" (default) picks by column
        count; None only queries.  Returns the variant in use."""
        v = -1 if variant is None else LAUNCH_VARIANTS.get(variant, variant)
        rc = self._lib.nmp_set_launch_variant(self._h, int(v))
        _lib.check(min(rc, 0), "nmp_set_launch_variant")
        return {i: k for k, i in LAUNCH_VARIANTS.items()}[rc]

    def set_math(self, mode: int):
        _lib.check(self._lib.nmp_set_math(self._h, int(mode)), "nmp_set_math")
        self.math = int(mode)

    def close(self):
        if getattr(self, "_h", None):
            self._lib.nmp_finalize(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------------
    def _check_block(self, t: torch.Tensor, shape: tuple, dtype, what: str):
        """A contiguous field-major block (or per-column vector) on the engine's
        device: the library is handed raw pointers offset by a column index."""
        assert tuple(t.shape) == shape and t.dtype == dtype, (what, tuple(t.shape), t.dtype)
        assert t.is_contiguous(), what
        assert t.device.type == "cuda" and t.device.index == self.device, (what, t.device)

    @staticmethod
    def _cols_range(n: int, cols) -> tuple[int, int]:
        lo, hi = (0, n) if cols is None else (int(cols[0]), int(cols[1]))
        assert 0 <= lo <= hi <= n
        return lo, hi

    def _call(self, name: str, stream, *args):
        """The library's entry `name`: the engine's handle, `args`, then
        `stream` (None: the device's current stream); its return code checked."""
        s = stream if stream is not None else torch.cuda.current_stream(self.device)
        _lib.check(getattr(self._lib, name)(self._h, *args, C.c_void_p(s.cuda_stream)), name)

    def _check_cols(self, cs: ColumnState, forcing: torch.Tensor):
        n = cs.ncol
        self._check_block(cs.state, (L.NSTATE, n), self.dtype, "state")
        self._check_block(cs.isnow, (n,), torch.int32, "isnow")
        self._check_block(cs.static_f, (L.NSTATIC_F, n), self.dtype, "static_f")
        self._check_block(cs.static_i, (L.NSTATIC_I, n), torch.int32, "static_i")
        self._check_block(cs.status, (n,), torch.int32, "status")
        # (leading axes are allowed, as ever: the pointer is the first slice's)
        self._check_block(forcing, tuple(forcing.shape[:-2]) + (L.NFORCING, n), self.dtype,
                          "forcing")

    def _check_words(self, t: torch.Tensor, rows: int, size: int, what: str):
        """(rows, npts) words of `size` bytes, whatever their dtype: a file's
        big-endian grids."""
        npts = int(t.shape[1]) if t.dim() == 2 else -1
        self._check_block(t, (rows, npts), t.dtype, what)
        assert t.element_size() == size, (what, t.dtype)

    def step(self, cs: ColumnState, forcing: torch.Tensor, zsoil, dt: float, julian: float,
             yearlen: int, diag: torch.Tensor | None = None, diag_level: int = L.DIAG_NONE,
             stream=None, cols: tuple[int, int] | None = None, order: torch.Tensor | None = None,
             cost: torch.Tensor | None = None):
        """One noahmp_sflx step for every column (enqueued on `stream`).

        cols=(lo, hi) steps only columns lo..hi-1, in place (pointer offsets with
        ld = cs.ncol; forcing and diag are indexed by the same columns), so
        column ranges can be stepped on different streams.

        order / cost (re-binning, nmp_step_binned): int32 / uint8 tensors of
        cs.ncol entries; the range's slice of `order` must hold a permutation of
        0..hi-lo-1 (indices relative to lo), `cost` receives each column's
        vege_flux trip count."""
        self._check_cols(cs, forcing)
        n = cs.ncol
        lo, hi = self._cols_range(n, cols)
        if diag_level != L.DIAG_NONE:
            nd = L.NDIAG_FULL if diag_level == L.DIAG_FULL_LEVEL else L.NDIAG_OUT
            assert diag is not None
            # raw pointers offset by `lo` with rows exactly n apart: a strided view
            # would be written in the wrong places
            self._check_block(diag, (nd, n), self.dtype, "diag")
        zs = (C.c_float * 4)(*[float(z) for z in zsoil])
        args = (hi - lo, n, zs, float(dt), float(julian), int(yearlen), _ptr(cs.state, lo),
                _ptr(cs.isnow, lo), _ptr(cs.static_f, lo), _ptr(cs.static_i, lo),
                _ptr(forcing, lo), _ptr(diag, lo), int(diag_level), _ptr(cs.status, lo))
        if order is not None or cost is not None:
            if order is not None:
                self._check_block(order, (n,), torch.int32, "order")
            if cost is not None:
                self._check_block(cost, (n,), torch.uint8, "cost")
            if order is not None and os.environ.get("NMP_CHECK_ORDER") == "1":
                s = stream if stream is not None else torch.cuda.current_stream(self.device)
                # nmp_step_binned trusts order to be a permutation (noahmp_engine.h);
                # the debug check costs a sort and a host sync per launch
                with torch.cuda.stream(s):
                    srt = torch.sort(order[lo:hi])[0]
                    ok = bool(torch.equal(srt, torch.arange(hi - lo, dtype=torch.int32,
                                                            device=order.device)))
                if not ok:
                    raise ValueError(f"order[{lo}:{hi}] is not a permutation of 0..{hi - lo - 1}")
            self._call("nmp_step_binned", stream, *args, _ptr(order, lo), _ptr(cost, lo))
            return
        self._call("nmp_step", stream, *args)

    def rebin(self, cost: torch.Tensor, order: torch.Tensor, tile: int, stream=None,
              cols: tuple[int, int] | None = None):
        """nmp_rebin: order[lo:hi] <- the columns lo..hi-1 sorted by cost within
        tiles of `tile` columns (indices relative to lo)."""
        n = int(cost.shape[0])
        lo, hi = self._cols_range(n, cols)
        self._check_block(cost, (n,), torch.uint8, "cost")
        self._check_block(order, (n,), torch.int32, "order")
        self._call("nmp_rebin", stream, hi - lo, _ptr(cost, lo), _ptr(order, lo), int(tile))

    def forcing_synth(self, climate: torch.Tensor, julian: float, yearlen: int, seed: int,
                      step: int, out: torch.Tensor, first_col: int = 0, stream=None,
                      cols: tuple[int, int] | None = None):
        """nmp_forcing_synth: one step of synthetic forcing, generated on the
        device from the (NCLIM, n) climate records into out (NFORCING, n);
        cols=(lo, hi) generates only those columns (first_col + lo is their
        global index, so ranges and ranks draw the same numbers as one launch)."""
        n = int(climate.shape[1])
        lo, hi = self._cols_range(n, cols)
        self._check_block(climate, (L.NCLIM, n), self.dtype, "climate")
        self._check_block(out, (L.NFORCING, n), self.dtype, "out")
        self._call("nmp_forcing_synth", stream, hi - lo, n, _ptr(climate, lo), float(julian),
                   int(yearlen), int(seed) & (2**64 - 1), int(step), int(first_col) + lo,
                   _ptr(out, lo))

    def forcing_from_ldasin(self, ldasin: torch.Tensor, out: torch.Tensor, stream=None,
                            cols: tuple[int, int] | None = None, geo: torch.Tensor | None = None,
                            solar: tuple[float, float, float] | None = None):
        """nmp_forcing_from_ldasin: the 12 forcing fields of one step into out
        (NFORCING, n), engine precision, from the (NLDASIN, n) fp32 LDASIN
        block (layout.LDASIN); SFCPRS, CO2AIR and O2AIR formed on the device
        from PSFC.  cols=(lo, hi) converts only those columns.

        geo, solar (nmp_forcing_from_ldasin_geo): COSZ formed on the device from
        geo = (3, n) float64 (sin lat, cos lat, lon; ncio.LdasinForcing.geo)
        and solar = timeman.solar_terms(julian, yearlen) instead of read from
        the block's COSZ row."""
        n = int(ldasin.shape[1])
        lo, hi = self._cols_range(n, cols)
        self._check_block(ldasin, (L.NLDASIN, n), torch.float32, "ldasin")
        self._check_block(out, (L.NFORCING, n), self.dtype, "out")
        if geo is None:
            self._call("nmp_forcing_from_ldasin", stream, hi - lo, n, _ptr(ldasin, lo),
                       _ptr(out, lo))
            return
        self._check_block(geo, (3, n), torch.float64, "geo")
        sd, cd, ha0 = (float(v) for v in solar)
        self._call("nmp_forcing_from_ldasin_geo", stream, hi - lo, n, _ptr(ldasin, lo),
                   _ptr(geo, lo), sd, cd, ha0, _ptr(out, lo))

    def ldasin_ingest(self, grid_be: torch.Tensor, point: torch.Tensor, out: torch.Tensor,
                      stream=None):
        """nmp_ldasin_ingest: rows T2D..LWDOWN of the (NLDASIN, n) fp32 block
        `out` from an LDASIN file's bytes: grid_be = (8, npts) 4-byte words,
        the file's big-endian fp32 grids in layout.LDASIN order; column c takes
        grid point point[c] (int32, (n,)).  The COSZ row is left as it is."""
        n = int(out.shape[1])
        self._check_words(grid_be, L.NLDASIN - 1, 4, "grid_be")
        self._check_block(point, (n,), torch.int32, "point")
        self._check_block(out, (L.NLDASIN, n), torch.float32, "out")
        self._call("nmp_ldasin_ingest", stream, n, n, int(grid_be.shape[1]), _ptr(grid_be),
                   _ptr(point), _ptr(out))

    def ldasin_regrid(self, grid_be: torch.Tensor, plan, out: torch.Tensor,
                      nearest_mask: int = 0, stream=None):
        """nmp_ldasin_regrid: rows T2D..LWDOWN of the (NLDASIN, n) fp32 block
        `out` from an LDASIN file stored on its own (coarse) grid: grid_be =
        (8, npts) 4-byte words, the file's big-endian fp32 grids in
        layout.LDASIN order; `plan` (regrid.RegridPlan on this device, built
        for n columns and npts source points) gives each column its four
        weighted source entries.  Bit v of nearest_mask: variable v takes its
        nearest entry (regrid.nearest_mask).  The COSZ row is left as it is."""
        n = int(out.shape[1])
        self._check_words(grid_be, L.NLDASIN - 1, 4, "grid_be")
        assert plan.dev is not None and plan.ncol == n, "plan.to(device) for this block"
        assert plan.npts == int(grid_be.shape[1]), (plan.npts, tuple(grid_be.shape))
        corner, weight = plan.dev["corner"], plan.dev["weight"]
        self._check_block(corner, (4, n), torch.int32, "corner")
        self._check_block(weight, (4, n), torch.float64, "weight")
        self._check_block(out, (L.NLDASIN, n), torch.float32, "out")
        assert 0 <= int(nearest_mask) < (1 << (L.NLDASIN - 1))
        self._call("nmp_ldasin_regrid", stream, n, n, plan.npts, _ptr(grid_be), _ptr(corner),
                   _ptr(weight), int(nearest_mask), _ptr(out))

    def ldasin_downscale(self, block: torch.Tensor, dz: torch.Tensor, lapse: float, stream=None):
        """nmp_ldasin_downscale: rows T2D, Q2D, PSFC and LWDOWN of the
        (NLDASIN, n) fp32 block corrected in place for the elevation
        difference dz (n,) fp32 (model minus source, m) with the lapse rate
        `lapse` (K/m); the other rows are untouched."""
        n = int(block.shape[1])
        self._check_block(block, (L.NLDASIN, n), torch.float32, "block")
        self._check_block(dz, (n,), torch.float32, "dz")
        self._call("nmp_ldasin_downscale", stream, n, n, _ptr(dz), float(lapse), _ptr(block))

    def ldasin_cosz(self, block: torch.Tensor, geo: torch.Tensor,
                    solar: tuple[float, float, float], stream=None,
                    cols: tuple[int, int] | None = None):
        """nmp_ldasin_cosz: row COSZ of the (NLDASIN, n) fp32 block := COSZ at
        the block's own input time, from geo (3, n) float64 and solar =
        timeman.solar_terms of that time; the other rows are untouched.
        cols=(lo, hi) writes only those columns."""
        n = int(block.shape[1])
        lo, hi = self._cols_range(n, cols)
        self._check_block(block, (L.NLDASIN, n), torch.float32, "block")
        self._check_block(geo, (3, n), torch.float64, "geo")
        sd, cd, ha0 = (float(v) for v in solar)
        self._call("nmp_ldasin_cosz", stream, hi - lo, n, _ptr(geo, lo), sd, cd, ha0,
                   _ptr(block, lo))

    def forcing_from_ldasin_interp(self, ldasin0: torch.Tensor, ldasin1: torch.Tensor | None,
                                   w1: float, out: torch.Tensor, geo: torch.Tensor,
                                   solar: tuple[float, float, float], hold_mask: int = 0,
                                   sw_zenith: bool = True, cosz_floor: float = 0.05, stream=None,
                                   cols: tuple[int, int] | None = None):
        """nmp_forcing_from_ldasin_interp: the 12 forcing fields of the step
        that starts a fraction w1 (0 <= w1 < 1) into an input interval, into
        out (NFORCING, n), engine precision, from the interval's two resident
        (NLDASIN, n) fp32 blocks (their COSZ rows written by ldasin_cosz);
        tinterp.interp_host is the numpy form.  geo, solar: the step's own, as
        in forcing_from_ldasin.  hold_mask: bit v = variable v keeps block 0's
        value (tinterp.hold_mask).  ldasin1 may be None when w1 == 0.
        cols=(lo, hi) forms only those columns."""
        n = int(ldasin0.shape[1])
        lo, hi = self._cols_range(n, cols)
        self._check_block(ldasin0, (L.NLDASIN, n), torch.float32, "ldasin0")
        if ldasin1 is not None:
            self._check_block(ldasin1, (L.NLDASIN, n), torch.float32, "ldasin1")
        self._check_block(out, (L.NFORCING, n), self.dtype, "out")
        self._check_block(geo, (3, n), torch.float64, "geo")
        sd, cd, ha0 = (float(v) for v in solar)
        self._call("nmp_forcing_from_ldasin_interp", stream, hi - lo, n, _ptr(ldasin0, lo),
                   _ptr(ldasin1, lo), float(w1), int(hold_mask), int(bool(sw_zenith)),
                   float(cosz_floor), _ptr(geo, lo), sd, cd, ha0, _ptr(out, lo))

    def ldasout_grid(self, diag: torch.Tensor, point: torch.Tensor, out: torch.Tensor,
                     fill: float, stream=None):
        """nmp_ldasout_grid: the (nfield, n) diagnostics `diag` (engine
        precision) onto out = (nfield, npts) words of the engine's size, the
        file's big-endian grids, `fill` off the columns' points (point: int32
        (n,))."""
        nf, n = int(diag.shape[0]), int(diag.shape[1])
        self._check_block(diag, (nf, n), self.dtype, "diag")
        self._check_block(point, (n,), torch.int32, "point")
        self._check_words(out, nf, self.precision, "out")
        self._call("nmp_ldasout_grid", stream, n, n, int(out.shape[1]), nf, _ptr(diag),
                   _ptr(point), float(fill), _ptr(out))

    # ---- accumulated output (nmp_accumulate / nmp_water_storage / nmp_accum_finish)
    def accumulate(self, diag: torch.Tensor, forcing: torch.Tensor, acc: torch.Tensor, dt: float,
                   stream=None, cols: tuple[int, int] | None = None):
        """nmp_accumulate: acc[f] += diag[f] * dt for the 16 output fluxes a
        step at DIAG_OUT_LEVEL wrote into `diag` (NDIAG_OUT, n) and acc[PRCP] +=
        forcing[PRCP] * dt from the step's (NFORCING, n) forcing; acc is
        (NACC, n) float64 for both precisions (layout.ACC).  cols=(lo, hi)
        accumulates only those columns, enqueued on `stream`."""
        n = int(acc.shape[1])
        lo, hi = self._cols_range(n, cols)
        self._check_block(diag, (L.NDIAG_OUT, n), self.dtype, "diag")
        self._check_block(forcing, (L.NFORCING, n), self.dtype, "forcing")
        self._check_block(acc, (L.NACC, n), torch.float64, "acc")
        self._call("nmp_accumulate", stream, hi - lo, n, float(dt), _ptr(diag, lo),
                   _ptr(forcing, lo), _ptr(acc, lo))

    def water_storage(self, cs: ColumnState, storage: torch.Tensor, stream=None,
                      cols: tuple[int, int] | None = None):
        """nmp_water_storage: storage[c] (n,) = the column's water storage in
        mm (canopy, snow, aquifer and soil water: the reference's BEG_WB /
        END_WB), 0 where IST != 1."""
        n = cs.ncol
        lo, hi = self._cols_range(n, cols)
        self._check_block(cs.state, (L.NSTATE, n), self.dtype, "state")
        self._check_block(cs.isnow, (n,), torch.int32, "isnow")
        self._check_block(cs.static_i, (L.NSTATIC_I, n), torch.int32, "static_i")
        self._check_block(storage, (n,), self.dtype, "storage")
        self._call("nmp_water_storage", stream, hi - lo, n, _ptr(cs.state, lo), _ptr(cs.isnow, lo),
                   _ptr(cs.static_i, lo), _ptr(storage, lo))

    def accum_finish(self, acc: torch.Tensor, stor_end: torch.Tensor, stor_beg: torch.Tensor,
                     out: torch.Tensor, span_s: float, stream=None,
                     cols: tuple[int, int] | None = None):
        """nmp_accum_finish: the interval's (NBUDGET, n) block `out`
        (layout.BUDGET: means over span_s seconds, totals, storage change
        stor_end - stor_beg and the water budget's residual) from acc (NACC, n)
        float64; then acc is zeroed and stor_beg takes stor_end, which starts
        the next interval."""
        n = int(acc.shape[1])
        lo, hi = self._cols_range(n, cols)
        self._check_block(acc, (L.NACC, n), torch.float64, "acc")
        self._check_block(stor_end, (n,), self.dtype, "stor_end")
        self._check_block(stor_beg, (n,), self.dtype, "stor_beg")
        self._check_block(out, (L.NBUDGET, n), self.dtype, "out")
        assert stor_end.data_ptr() != stor_beg.data_ptr() or n == 0
        self._call("nmp_accum_finish", stream, hi - lo, n, float(span_s), _ptr(acc, lo),
                   _ptr(stor_end, lo), _ptr(stor_beg, lo), _ptr(out, lo))

    # ---- state output (nmp_state_output) ---------------------------------------
    def state_output(self, cs: ColumnState, groups: int, out_rows: torch.Tensor, fill: float,
                     stream=None, cols: tuple[int, int] | None = None):
        """nmp_state_output: the rows of the state-output groups in the mask
        `groups` (stateout.parse_groups; layout.STATE_OUT) of every column into
        out_rows (len(stateout.rows(groups)), n), engine precision, `fill` on
        inactive snow layers; stateout.state_output_host is the numpy form.
        out_rows may be a block's trailing rows (a contiguous row slice).
        cols=(lo, hi) writes only those columns, enqueued on `stream`."""
        from . import stateout
        n = cs.ncol
        lo, hi = self._cols_range(n, cols)
        nrow = len(stateout.rows(groups))   # ValueError for an empty or out-of-range mask
        self._check_block(cs.state, (L.NSTATE, n), self.dtype, "state")
        self._check_block(cs.isnow, (n,), torch.int32, "isnow")
        self._check_block(cs.static_i, (L.NSTATIC_I, n), torch.int32, "static_i")
        self._check_block(out_rows, (nrow, n), self.dtype, "out_rows")
        self._call("nmp_state_output", stream, hi - lo, n, _ptr(cs.state, lo), _ptr(cs.isnow, lo),
                   _ptr(cs.static_i, lo), int(groups), float(fill), _ptr(out_rows, lo), n)

    # ---- spin-up drift (nmp_state_drift / nmp_drift_reduce) --------------------
    def state_drift(self, cs: ColumnState, snap: torch.Tensor, drift: torch.Tensor | None = None,
                    stream=None, cols: tuple[int, int] | None = None):
        """nmp_state_drift: with `drift` (NDRIFT, n), the drift rows
        (layout.DRIFT_GROUPS) of the state's tracked values against the
        snapshot `snap` (NTRACKED, n); then `snap` takes the new tracked
        values (layout.TRACKED).  drift=None only takes the snapshot.  Engine
        precision; spinup.tracked_host / drift_host are the numpy form.
        cols=(lo, hi) handles only those columns, enqueued on `stream`."""
        n = cs.ncol
        lo, hi = self._cols_range(n, cols)
        self._check_block(cs.state, (L.NSTATE, n), self.dtype, "state")
        self._check_block(cs.isnow, (n,), torch.int32, "isnow")
        self._check_block(cs.static_i, (L.NSTATIC_I, n), torch.int32, "static_i")
        self._check_block(snap, (L.NTRACKED, n), self.dtype, "snap")
        if drift is not None:
            self._check_block(drift, (L.NDRIFT, n), self.dtype, "drift")
        self._call("nmp_state_drift", stream, hi - lo, n, _ptr(cs.state, lo), _ptr(cs.isnow, lo),
                   _ptr(cs.static_i, lo), _ptr(snap, lo), n, _ptr(drift, lo), n)

    def drift_reduce(self, drift: torch.Tensor, tol, weight: torch.Tensor | None = None,
                     stream=None):
        """nmp_drift_reduce: per drift group the largest drift of the (NDRIFT,
        n) block `drift` (engine precision) and its column, the count of
        columns with !(d <= tol) and the weighted sum by the fixed tree
        (spinup.reduce_host is the numpy form); tol: 7 numbers; weight: (n,)
        float64 on the device or None (= 1), a column of weight 0 is skipped.
        Returns a spinup.DriftResult (`max`, `arg`, `mean`, `count`, `wsum`,
        `wtot`).  Enqueued on `stream`; the 29 result words are then copied to
        the host, which waits for them.  The scratch and the result buffers
        live with the engine, one set per column count, so calls of one size
        must be ordered by their streams."""
        from . import spinup
        n = int(drift.shape[1]) if drift.dim() == 2 else -1
        self._check_block(drift, (L.NDRIFT, n), self.dtype, "drift")
        if weight is not None:
            self._check_block(weight, (n,), torch.float64, "weight")
        tol = np.ascontiguousarray(tol, np.float64)
        assert tol.shape == (L.NDRIFT,), tol.shape
        buf = self._drift_bufs(n)
        s = stream if stream is not None else torch.cuda.current_stream(self.device)
        res, w = buf["res"], buf["words"]
        with torch.cuda.stream(s):
            buf["tol_host"].copy_(torch.from_numpy(tol))
            buf["tol"].copy_(buf["tol_host"], non_blocking=True)
            _lib.check(self._lib.nmp_drift_reduce(
                self._h, n, n, _ptr(drift), _ptr(weight), _ptr(buf["tol"]), _ptr(buf["partial"]),
                _ptr(w, 0), _ptr(w, L.NDRIFT), _ptr(w, 2 * L.NDRIFT), _ptr(w, 3 * L.NDRIFT),
                _ptr(w, 4 * L.NDRIFT), C.c_void_p(s.cuda_stream)), "nmp_drift_reduce")
            res.copy_(w, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(s)
        ev.synchronize()
        h = res.numpy().copy()
        g = L.NDRIFT
        return spinup.DriftResult(h[:g].view(np.float64), h[g:2 * g], h[2 * g:3 * g].view(np.float64),
                                  h[3 * g:4 * g], float(h[4 * g:].view(np.float64)[0]))

    def _drift_bufs(self, n: int) -> dict:
        """drift_reduce's buffers for n columns, allocated once per engine and
        column count: the pass-1 scratch, the tolerances, and the result words
        [max 7 | arg 7 | wsum 7 | count 7 | wtot] on the device and pinned."""
        bufs = self.__dict__.setdefault("_drift_buf", {})
        b = bufs.get(n)
        if b is None:
            dev = torch.device("cuda", self.device)
            nchunk = max(-(-n // L.DRIFT_CHUNK), 1)
            b = bufs[n] = dict(
                partial=torch.empty(L.DRIFT_SCRATCH * nchunk, dtype=torch.int64, device=dev),
                tol=torch.empty(L.NDRIFT, dtype=torch.float64, device=dev),
                tol_host=torch.empty(L.NDRIFT, dtype=torch.float64, pin_memory=True),
                words=torch.zeros(4 * L.NDRIFT + 1, dtype=torch.int64, device=dev),
                res=torch.empty(4 * L.NDRIFT + 1, dtype=torch.int64, pin_memory=True))
        return b

    # ---- vegetation fraction through the year (nmp_static_monthly) ---------------
    def static_monthly(self, table: torch.Tensor, m0: int, m1: int, w: float,
                       out_row: torch.Tensor, stream=None, cols: tuple[int, int] | None = None):
        """nmp_static_monthly: out_row[c] (n,), engine precision = the monthly
        climatology `table` (12, n) float32 between its rows m0 and m1 with the
        later one's weight w, 0 <= w < 1 (vegclim.month_weights gives the three
        for a date; vegclim.static_monthly_host is the numpy form).  out_row is
        e.g. cs.static_f[L.STATIC_F.index("SHDFAC")], a row of a field-major
        block.  cols=(lo, hi) writes only those columns, enqueued on `stream`."""
        n = int(out_row.shape[0]) if out_row.dim() == 1 else -1
        lo, hi = self._cols_range(n, cols)
        self._check_block(table, (12, n), torch.float32, "table")
        self._check_block(out_row, (n,), self.dtype, "out_row")
        self._call("nmp_static_monthly", stream, hi - lo, n, _ptr(table, lo), int(m0), int(m1),
                   float(w), _ptr(out_row, lo))

    # ---- interval extremes (nmp_extremes_update / nmp_extremes_output) -----------
    def extremes_update(self, kind_rows, k: int, val: torch.Tensor, when: torch.Tensor,
                        diag: torch.Tensor | None = None, forcing: torch.Tensor | None = None,
                        state: torch.Tensor | None = None, stream=None,
                        cols: tuple[int, int] | None = None):
        """nmp_extremes_update: step k >= 1 of an output interval into the
        running extremes val (2*nseries, n), engine precision, and when
        (2*nseries, n) int32 -- row 2s the maximum of series s, row 2s + 1 its
        minimum.  kind_rows: the series' (kind, row) pairs (extremes.pairs);
        diag (NDIAG_OUT, n), forcing (NFORCING, n) and state (NSTATE, n) are the
        step's blocks, None where no series names one.  extremes.update_host
        is the numpy form.  cols=(lo, hi) updates only those columns, enqueued
        on `stream`."""
        kr = np.ascontiguousarray(np.asarray(kind_rows, np.int32).reshape(-1, 2))
        ns, n = int(kr.shape[0]), int(val.shape[1]) if val.dim() == 2 else -1
        lo, hi = self._cols_range(n, cols)
        self._check_block(val, (2 * ns, n), self.dtype, "val")
        self._check_block(when, (2 * ns, n), torch.int32, "when")
        for t, rows, what in ((diag, L.NDIAG_OUT, "diag"), (forcing, L.NFORCING, "forcing"),
                              (state, L.NSTATE, "state")):
            if t is not None:
                self._check_block(t, (rows, n), self.dtype, what)
        self._call("nmp_extremes_update", stream, hi - lo, n, ns,
                   kr.ctypes.data_as(C.POINTER(C.c_int32)), _ptr(diag, lo), _ptr(forcing, lo),
                   _ptr(state, lo), int(k), _ptr(val, lo), _ptr(when, lo), n)

    def extremes_output(self, stats, dt: float, val: torch.Tensor, when: torch.Tensor,
                        out_rows: torch.Tensor, stream=None,
                        cols: tuple[int, int] | None = None):
        """nmp_extremes_output: the output rows of the series' stat masks
        `stats` (extremes.masks; in series order, within a series MAX, MIN,
        TMAX, TMIN) from val and when into out_rows (the masks' bits in all,
        n), engine precision: values as stored, times (T)((double)when * dt)
        seconds.  out_rows may be rows of a block (a contiguous row slice).
        extremes.output_host is the numpy form.  cols=(lo, hi) writes only
        those columns, enqueued on `stream`."""
        m = np.ascontiguousarray(np.asarray(stats, np.int32).reshape(-1))
        ns, n = int(m.shape[0]), int(val.shape[1]) if val.dim() == 2 else -1
        lo, hi = self._cols_range(n, cols)
        self._check_block(val, (2 * ns, n), self.dtype, "val")
        self._check_block(when, (2 * ns, n), torch.int32, "when")
        if all(0 < int(x) < 16 for x in m):   # (the library refuses any other mask)
            nrow = sum(bin(int(x)).count("1") for x in m)
            self._check_block(out_rows, (nrow, n), self.dtype, "out_rows")
        self._call("nmp_extremes_output", stream, hi - lo, ns,
                   m.ctypes.data_as(C.POINTER(C.c_int32)), float(dt), _ptr(val, lo), _ptr(when, lo),
                   n, _ptr(out_rows, lo), n)

    # ---- interval statistics (nmp_intstats_update / nmp_intstats_output) ---------
    def intstats_update(self, table, thresholds, k: int, acc: torch.Tensor, cnt: torch.Tensor,
                        diag: torch.Tensor | None = None, forcing: torch.Tensor | None = None,
                        state: torch.Tensor | None = None, stream=None,
                        cols: tuple[int, int] | None = None):
        """nmp_intstats_update: step k >= 1 of an output interval into the
        running sums acc (nitems, n) float64 and the counters cnt (3*nitems,
        n) int32 -- row 3i the steps item i's condition held, 3i + 1 the
        current run, 3i + 2 the longest run.  table: the items' (kind, row,
        operator, stat mask) words (intstats.table); thresholds: one double per
        item (intstats.thresholds); diag (NDIAG_OUT, n), forcing (NFORCING, n)
        and state (NSTATE, n) are the step's blocks, None where no item names
        one.  intstats.update_host is the numpy form.  cols=(lo, hi) updates
        only those columns, enqueued on `stream`."""
        tab = np.ascontiguousarray(np.asarray(table, np.int32).reshape(-1, 4))
        thr = np.ascontiguousarray(np.asarray(thresholds, np.float64).reshape(-1))
        ni, n = int(tab.shape[0]), int(acc.shape[1]) if acc.dim() == 2 else -1
        assert thr.shape[0] == ni, "one threshold per item"
        lo, hi = self._cols_range(n, cols)
        self._check_block(acc, (ni, n), torch.float64, "acc")
        self._check_block(cnt, (3 * ni, n), torch.int32, "cnt")
        for t, rows, what in ((diag, L.NDIAG_OUT, "diag"), (forcing, L.NFORCING, "forcing"),
                              (state, L.NSTATE, "state")):
            if t is not None:
                self._check_block(t, (rows, n), self.dtype, what)
        self._call("nmp_intstats_update", stream, hi - lo, n, ni,
                   tab.ctypes.data_as(C.POINTER(C.c_int32)),
                   thr.ctypes.data_as(C.POINTER(C.c_double)), _ptr(diag, lo), _ptr(forcing, lo),
                   _ptr(state, lo), int(k), _ptr(acc, lo), _ptr(cnt, lo), n)

    def intstats_output(self, table, k: int, dt: float, acc: torch.Tensor, cnt: torch.Tensor,
                        out_rows: torch.Tensor, stream=None,
                        cols: tuple[int, int] | None = None):
        """nmp_intstats_output: the output rows of the items' stat masks (in
        item order, within an item MEAN, DUR, DEG, SPELL) from acc and cnt
        after the interval's k steps of dt seconds into out_rows (the masks'
        bits in all, n), engine precision: (T)(acc / (double)k), (T)((double)
        count * dt), (T)(acc * dt), (T)((double)longest * dt).  out_rows may
        be rows of a block (a contiguous row slice).  intstats.output_host is
        the numpy form.  cols=(lo, hi) writes only those columns, enqueued on
        `stream`."""
        tab = np.ascontiguousarray(np.asarray(table, np.int32).reshape(-1, 4))
        ni, n = int(tab.shape[0]), int(acc.shape[1]) if acc.dim() == 2 else -1
        lo, hi = self._cols_range(n, cols)
        self._check_block(acc, (ni, n), torch.float64, "acc")
        self._check_block(cnt, (3 * ni, n), torch.int32, "cnt")
        if all(0 < int(x) < 16 for x in tab[:, 3]):   # (the library refuses any other mask)
            nrow = sum(bin(int(x)).count("1") for x in tab[:, 3])
            self._check_block(out_rows, (nrow, n), self.dtype, "out_rows")
        self._call("nmp_intstats_output", stream, hi - lo, ni,
                   tab.ctypes.data_as(C.POINTER(C.c_int32)), int(k), float(dt), _ptr(acc, lo),
                   _ptr(cnt, lo), n, _ptr(out_rows, lo), n)

    # ---- region-aggregated output (nmp_region_reduce) ---------------------------
    def region_reduce(self, fields: torch.Tensor, plan, sums: torch.Tensor,
                      means: torch.Tensor | None = None, stream=None):
        """nmp_region_reduce: sums[f, r] (and means[f, r] = sums / plan.wsum)
        of the (nfield, n) block `fields` (engine precision) over the columns
        of each region of `plan` (regions.RegionPlan on this device, built for
        n columns), float64 (nfield, nreg), by the plan's fixed summation
        tree; enqueued on `stream`.  The pass-1 scratch lives with the plan, so
        calls that share a plan must be ordered by their streams."""
        assert fields.dim() == 2, tuple(fields.shape)
        nf, n = int(fields.shape[0]), int(fields.shape[1])
        assert plan.dev is not None and plan.ncol == n, "plan.to(device) for this block"
        self._check_block(fields, (nf, n), self.dtype, "fields")
        self._check_block(sums, (nf, plan.nreg), torch.float64, "sums")
        if means is not None:
            self._check_block(means, (nf, plan.nreg), torch.float64, "means")
        d = plan.dev
        self._check_block(d["entry_col"], (plan.nchunk * L.REGION_CHUNK,), torch.int32, "entry_col")
        self._check_block(d["entry_w"], (plan.nchunk * L.REGION_CHUNK,), torch.float64, "entry_w")
        self._check_block(d["region_chunk0"], (plan.nreg + 1,), torch.int64, "region_chunk0")
        self._check_block(d["wsum"], (plan.nreg,), torch.float64, "wsum")
        self._call("nmp_region_reduce", stream, n, n, nf, _ptr(fields), plan.nchunk,
                   _ptr(d["entry_col"]), _ptr(d["entry_w"]), plan.nreg, _ptr(d["region_chunk0"]),
                   _ptr(d["wsum"]), _ptr(plan.partial(nf)), _ptr(sums), _ptr(means))

    # ---- the reference's other public routines (nmp_frh2o / nmp_calhum) ------
    def frh2o(self, sltyp, tkelv, smc, sh2o, status=None, stream=None):
        """frh2o (func.f90:4494-4598) elementwise.  Device tensors (engine
        precision, int32 sltyp) -> a new tensor of FREE, enqueued on `stream`;
        numpy arrays -> numpy (nmp_frh2o_host, synchronous).  `status` (int32,
        same kind as the inputs) receives NMP_ST_FLERCH / NMP_ST_STOP bits."""
        n = int(len(tkelv))
        if isinstance(tkelv, np.ndarray):
            rt = np.float32 if self.precision == 4 else np.float64
            a = [np.ascontiguousarray(x, rt) for x in (tkelv, smc, sh2o)]
            si = np.ascontiguousarray(sltyp, np.int32)
            # the library copies n elements of every array: a shorter one would be over-read
            for x in (*a, si):
                assert x.shape == (n,), f"frh2o: every input must have shape ({n},), got {x.shape}"
            out = np.empty(n, rt)
            st = status if status is not None else np.zeros(n, np.int32)
            assert st.dtype == np.int32 and st.flags.c_contiguous and st.shape == (n,)
            _lib.check(self._lib.nmp_frh2o_host(self._h, n, C.c_void_p(si.ctypes.data),
                                                *[C.c_void_p(x.ctypes.data) for x in a],
                                                C.c_void_p(out.ctypes.data),
                                                C.c_void_p(st.ctypes.data)), "nmp_frh2o_host")
            return out
        for t in (tkelv, smc, sh2o):
            assert t.dtype == self.dtype and t.is_contiguous() and t.shape == (n,)
            assert t.device.type == "cuda" and t.device.index == self.device
        assert sltyp.dtype == torch.int32 and sltyp.is_contiguous() and sltyp.shape == (n,)
        assert sltyp.device.type == "cuda" and sltyp.device.index == self.device, sltyp.device
        if status is not None:
            # the kernel ORs int32 bits into n elements of it on the device
            assert status.dtype == torch.int32 and status.is_contiguous() and status.shape == (n,)
            assert status.device.type == "cuda" and status.device.index == self.device
        out = torch.empty(n, dtype=self.dtype, device=tkelv.device)
        self._call("nmp_frh2o", stream, n, _ptr(sltyp), _ptr(tkelv), _ptr(smc), _ptr(sh2o),
                   _ptr(out), _ptr(status))
        return out

    def calhum(self, sfctmp, sfcprs, stream=None):
        """calhum (func.f90:3958-3984) elementwise -> (Q2SAT, DQSDT2); device
        tensors (enqueued on `stream`) or numpy arrays (synchronous)."""
        n = int(len(sfctmp))
        if isinstance(sfctmp, np.ndarray):
            rt = np.float32 if self.precision == 4 else np.float64
            t, p = (np.ascontiguousarray(x, rt) for x in (sfctmp, sfcprs))
            assert t.shape == p.shape == (n,), f"calhum: inputs must have shape ({n},)"
            q, d = np.empty(n, rt), np.empty(n, rt)
            _lib.check(self._lib.nmp_calhum_host(self._h, n, C.c_void_p(t.ctypes.data),
                                                 C.c_void_p(p.ctypes.data), C.c_void_p(q.ctypes.data),
                                                 C.c_void_p(d.ctypes.data)), "nmp_calhum_host")
            return q, d
        for x in (sfctmp, sfcprs):
            assert x.dtype == self.dtype and x.is_contiguous() and x.shape == (n,)
            assert x.device.type == "cuda" and x.device.index == self.device
        q = torch.empty(n, dtype=self.dtype, device=sfctmp.device)
        d = torch.empty_like(q)
        self._call("nmp_calhum", stream, n, _ptr(sfctmp), _ptr(sfcprs), _ptr(q), _ptr(d))
        return q, d

    def sflx_columns(self, rec: np.ndarray) -> np.ndarray:
        """noahmp_sflx with the reference calling sequence on host records
        (layout.sflx_args_dtype(); nmp_sflx_columns), updated in place and returned.
        Synchronous: packs, steps on the engine's GPU, unpacks."""
        assert rec.dtype == L.sflx_args_dtype() and rec.flags.c_contiguous and rec.ndim == 1
        _lib.check(self._lib.nmp_sflx_columns(self._h, C.c_void_p(rec.ctypes.data),
                                              int(rec.shape[0])), "nmp_sflx_columns")
        return rec

    def run(self, cs: ColumnState, forcings: torch.Tensor, zsoil, dt: float, julian0: float,
            yearlen: int, nsteps: int, diag: torch.Tensor | None = None,
            diag_level: int = L.DIAG_NONE, stream=None, out_every: int | None = None):
        """nsteps steps in one launch, cycling through forcings[(period, 12, n)].

        Diagnostics: with `out_every` None, `diag` (nd, n) receives the last step
        (nmp_run); otherwise every out_every-th step writes the next slot of the
        ring `diag` (slots, nd, n), wrapping (nmp_run_out)."""
        n = cs.ncol
        assert forcings.dim() == 3
        self._check_cols(cs, forcings[0])
        zs = (C.c_float * 4)(*[float(z) for z in zsoil])
        if diag_level != L.DIAG_NONE:
            nd = L.NDIAG_FULL if diag_level == L.DIAG_FULL_LEVEL else L.NDIAG_OUT
            assert diag is not None and diag.dim() == (2 if out_every is None else 3)
            self._check_block(diag, tuple(diag.shape[:-2]) + (nd, n), self.dtype, "diag")
        args = (n, n, zs, float(dt), float(julian0), int(yearlen), int(nsteps), _ptr(cs.state),
                _ptr(cs.isnow), _ptr(cs.static_f), _ptr(cs.static_i), _ptr(forcings),
                L.NFORCING * n, forcings.shape[0], _ptr(diag), int(diag_level))
        if out_every is None:
            self._call("nmp_run", stream, *args, _ptr(cs.status))
            return
        slots = diag.shape[0] if diag is not None else 1
        dstride = diag[0].numel() if diag is not None else 0
        self._call("nmp_run_out", stream, *args, int(out_every), int(slots), int(dstride),
                   _ptr(cs.status))


class StreamShards:
    """Steps one ColumnState as `nshards` column ranges, each on its own HIP stream.

    Columns are independent and a range's step t+1 depends only on its own step
    t, so the ranges' launches need no synchronisation with each other.  While
    one range's launch drains its last waves, the other range's waves fill the
    idle SIMDs, which hides the per-launch tail (DESIGN.md "Launch structure").
    `join()` makes a stream wait for every range, and is needed before the
    caller reads state or diagnostics."""

    def __init__(self, engine: Engine, cs: ColumnState, nshards: int = 2, device=None,
                 rebin_tile: int = 0, rebin_every: int = 1, launch_cols: int = 0,
                 first_frac: float | None = None, stagger: bool = False):
        """rebin_tile > 0 turns on column re-binning (nmp_step_binned /
        nmp_rebin): every `rebin_every` steps each range re-sorts its columns
        within tiles of rebin_tile columns by the trip counts the previous step
        recorded, and the next launches step them in that order.
        launch_cols > 0 (launch-size study): each range is stepped as
        sequential launches of at most launch_cols columns on its stream.
        first_frac (two ranges only): the first range's share of the columns
        (default: equal ranges).  stagger: the first step of range i > 0 starts
        after range i - 1's first launch, so the ranges run out of phase (their
        launches' ramp and drain fall on the other range's full waves)."""
        n = cs.ncol
        nshards = max(1, min(int(nshards), max(n, 1)))
        self.engine, self.cs = engine, cs
        dev = torch.device("cuda", engine.device) if device is None else torch.device(device)
        self.streams = [torch.cuda.Stream(dev) for _ in range(nshards)]
        self.ranges = [(n * i // nshards, n * (i + 1) // nshards) for i in range(nshards)]
        if first_frac is not None and nshards == 2:
            cut = min(max(int(round(n * first_frac)) // 256 * 256, 0), n)
            self.ranges = [(0, cut), (cut, n)]
        self.rebin_tile, self.rebin_every, self.nstep = int(rebin_tile), max(1, int(rebin_every)), 0
        self.launch_cols = int(launch_cols)
        self.stagger, self._stag_ev = bool(stagger), None
        assert not (self.launch_cols and self.rebin_tile), "launch_cols: plain launches only"
        self.order = self.cost = None
        if self.rebin_tile:
            # identity order to start with, relative to each range's first column
            self.order = torch.cat([torch.arange(hi - lo, dtype=torch.int32)
                                    for lo, hi in self.ranges]).to(dev) if n else \
                torch.zeros(0, dtype=torch.int32, device=dev)
            self.cost = torch.zeros(n, dtype=torch.uint8, device=dev)

    def step(self, forcing: torch.Tensor, zsoil, dt: float, julian: float, yearlen: int,
             diag: torch.Tensor | None = None, diag_level: int = L.DIAG_NONE, events=None,
             after="current", pre=None, post=None):
        """One step of every range.  `after`: the stream, or a tuple of streams
        and events, whose pending work (the forcing upload, a previous reader
        of `diag`) each range waits for first -- by default the caller's current stream,
        where torch enqueues uploads; tensors are kept alive until the ranges
        are done with them.  Pass None only when the inputs are known to be
        complete (e.g. after a synchronize).
        events: per-range (start, end) pairs.  pre(stream, (lo, hi)): work
        enqueued on each range's stream before its step (e.g. generating that
        range's forcing on the device, Engine.forcing_synth).
        post(stream, (lo, hi)): work enqueued on each range's stream after its
        step and before its end event (e.g. Engine.accumulate on the step's
        diagnostics)."""
        if isinstance(after, str) and after == "current":
            after = torch.cuda.current_stream(self.streams[0].device)
        if after is not None and not isinstance(after, (tuple, list)):
            after = (after,)
        for i, (st, rng) in enumerate(zip(self.streams, self.ranges)):
            if after is not None:
                for a in after:
                    if isinstance(a, torch.cuda.Event):
                        st.wait_event(a)
                    else:
                        st.wait_stream(a)
                forcing.record_stream(st)
                if diag is not None:
                    diag.record_stream(st)
            if self.stagger and self.nstep == 0 and i > 0:
                st.wait_event(self._stag_ev)
            if pre is not None:
                pre(st, rng)
            if events is not None:
                events[i][0].record(st)
            if self.rebin_tile and self.nstep > 0 and self.nstep % self.rebin_every == 0:
                self.engine.rebin(self.cost, self.order, self.rebin_tile, stream=st, cols=rng)
            if self.launch_cols:
                for lo in range(rng[0], rng[1], self.launch_cols):
                    self.engine.step(self.cs, forcing, zsoil, dt, julian, yearlen, diag,
                                     diag_level, stream=st,
                                     cols=(lo, min(lo + self.launch_cols, rng[1])))
            else:
                self.engine.step(self.cs, forcing, zsoil, dt, julian, yearlen, diag, diag_level,
                                 stream=st, cols=None if len(self.streams) == 1 else rng,
                                 order=self.order, cost=self.cost)
            if post is not None:
                post(st, rng)
            if events is not None:
                events[i][1].record(st)
            if self.stagger and self.nstep == 0:
                self._stag_ev = torch.cuda.Event()
                self._stag_ev.record(st)
        self.nstep += 1

    @property
    def producers(self):
        """Every stream that writes the ranges' state and diagnostics."""
        return list(self.streams)

    def join(self, stream: torch.cuda.Stream | None = None):
        """Make `stream` (default: the current stream) wait for every range."""
        s = stream if stream is not None else torch.cuda.current_stream(self.streams[0].device)
        for st in self.producers:
            s.wait_stream(st)
