"""Vegetation fraction through the year, host side: the numpy twin of
nmp_static_monthly (include/noahmp_engine.h states the operation order;
csrc/vegclim.hip is the device form) and the date arithmetic around it.

With opt_veg = 1 the green vegetation fraction SHDFAC is the vegetated
fraction of every column (noahmp_sflx sets fveg = SHDFAC,
core/module_noahmp_func.f90:366-368).  The static file carries it as 12
monthly GREENFRAC grids, taken as mid-month values of 12 equal months;
`month_weights` places a date between two of them exactly as
ncio.read_static does for the run's first instant, and `shdfac_host` forms the
row.  SHDFAC is a pure function of the instant it is evaluated at -- the
step's start, or 00:00 of its day (`quantise`) -- so no state travels in
restarts, and a jump back in time or a spin-up rewind is right by
construction.

Every operation is one IEEE double operation, the result rounded once to fp32
and then widened: `shdfac_host` returns the device's bits, and at the run's
first instant ncio.read_static's.
"""
from __future__ import annotations

import datetime
import math

import numpy as np

from . import timeman

CADENCES = ("daily", "step")


def month_weights(when: datetime.datetime):
    """(m0, m1, w): the months (0..11) whose mid-month values bracket `when`
    and the weight of the later one, 0 <= w < 1; ncio._month_weighted's
    arithmetic.  Early January lies between December (m0 = 11) and January."""
    t = 12.0 * timeman.julian(when) / timeman.yearlen(when.year) - 0.5
    f = math.floor(t)
    m0 = int(f) % 12
    return m0, (m0 + 1) % 12, t - f


def quantise(t0: datetime.datetime, cadence: str) -> datetime.datetime:
    """The instant the SHDFAC of the step that starts at t0 is evaluated at:
    "step" = t0 itself (the instant whose JULIAN the step is given), "daily" =
    00:00 of t0's day on the model clock."""
    if cadence == "step":
        return t0
    if cadence == "daily":
        return datetime.datetime(t0.year, t0.month, t0.day)
    raise ValueError(f"veg_clim must be one of {CADENCES} or None, not {cadence!r}")


def check_table(table12, ncol: int | None = None) -> np.ndarray:
    """The (12, ncol) fp32 table of a run, or a ValueError."""
    g = np.asarray(table12)
    if g.ndim != 2 or g.shape[0] != 12 or (ncol is not None and g.shape[1] != ncol):
        raise ValueError("greenfrac must have shape (12, "
                         f"{'ncol' if ncol is None else ncol}), not {g.shape}")
    return np.ascontiguousarray(g, np.float32)


def static_monthly_host(table12: np.ndarray, m0: int, m1: int, w: float,
                        dtype=np.float32) -> np.ndarray:
    """nmp_static_monthly in numpy: table12 (12, n) float32 -> (n,) `dtype`.
    The library's argument rules (NMP_E_ARG) are a ValueError."""
    if not (0 <= int(m0) <= 11 and 0 <= int(m1) <= 11):
        raise ValueError(f"m0 and m1 must lie in 0..11, not {m0!r}, {m1!r}")
    if not (0.0 <= w < 1.0):
        raise ValueError(f"w must lie in [0, 1), not {w!r}")
    g = np.asarray(table12)
    assert g.dtype == np.float32 and g.ndim == 2 and g.shape[0] == 12, (g.dtype, g.shape)
    w = float(w)
    u = 1.0 - w
    with np.errstate(all="ignore"):
        a = g[int(m0)].astype(np.float64)
        b = g[int(m1)].astype(np.float64)
        r = (u * a + w * b).astype(np.float32)   # two rounded products, one add, one rounding
    return r.astype(dtype)


def shdfac_host(table12: np.ndarray, when: datetime.datetime, dtype=np.float32) -> np.ndarray:
    """The SHDFAC row at `when` from the (12, n) float32 climatology: the
    kernel restated operation for operation."""
    m0, m1, w = month_weights(when)
    return static_monthly_host(table12, m0, m1, w, dtype)
