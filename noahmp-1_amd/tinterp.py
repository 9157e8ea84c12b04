"""Forcing between input times, host side: the numpy twin of
nmp_forcing_from_ldasin_interp and nmp_ldasin_cosz (include/noahmp_engine.h
states the operation order; csrc/interp.hip is the device form).

A step that starts at t, t0 <= t < t1, takes its forcing from the LDASIN
blocks of the input times t0 and t1 with the weights `weights(t, t0, every)`:
plain variables linearly, held variables (the default holds RAINRATE, an
interval rate) from block 0, and SWDOWN by its clearness ratio -- each end
point's SWDOWN divided by the cosine of the solar zenith angle there (bounded
below by `cosz_floor`), interpolated linearly and multiplied by the step's own
COSZ, so the radiation follows the sun between the files instead of cutting
across its arc.

Every operation is one IEEE double operation, each result rounded once to
fp32: given the three COSZ rows the device used (its double cosine is not
correctly rounded), `interp_host` returns the device's bits.
"""
from __future__ import annotations

import datetime

import numpy as np

from . import layout as L, timeman

DEFAULT_HOLD = ("RAINRATE",)
DEFAULT_COSZ_FLOOR = 0.05
_V = L.LDASIN.index
_F = L.FORCING.index
# LDASIN row -> forcing row of the 8 file variables (PSFC also feeds SFCPRS)
_ROWS = [(_V("T2D"), _F("SFCTMP")), (_V("Q2D"), _F("Q2")), (_V("U2D"), _F("UU")),
         (_V("V2D"), _F("VV")), (_V("PSFC"), _F("PSFC")), (_V("RAINRATE"), _F("PRCP")),
         (_V("SWDOWN"), _F("SOLDN")), (_V("LWDOWN"), _F("LWDN"))]


def hold_mask(names) -> int:
    """Bit v for every LDASIN variable name (or index) in `names`; COSZ is no
    file variable and cannot be held."""
    m = 0
    for v in names:
        i = _V(v) if isinstance(v, str) else int(v)
        if not 0 <= i < L.NLDASIN - 1:
            raise ValueError(f"cannot hold {v!r}: not one of {L.LDASIN[:-1]}")
        m |= 1 << i
    return m


def weights(t: datetime.datetime, t0: datetime.datetime, every: datetime.timedelta):
    """(w0, w1) of the step that starts at t in the input interval
    [t0, t0 + every): w1 = (t - t0) / every in double, w0 = 1.0 - w1."""
    w1 = (t - t0).total_seconds() / every.total_seconds()
    if not 0.0 <= w1 < 1.0:
        raise ValueError(f"{t.isoformat()} is outside the input interval of {t0.isoformat()}")
    return 1.0 - w1, w1


def check_args(w1: float, mask: int, sw_zenith: bool, cosz_floor: float):
    """The library's argument rules (NMP_E_ARG), as a ValueError."""
    if not (0.0 <= w1 < 1.0):
        raise ValueError(f"w1 must lie in [0, 1), not {w1!r}")
    if mask < 0 or mask >> (L.NLDASIN - 1):
        raise ValueError(f"hold_mask {mask:#x} has a bit at or above COSZ")
    if sw_zenith and not (0.0 < cosz_floor <= 1.0):
        raise ValueError(f"cosz_floor must lie in (0, 1], not {cosz_floor!r}")


def cosz_row_host(lat_rad, lon_rad, t: datetime.datetime, sincos_lat=None) -> np.ndarray:
    """The fp32 COSZ row at time t from timeman.cosz (numpy's cosine: it can
    differ from the device's row by one fp32 ulp)."""
    return np.asarray(timeman.cosz(lat_rad, lon_rad, timeman.julian(t), timeman.yearlen(t.year),
                                   sincos_lat=sincos_lat)).astype(np.float32)


def interp_host(blk0, blk1, w1: float, cosz_t, hold_mask: int = 1 << _V("RAINRATE"),
                sw_zenith: bool = True, cosz_floor: float = DEFAULT_COSZ_FLOOR) -> np.ndarray:
    """nmp_forcing_from_ldasin_interp in numpy: the (12, n) fp32 forcing of a
    step from the (NLDASIN, n) fp32 blocks of its interval's ends (their COSZ
    rows: COSZ at the input times), the weight w1 and the step's fp32 COSZ row
    `cosz_t`.  blk1 may be None when w1 == 0."""
    check_args(w1, hold_mask, sw_zenith, cosz_floor)
    b0 = np.asarray(blk0, np.float32)
    n = b0.shape[1]
    czt32 = np.asarray(cosz_t, np.float32)
    assert b0.shape == (L.NLDASIN, n) and czt32.shape == (n,)
    w1 = np.float64(w1)
    w0 = np.float64(1.0) - w1
    res = np.empty((L.NLDASIN - 1, n), np.float32)
    if w1 == 0.0:
        res[...] = b0[:L.NLDASIN - 1]  # block 0's step: block 1 is not read
    else:
        b1 = np.asarray(blk1, np.float32)
        assert b1.shape == b0.shape
        floor = np.float64(cosz_floor)
        with np.errstate(all="ignore"):
            for v in range(L.NLDASIN - 1):
                a = b0[v].astype(np.float64)
                if (hold_mask >> v) & 1:
                    res[v] = b0[v]
                elif sw_zenith and v == _V("SWDOWN"):
                    czt = czt32.astype(np.float64)
                    cz0 = b0[_V("COSZ")].astype(np.float64)
                    cz1 = b1[_V("COSZ")].astype(np.float64)
                    m0 = np.where(cz0 > floor, cz0, floor)
                    m1 = np.where(cz1 > floor, cz1, floor)
                    k0 = a / m0
                    k1 = b1[v].astype(np.float64) / m1
                    k = k0 * w0 + k1 * w1
                    res[v] = np.where(czt > 0.0, czt * k, 0.0).astype(np.float32)
                else:
                    res[v] = (a * w0 + b1[v].astype(np.float64) * w1).astype(np.float32)
    out = np.empty((L.NFORCING, n), np.float32)
    for v, f in _ROWS:
        out[f] = res[v]
    psfc = res[_V("PSFC")]
    out[_F("SFCPRS")] = psfc
    out[_F("COSZ")] = czt32
    with np.errstate(all="ignore"):
        out[_F("CO2AIR")] = (395.0e-6 * psfc.astype(np.float64)).astype(np.float32)
        out[_F("O2AIR")] = (0.209 * psfc.astype(np.float64)).astype(np.float32)
    return out
