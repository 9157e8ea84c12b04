"""Interval extremes (nmp_extremes_update / nmp_extremes_output): the series
an offline run can track over each output interval -- their maximum, their
minimum and the time each occurred -- the spec that selects them, their LDASOUT
row names, and the two kernels' numpy restatement.

A series is one value per column per step: a row of the step's 16 output
fluxes (layout.DIAG_OUT), of its forcing block (layout.FORCING) or of the state
the step left (the single-row fields of layout.STATE_FIELDS and the soil layers
SMC1..4, SH2O1..4, STC1..4).  Snow-layer rows are not offered: an inactive
layer holds a stale value.

The rule (include/noahmp_engine.h "Interval extremes") moves values, it does no
arithmetic on them, so `update_host` and `output_host` equal csrc/extremes.hip
bit for bit in fp32 and fp64, NaN payloads and the sign of zero included.
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

from . import layout as L

DEFAULT_STATS = L.EXT_MAX | L.EXT_MIN
# the stat bits in output-row order
STAT_ORDER = [("MAX", L.EXT_MAX), ("MIN", L.EXT_MIN), ("TMAX", L.EXT_TMAX), ("TMIN", L.EXT_TMIN)]
_ALL = L.EXT_MAX | L.EXT_MIN | L.EXT_TMAX | L.EXT_TMIN
_NROWS = {L.EXT_SRC_DIAG: L.NDIAG_OUT, L.EXT_SRC_FORCING: L.NFORCING, L.EXT_SRC_STATE: L.NSTATE}


class Series(NamedTuple):
    name: str
    kind: int    # layout.EXT_SRC_*
    row: int     # the row of its block
    stats: int   # mask of layout.EXT_MAX | EXT_MIN | EXT_TMAX | EXT_TMIN


def _sources() -> dict:
    """name -> (kind, row) of every series on offer."""
    out = {}
    for i, n in enumerate(L.DIAG_OUT):
        out[n] = (L.EXT_SRC_DIAG, i)
    for i, n in enumerate(L.FORCING):
        out[n] = (L.EXT_SRC_FORCING, i)
    for n, w in L.STATE_FIELDS:
        if w == 1:
            out[n] = (L.EXT_SRC_STATE, L.STATE_OFF[n][0])
    for i in range(1, L.NSOIL + 1):
        out[f"SMC{i}"] = (L.EXT_SRC_STATE, L.si("SMC") + i - 1)
        out[f"SH2O{i}"] = (L.EXT_SRC_STATE, L.si("SH2O") + i - 1)
        out[f"STC{i}"] = (L.EXT_SRC_STATE, L.si("STC") + 2 + i)   # soil layer i of the 7 layers
    return out


SOURCES = _sources()
assert len(SOURCES) == 16 + 12 + 28 + 12


def parse_stats(stats) -> int:
    """The stat mask of "max+tmax", an iterable of stat names or a mask."""
    if isinstance(stats, (int, np.integer)) and not isinstance(stats, bool):
        m = int(stats)
        if m <= 0 or m & ~_ALL:
            raise ValueError(f"extremes: stat mask {m:#x} is empty or has a bit above {L.EXT_TMIN}")
        return m
    names = stats.split("+") if isinstance(stats, str) else list(stats)
    m = 0
    for s in names:
        key = str(s).strip().upper()
        if key not in L.EXT_STATS:
            raise ValueError(f"extremes: unknown stat {s!r} (one of max, min, tmax, tmin)")
        m |= L.EXT_STATS[key]
    if not m:
        raise ValueError("extremes: no stat selected")
    return m


def parse(spec) -> list:
    """The series of "T2M,TRAD:max,PRCP:max+tmax", or of an iterable of names
    (each may carry its ":stats") or (name, stats) pairs; the default stats are
    max+min.  ValueError for an unknown name or stat, a duplicate, an empty
    selection and more than layout.EXT_MAXSERIES series."""
    if isinstance(spec, str):
        items = [s.strip() for s in spec.split(",") if s.strip()]
    else:
        items = list(spec)
    out, seen = [], set()
    for it in items:
        if isinstance(it, Series):
            name, stats = it.name, it.stats
        elif isinstance(it, str):
            name, _, st = it.partition(":")
            name, stats = name.strip(), (parse_stats(st) if st.strip() else DEFAULT_STATS)
            if ":" in it and not st.strip():
                raise ValueError(f"extremes: no stat after ':' in {it!r}")
        else:
            name, st = it
            name, stats = str(name).strip(), parse_stats(st)
        if name not in SOURCES:
            raise ValueError(f"extremes: unknown series {name!r} (an output flux, a forcing row, a "
                             "single-row state field or SMC1..4, SH2O1..4, STC1..4)")
        if name in seen:
            raise ValueError(f"extremes: series {name!r} named twice")
        seen.add(name)
        out.append(Series(name, *SOURCES[name], parse_stats(stats)))
    if not out:
        raise ValueError("extremes: no series selected")
    if len(out) > L.EXT_MAXSERIES:
        raise ValueError(f"extremes: {len(out)} series, at most {L.EXT_MAXSERIES}")
    return out


def spec_string(series) -> str:
    """The canonical spec of `series` (what a restart carries): parse() of it
    gives them back."""
    return ",".join(f"{s.name}:" + "+".join(n.lower() for n, b in STAT_ORDER if s.stats & b)
                    for s in series)


def row_names(series) -> list:
    """<NAME>_MAX, _MIN, _TMAX, _TMIN of the series' output rows, in
    nmp_extremes_output's row order."""
    return [f"{s.name}_{n}" for s in series for n, b in STAT_ORDER if s.stats & b]


def pairs(series) -> np.ndarray:
    """The (kind, row) pairs nmp_extremes_update takes, int32 (nseries, 2)."""
    return np.array([[s.kind, s.row] for s in series], np.int32).reshape(-1, 2)


def masks(series) -> np.ndarray:
    """The stat masks nmp_extremes_output takes, int32 (nseries,)."""
    return np.array([s.stats for s in series], np.int32)


def has_diag(series) -> bool:
    return any(s.kind == L.EXT_SRC_DIAG for s in series)


def _check(kind_rows):
    kr = np.asarray(kind_rows, np.int64).reshape(-1, 2)
    if not 1 <= kr.shape[0] <= L.EXT_MAXSERIES:
        raise ValueError(f"extremes: {kr.shape[0]} series, 1..{L.EXT_MAXSERIES} allowed")
    for kind, row in kr:
        if int(kind) not in _NROWS:
            raise ValueError(f"extremes: series kind {kind} is none of the three")
        if not 0 <= row < _NROWS[int(kind)]:
            raise ValueError(f"extremes: row {row} outside its block of {_NROWS[int(kind)]}")
    return kr


def update_host(val: np.ndarray, when: np.ndarray, k: int, kind_rows, diag=None, forcing=None,
                state=None):
    """nmp_extremes_update in numpy, in place: val (2*nseries, n) of the
    blocks' dtype and when (2*nseries, n) int32 after step k >= 1 of the
    interval, from the step's diag (16, n), forcing (12, n) and state (56, n)
    (None where no series names the block).  kind_rows: (kind, row) pairs
    (pairs()).  Values are moved, never computed with."""
    kr = _check(kind_rows)
    k = int(k)
    if k < 1:
        raise ValueError("extremes: k counts the interval's steps from 1")
    blocks = {L.EXT_SRC_DIAG: diag, L.EXT_SRC_FORCING: forcing, L.EXT_SRC_STATE: state}
    assert val.shape[0] == when.shape[0] == 2 * kr.shape[0] and when.dtype == np.int32
    with np.errstate(invalid="ignore"):
        for s, (kind, row) in enumerate(kr):
            block = blocks[int(kind)]
            if block is None:
                raise ValueError("extremes: a named series' block is missing")
            v = np.asarray(block)[row]
            assert v.dtype == val.dtype, (v.dtype, val.dtype)
            if k == 1:
                val[2 * s], val[2 * s + 1] = v, v
                when[2 * s], when[2 * s + 1] = 1, 1
                continue
            mx, mn = val[2 * s], val[2 * s + 1]
            take = (v > mx) | ((mx != mx) & (v == v))
            mx[take] = v[take]
            when[2 * s][take] = k
            take = (v < mn) | ((mn != mn) & (v == v))
            mn[take] = v[take]
            when[2 * s + 1][take] = k
    return val, when


def output_host(val: np.ndarray, when: np.ndarray, stats, dt: float) -> np.ndarray:
    """nmp_extremes_output in numpy: the output rows (sum of the masks' bits,
    n) of val's dtype T -- a value row is val as stored, a time row
    (T)((double)when * dt)."""
    stats = [int(m) for m in np.asarray(stats).reshape(-1)]
    if not 1 <= len(stats) <= L.EXT_MAXSERIES:
        raise ValueError(f"extremes: {len(stats)} series, 1..{L.EXT_MAXSERIES} allowed")
    dt = float(dt)
    if not (np.isfinite(dt) and dt > 0.0):
        raise ValueError("extremes: dt must be finite and positive")
    assert val.shape[0] == when.shape[0] == 2 * len(stats)
    rows = []
    for s, m in enumerate(stats):
        if m <= 0 or m & ~_ALL:
            raise ValueError(f"extremes: stat mask {m:#x} is empty or has a bit above "
                             f"{L.EXT_TMIN}")
        if m & L.EXT_MAX:
            rows.append(val[2 * s].copy())
        if m & L.EXT_MIN:
            rows.append(val[2 * s + 1].copy())
        if m & L.EXT_TMAX:
            rows.append((when[2 * s].astype(np.float64) * np.float64(dt)).astype(val.dtype))
        if m & L.EXT_TMIN:
            rows.append((when[2 * s + 1].astype(np.float64) * np.float64(dt)).astype(val.dtype))
    return np.stack(rows)
