"""Interval statistics (nmp_intstats_update / nmp_intstats_output): what an
offline run can say about the steps of each output interval beyond their
extremes -- the mean of a series, or, for a series with a condition, how long
the condition held, its longest unbroken spell and the value-seconds beyond the
threshold -- the spec that selects the items, their LDASOUT row names, and the
two kernels' numpy restatement.

An item is a series with either nothing or a condition attached.  The series
are those of extremes.SOURCES: a row of the step's 16 output fluxes, of its
forcing block or of the state the step left (single-row fields and the soil
layers SMC1..4, SH2O1..4, STC1..4; no snow-layer rows).  A condition is an
operator gt, ge, lt or le and a threshold.

Spec: comma-separated items `[LABEL=]NAME[@OPc][:stat+stat]`:
  T2M  or  T2M:mean                 -> T2M_MEAN
  FROST=T2M@lt273.15:dur+spell      -> FROST_DUR, FROST_SPELL
  GDD=SFCTMP@gt278.15:deg           -> GDD_DEG
  SNOWCOV=SNEQV@gt1                 -> SNOWCOV_DUR
An item without a condition takes `mean` and only `mean` (its label defaults to
the series' name); a conditioned item takes any of dur, deg, spell (default
dur) and must carry a label.

The rule (include/noahmp_engine.h "Interval statistics") is one double add per
step and item and one division or product and one conversion at output, so
`update_host` and `output_host` equal csrc/intstats.hip bit for bit in fp32 and
fp64.
"""
from __future__ import annotations

import math
import re
from typing import NamedTuple

import numpy as np

from . import layout as L
from .extremes import SOURCES

# the stat bits in output-row order
STAT_ORDER = [("MEAN", L.IST_MEAN), ("DUR", L.IST_DUR), ("DEG", L.IST_DEG),
              ("SPELL", L.IST_SPELL)]
_COND = L.IST_DUR | L.IST_DEG | L.IST_SPELL
_NROWS = {L.EXT_SRC_DIAG: L.NDIAG_OUT, L.EXT_SRC_FORCING: L.NFORCING, L.EXT_SRC_STATE: L.NSTATE}
_OP_NAMES = {v: k for k, v in L.IST_OPS.items()}
_LABEL = re.compile(r"[A-Z][A-Z0-9_]*\Z")
MAX_LABEL = 24


class Item(NamedTuple):
    label: str   # the prefix of its row names
    name: str    # the series (extremes.SOURCES)
    kind: int    # layout.EXT_SRC_*
    row: int     # the row of its block
    op: int      # layout.IST_NONE (a mean item) | IST_GT | IST_GE | IST_LT | IST_LE
    c: float     # the threshold (0.0 for a mean item)
    stats: int   # mask of layout.IST_MEAN, or of IST_DUR | IST_DEG | IST_SPELL


def _parse_stats(text: str, what: str) -> int:
    m = 0
    for s in text.split("+"):
        key = s.strip().upper()
        if key not in L.IST_STATS:
            raise ValueError(f"interval_stats: unknown stat {s!r} in {what!r} (one of mean, dur, "
                             "deg, spell)")
        m |= L.IST_STATS[key]
    return m


def _check_item(it: Item) -> Item:
    if it.name not in SOURCES or SOURCES[it.name] != (it.kind, it.row):
        raise ValueError(f"interval_stats: unknown series {it.name!r} (an output flux, a forcing "
                         "row, a single-row state field or SMC1..4, SH2O1..4, STC1..4)")
    if not isinstance(it.label, str) or not _LABEL.match(it.label) or len(it.label) > MAX_LABEL:
        raise ValueError(f"interval_stats: label {it.label!r} is not [A-Z][A-Z0-9_]* of at most "
                         f"{MAX_LABEL} characters")
    if it.op == L.IST_NONE:
        if it.stats != L.IST_MEAN:
            raise ValueError(f"interval_stats: {it.label}: an item without a condition takes "
                             "mean, and only mean")
    elif it.op in _OP_NAMES:
        if it.stats <= 0 or it.stats & ~_COND:
            raise ValueError(f"interval_stats: {it.label}: a conditioned item takes dur, deg "
                             "and spell")
        if not math.isfinite(it.c):
            raise ValueError(f"interval_stats: {it.label}: the threshold must be finite")
    else:
        raise ValueError(f"interval_stats: {it.label}: operator {it.op} is none of gt, ge, lt, le")
    return it


def _parse_one(text: str) -> Item:
    body, colon, st = text.partition(":")
    if colon and not st.strip():
        raise ValueError(f"interval_stats: no stat after ':' in {text!r}")
    label, eq, rest = body.partition("=")
    if not eq:
        label, rest = None, body
    name, at, cond = rest.partition("@")
    name = name.strip()
    if name not in SOURCES:
        raise ValueError(f"interval_stats: unknown series {name!r} in {text!r} (an output flux, a "
                         "forcing row, a single-row state field or SMC1..4, SH2O1..4, STC1..4)")
    op, c = L.IST_NONE, 0.0
    if at:
        cond = cond.strip()
        if cond[:2].lower() not in L.IST_OPS:
            raise ValueError(f"interval_stats: unknown operator in {text!r} (one of gt, ge, lt, "
                             "le, then the threshold)")
        op = L.IST_OPS[cond[:2].lower()]
        try:
            c = float(cond[2:])
        except ValueError:
            raise ValueError(f"interval_stats: no threshold after the operator in {text!r}") \
                from None
        if label is None:
            raise ValueError(f"interval_stats: the conditioned item {text!r} needs a label "
                             "(LABEL=NAME@OPc)")
    stats = _parse_stats(st, text) if colon else (L.IST_DUR if at else L.IST_MEAN)
    return _check_item(Item(name if label is None else label.strip(), name, *SOURCES[name], op, c,
                            stats))


def parse(spec) -> list:
    """The items of "T2M,FROST=T2M@lt273.15:dur+spell", or of an iterable of
    such strings or Items.  ValueError for an unknown name, operator or stat,
    a stat of the wrong item type, a missing, malformed or duplicate label, a
    non-finite threshold, an empty selection and more than
    layout.IST_MAXITEMS items."""
    if isinstance(spec, str):
        parts = [s.strip() for s in spec.split(",") if s.strip()]
    else:
        parts = list(spec)
    out, seen = [], set()
    for p in parts:
        if isinstance(p, Item):
            it = _check_item(p)
        elif isinstance(p, str):
            it = _parse_one(p.strip())
        else:
            raise ValueError(f"interval_stats: {p!r} is neither a spec string nor an Item")
        if it.label in seen:
            raise ValueError(f"interval_stats: label {it.label!r} used twice")
        seen.add(it.label)
        out.append(it)
    if not out:
        raise ValueError("interval_stats: no item selected")
    if len(out) > L.IST_MAXITEMS:
        raise ValueError(f"interval_stats: {len(out)} items, at most {L.IST_MAXITEMS}")
    return out


def spec_string(items) -> str:
    """The canonical spec of `items` (what a restart carries): parse() of it
    gives them back.  Thresholds are printed with repr(float)."""
    out = []
    for it in items:
        s = it.name if it.label == it.name else f"{it.label}={it.name}"
        if it.op != L.IST_NONE:
            s = f"{it.label}={it.name}@{_OP_NAMES[it.op]}{float(it.c)!r}"
        out.append(s + ":" + "+".join(n.lower() for n, b in STAT_ORDER if it.stats & b))
    return ",".join(out)


def row_names(items) -> list:
    """<LABEL>_MEAN, _DUR, _DEG, _SPELL of the items' output rows, in
    nmp_intstats_output's row order."""
    return [f"{it.label}_{n}" for it in items for n, b in STAT_ORDER if it.stats & b]


def table(items) -> np.ndarray:
    """The (kind, row, operator, stat mask) words both entries take, int32 (nitems, 4)."""
    return np.array([[it.kind, it.row, it.op, it.stats] for it in items], np.int32).reshape(-1, 4)


def thresholds(items) -> np.ndarray:
    """The thresholds nmp_intstats_update takes, float64 (nitems,)."""
    return np.array([it.c for it in items], np.float64)


def has_diag(items) -> bool:
    return any(it.kind == L.EXT_SRC_DIAG for it in items)


def _check_table(tab, thr=None):
    tab = np.asarray(tab, np.int64).reshape(-1, 4)
    if not 1 <= tab.shape[0] <= L.IST_MAXITEMS:
        raise ValueError(f"interval_stats: {tab.shape[0]} items, 1..{L.IST_MAXITEMS} allowed")
    if thr is not None:
        thr = np.asarray(thr, np.float64).reshape(-1)
        if thr.shape[0] != tab.shape[0]:
            raise ValueError("interval_stats: one threshold per item")
    for i, (kind, row, op, m) in enumerate(tab):
        if int(kind) not in _NROWS:
            raise ValueError(f"interval_stats: series kind {kind} is none of the three")
        if not 0 <= row < _NROWS[int(kind)]:
            raise ValueError(f"interval_stats: row {row} outside its block of {_NROWS[int(kind)]}")
        if not L.IST_NONE <= op <= L.IST_LE:
            raise ValueError(f"interval_stats: operator {op} is none of the five")
        if m <= 0 or m & ~(L.IST_MEAN if op == L.IST_NONE else _COND):
            raise ValueError(f"interval_stats: stat mask {int(m):#x} is empty or does not fit the "
                             "item's type")
        if thr is not None and op != L.IST_NONE and not np.isfinite(thr[i]):
            raise ValueError("interval_stats: a threshold is not finite")
    return tab, thr


def update_host(acc: np.ndarray, cnt: np.ndarray, k: int, tab, thr, diag=None, forcing=None,
                state=None):
    """nmp_intstats_update in numpy, in place: acc (nitems, n) float64 and cnt
    (3*nitems, n) int32 after step k >= 1 of the interval, from the step's diag
    (16, n), forcing (12, n) and state (56, n) (None where no item names the
    block).  tab: table(); thr: thresholds().  One explicit double add per
    step, in step order."""
    tab, thr = _check_table(tab, thr)
    k = int(k)
    if k < 1:
        raise ValueError("interval_stats: k counts the interval's steps from 1")
    blocks = {L.EXT_SRC_DIAG: diag, L.EXT_SRC_FORCING: forcing, L.EXT_SRC_STATE: state}
    assert acc.shape[0] == tab.shape[0] and cnt.shape[0] == 3 * tab.shape[0]
    assert acc.dtype == np.float64 and cnt.dtype == np.int32
    with np.errstate(invalid="ignore", over="ignore"):
        for i, (kind, row, op, _) in enumerate(tab):
            block = blocks[int(kind)]
            if block is None:
                raise ValueError("interval_stats: a named item's block is missing")
            v = np.asarray(block)[row]
            a = np.zeros_like(acc[i]) if k == 1 else acc[i].copy()
            dv = v.astype(np.float64)
            if op == L.IST_NONE:
                acc[i] = a + dv
                continue
            ct = v.dtype.type(thr[i])
            h = {L.IST_GT: v > ct, L.IST_GE: v >= ct, L.IST_LT: v < ct, L.IST_LE: v <= ct}[int(op)]
            dc = np.float64(ct)
            d = dv - dc if op in (L.IST_GT, L.IST_GE) else dc - dv
            n, run, lng = cnt[3 * i], cnt[3 * i + 1], cnt[3 * i + 2]
            if k == 1:
                n[:], run[:], lng[:] = 0, 0, 0
            acc[i] = np.where(h, a + d, a)
            n[h] += 1
            run[h] += 1
            run[~h] = 0
            np.maximum(lng, run, out=lng)
    return acc, cnt


def output_host(acc: np.ndarray, cnt: np.ndarray, tab, k: int, dt: float, dtype) -> np.ndarray:
    """nmp_intstats_output in numpy: the output rows (sum of the masks' bits,
    n) of the engine's type `dtype` after the interval's k steps of dt
    seconds: MEAN (T)(acc / (double)k), DUR (T)((double)count * dt), DEG
    (T)(acc * dt), SPELL (T)((double)longest * dt)."""
    tab, _ = _check_table(tab)
    k, dt = int(k), float(dt)
    if k < 1:
        raise ValueError("interval_stats: k counts the interval's steps from 1")
    if not (np.isfinite(dt) and dt > 0.0):
        raise ValueError("interval_stats: dt must be finite and positive")
    assert acc.shape[0] == tab.shape[0] and cnt.shape[0] == 3 * tab.shape[0]
    assert acc.dtype == np.float64 and cnt.dtype == np.int32
    rows, dt64 = [], np.float64(dt)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        for i, m in enumerate(tab[:, 3]):
            if m & L.IST_MEAN:
                rows.append((acc[i] / np.float64(k)).astype(dtype))
            if m & L.IST_DUR:
                rows.append((cnt[3 * i].astype(np.float64) * dt64).astype(dtype))
            if m & L.IST_DEG:
                rows.append((acc[i] * dt64).astype(dtype))
            if m & L.IST_SPELL:
                rows.append((cnt[3 * i + 2].astype(np.float64) * dt64).astype(dtype))
    return np.stack(rows)
