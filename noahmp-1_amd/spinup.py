"""Spin-up (nmp_state_drift / nmp_drift_reduce): the tracked values of the land
state, their drift between two passes over the forcing period and its
reduction, restated in numpy, and the records a spin-up keeps.

A spin-up (driver.OfflineDriver.spinup) runs the forcing period over and over
from the state the last pass left until the state at the end of a pass stops
changing.  The change is measured on the device: 13 tracked values per column
(layout.TRACKED, NMP_K_* of include/noahmp_engine.h), 7 drift groups
(layout.DRIFT_GROUPS, NMP_G_*) against the snapshot of the pass before, and per
group the largest drift and its column, the count of columns over the
tolerance and the weighted mean.

`tracked_host` and `drift_host` restate csrc/drift.hip's per-column kernel
operation for operation at the engine's dtype, `reduce_host` the reduction's
fixed tree: every operation is one IEEE operation in the header's order, so
their results equal the kernels' bit for bit in fp32 and fp64.
"""
from __future__ import annotations

import math
from dataclasses import asdict, dataclass, field

import numpy as np

from . import layout as L

GROUPS = list(L.DRIFT_GROUPS)
_WAVE = 64
_PER_LANE = L.DRIFT_CHUNK // _WAVE
QNAN_BITS = 0x7ff8000000000000


def parse_tol(spec) -> np.ndarray:
    """The 7 tolerances (float64, in layout.DRIFT_GROUPS order) of
    "SOIL_M=0.001,SOIL_T=0.01", a dict of them, or 7 numbers; a group that is
    not named gets +inf (always converged).  ValueError for an unknown group,
    a group named twice, a negative value, a NaN or something that is no
    number."""
    tol = np.full(L.NDRIFT, np.inf, np.float64)
    if isinstance(spec, str):
        items = []
        for part in spec.split(","):
            if not part.strip():
                continue
            name, eq, val = part.partition("=")
            if not eq:
                raise ValueError(f"spin-up tolerance: {part.strip()!r} is not GROUP=VALUE")
            items.append((name.strip(), val.strip()))
        if not items:
            raise ValueError("spin-up tolerance: no group named")
    elif isinstance(spec, dict):
        items = list(spec.items())
    else:
        vals = list(spec)
        if len(vals) != L.NDRIFT:
            raise ValueError(f"spin-up tolerance: {L.NDRIFT} values, not {len(vals)}")
        items = list(zip(GROUPS, vals))
    seen = set()
    for name, val in items:
        if name not in GROUPS:
            raise ValueError(f"spin-up tolerance: unknown group {name!r} (one of "
                             f"{', '.join(GROUPS)})")
        if name in seen:
            raise ValueError(f"spin-up tolerance: group {name} named twice")
        seen.add(name)
        try:
            v = float(val)
        except (TypeError, ValueError):
            raise ValueError(f"spin-up tolerance: {name}={val!r} is not a number") from None
        if math.isnan(v) or v < 0.0:
            raise ValueError(f"spin-up tolerance: {name}={val} must be a number >= 0")
        tol[GROUPS.index(name)] = v
    return tol


def algorithmic_bytes(precision: int) -> dict:
    """Bytes per column the two kernels have to move at engine precision 4 or
    8 (tools/io_kernels_bench.py).  state_drift: the 24 state rows the header
    names, ISNOW and IST, the snapshot read and written (13 rows each) and the
    7 drift rows written; drift_reduce: the 7 drift rows and the weight."""
    p = int(precision)
    return {"state_drift": (24 + 2 * L.NTRACKED + L.NDRIFT) * p + 8,
            "state_drift_snapshot": (24 + L.NTRACKED) * p + 8,
            "drift_reduce": L.NDRIFT * p + 8}


# ---- the per-column kernel -----------------------------------------------------------
def tracked_host(state, isnow, static_i, dtype=None) -> np.ndarray:
    """The (13, n) tracked values nmp_state_drift forms from state (56, n),
    isnow (n,) and static_i (6, n), in `dtype` (default: state's)."""
    T = np.dtype(dtype if dtype is not None else np.asarray(state).dtype).type
    st = np.asarray(state).astype(T, copy=False)
    isn = np.asarray(isnow, np.int32)
    one = lambda name, k=0: st[L.STATE_OFF[name][0] + k]  # noqa: E731
    out = np.empty((L.NTRACKED, isn.shape[0]), T)
    with np.errstate(all="ignore"):
        for i in range(L.NSOIL):
            out[L.TRACKED["SMC"] + i] = one("SMC", i)
            out[L.TRACKED["STC"] + i] = one("STC", L.NSNOW + i)
        for name in ("SNEQV", "WA", "ZWT"):
            out[L.TRACKED[name]] = one(name)
        dz = L.soil_thickness_host([one("ZSNSO", 2 + i) for i in range(L.NSOIL + 1)], isn)
        w = L.water_storage_host(one("CANLIQ"), one("CANICE"), one("SNEQV"), one("WA"),
                                 [one("SMC", i) for i in range(L.NSOIL)], dz)
        ist = np.asarray(static_i)[L.STATIC_I.index("IST")]
        out[L.TRACKED["TWS"]] = np.where(ist == 1, w, T(0))
        p = [one(n) for n in L.CARBON_POOLS]
        out[L.TRACKED["CTOT"]] = ((((p[0] + p[1]) + p[2]) + p[3]) + p[4]) + p[5]
    return out


def drift_host(now: np.ndarray, snap: np.ndarray) -> np.ndarray:
    """The (7, n) drift rows of the tracked values `now` against `snap` (both
    (13, n), the same dtype), as nmp_state_drift writes them."""
    now, snap = np.asarray(now), np.asarray(snap)
    assert now.dtype == snap.dtype and now.shape == snap.shape and now.shape[0] == L.NTRACKED
    out = np.empty((L.NDRIFT, now.shape[1]), now.dtype)
    with np.errstate(all="ignore"):
        d = np.abs(now - snap)
        for g, key in (("SOIL_M", "SMC"), ("SOIL_T", "STC")):
            k = L.TRACKED[key]
            m = d[k]
            for i in range(1, L.NSOIL):
                x = d[k + i]
                m = np.where((x > m) | (x != x), x, m)
            out[GROUPS.index(g)] = m
        for g, key in (("SNEQV", "SNEQV"), ("WA", "WA"), ("ZWT", "ZWT"), ("TWS", "TWS"),
                       ("CARBON", "CTOT")):
            out[GROUPS.index(g)] = d[L.TRACKED[key]]
    return out


# ---- the reduction -------------------------------------------------------------------
@dataclass
class DriftResult:
    """nmp_drift_reduce's numbers, per drift group: the largest drift (float64,
    the quiet NaN where a column's drift is NaN), its column (int64, -1 where
    no column counts), the weighted sum by the fixed tree, the count of
    columns over the tolerance, and the weights' sum `wtot`."""
    max: np.ndarray
    arg: np.ndarray
    wsum: np.ndarray
    count: np.ndarray
    wtot: float

    @property
    def mean(self) -> np.ndarray:
        """wsum / wtot (NaN where no column counts)."""
        with np.errstate(all="ignore"):
            return self.wsum / np.float64(self.wtot)

    @property
    def converged(self) -> bool:
        return not self.count.any()


def _tree(x: np.ndarray, use: np.ndarray) -> np.ndarray:
    """The fixed tree over the last axis of x (..., n): `use` (n,) marks the
    columns that take part; x holds the (already rounded) terms."""
    n = x.shape[-1]
    nchunk = -(-n // L.DRIFT_CHUNK)
    pad = nchunk * L.DRIFT_CHUNK - n
    x = np.concatenate([x, np.zeros(x.shape[:-1] + (pad,), np.float64)], -1)
    use = np.concatenate([use, np.zeros(pad, bool)])
    x = x.reshape(x.shape[:-1] + (nchunk, _PER_LANE, _WAVE))
    use = use.reshape(nchunk, _PER_LANE, _WAVE)
    lane = np.zeros(x.shape[:-3] + (nchunk, _WAVE), np.float64)
    with np.errstate(all="ignore"):
        for j in range(_PER_LANE):
            lane = np.where(use[:, j], lane + x[..., j, :], lane)  # a column left out leaves x
        for s in (32, 16, 8, 4, 2, 1):
            lane = lane[..., :s] + lane[..., s:2 * s]
        partial = lane[..., 0]
        total = np.zeros(x.shape[:-3], np.float64)
        for k in range(nchunk):
            total = total + partial[..., k]
    return total


def reduce_host(drift, tol, weight=None) -> DriftResult:
    """nmp_drift_reduce in numpy: drift (7, n) float32 or float64, tol 7
    doubles, weight (n,) doubles or None (= 1); a column of weight exactly 0 is
    skipped in everything."""
    d = np.asarray(drift)
    assert d.ndim == 2 and d.shape[0] == L.NDRIFT, d.shape
    n = d.shape[1]
    tol = np.asarray(tol, np.float64)
    assert tol.shape == (L.NDRIFT,)
    w = np.ones(n, np.float64) if weight is None else np.asarray(weight, np.float64)
    assert w.shape == (n,)
    use = w != 0.0
    d64 = d.astype(np.float64)                      # exact
    mx = np.zeros(L.NDRIFT, np.float64)
    arg = np.full(L.NDRIFT, -1, np.int64)
    count = np.zeros(L.NDRIFT, np.int64)
    idx = np.flatnonzero(use)
    with np.errstate(all="ignore"):
        for g in range(L.NDRIFT):
            v = d64[g, idx]
            count[g] = int((~(v <= tol[g])).sum())
            if not idx.size:
                continue
            nan = np.isnan(v)
            if nan.any():
                mx[g] = np.array([QNAN_BITS], np.uint64).view(np.float64)[0]
                arg[g] = idx[np.flatnonzero(nan)[0]]
            else:
                m = v.max()
                first = np.flatnonzero(v == m)[0]
                mx[g], arg[g] = v[first], idx[first]
        wsum = _tree(d64 * w, use)
        wtot = _tree(w[None], use)[0]
    return DriftResult(mx, arg, wsum, count, float(wtot))


# ---- what a spin-up keeps ------------------------------------------------------------
@dataclass
class SpinupRecord:
    """One spin-up loop's convergence numbers, per drift group in
    layout.DRIFT_GROUPS order: the largest drift, the (global) column that holds
    it, the weighted mean drift, the count of columns over the tolerance, and
    the tolerance (inf where none was given)."""
    loop: int
    max: list = field(default_factory=list)
    arg: list = field(default_factory=list)
    mean: list = field(default_factory=list)
    count: list = field(default_factory=list)
    tol: list = field(default_factory=list)

    @property
    def converged(self) -> bool:
        return not any(self.count)

    def as_json(self) -> dict:
        """Plain numbers; a value JSON cannot hold (NaN, inf) becomes its name."""
        num = lambda v: v if math.isfinite(v) else repr(v)  # noqa: E731
        d = asdict(self)
        for k in ("max", "mean", "tol"):
            d[k] = [num(float(v)) for v in d[k]]
        return d
