"""Region plans of the region-aggregated output (nmp_region_reduce).

A `RegionPlan` lists, region after region, the columns of each region with
their weights in the layout the kernel reads (include/noahmp_engine.h: entries
padded to chunks of 256 per region, a CSR of chunks per region), and fixes the
summation tree with it: the sums depend on the plan and the values, never on
how the kernel was launched.  `reduce_host` restates that tree in numpy for a
user without a device result at hand.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

from .layout import REGION_CHUNK

_WAVE = 64
_PER_LANE = REGION_CHUNK // _WAVE


@dataclass
class RegionPlan:
    ncol: int                  # columns of the block the plan indexes
    region_id: np.ndarray      # (nreg,) int64, sorted unique ids that hold a column
    ncolumns: np.ndarray       # (nreg,) int64 columns per region
    entry_col: np.ndarray      # (nchunk * 256,) int32, -1 = pad
    entry_w: np.ndarray        # (nchunk * 256,) float64, 0 = pad
    region_chunk0: np.ndarray  # (nreg + 1,) int64 CSR of chunks per region
    wsum: np.ndarray           # (nreg,) float64: the tree's sum of the weights
    dev: dict | None = None    # the four arrays as tensors on `device` (to())
    device: object = None
    _partial: dict = field(default_factory=dict, repr=False)

    @property
    def nreg(self) -> int:
        return int(self.region_id.size)

    @property
    def nchunk(self) -> int:
        return int(self.region_chunk0[-1])

    @classmethod
    def from_ids(cls, region_id, weight=None) -> "RegionPlan":
        """region_id: (n,) ints, one per column of the block in its order; a
        column with id < 0 is in no region.  weight: (n,) doubles (default 1).
        Regions are ordered by id; within a region the columns keep their
        ascending order."""
        ids = np.asarray(region_id)
        if ids.ndim != 1 or ids.dtype.kind not in "iu":
            raise ValueError("region_id must be a one-dimensional integer array")
        ids = ids.astype(np.int64)
        n = int(ids.size)
        if n >= 2**31:
            raise ValueError("a region plan indexes columns in 32 bits")
        w = np.ones(n, np.float64) if weight is None else np.asarray(weight, np.float64)
        if w.shape != (n,):
            raise ValueError(f"weight must have shape ({n},), not {w.shape}")
        cols = np.flatnonzero(ids >= 0)
        cols = cols[np.argsort(ids[cols], kind="stable")]
        uniq, counts = np.unique(ids[cols], return_counts=True)
        nch = -(-counts // REGION_CHUNK)
        chunk0 = np.concatenate([[0], np.cumsum(nch)]).astype(np.int64)
        # entry of the i-th column of region r: the region's first entry + i
        first = np.concatenate([[0], np.cumsum(counts)])[:-1]
        dest = np.repeat(chunk0[:-1] * REGION_CHUNK - first, counts) + np.arange(cols.size)
        entry_col = np.full(int(chunk0[-1]) * REGION_CHUNK, -1, np.int32)
        entry_w = np.zeros(entry_col.size, np.float64)
        entry_col[dest] = cols
        entry_w[dest] = w[cols]
        plan = cls(n, uniq.astype(np.int64), counts.astype(np.int64), entry_col, entry_w, chunk0,
                   np.zeros(uniq.size, np.float64))
        # the divisor of the means by the tree itself: a field of ones then has
        # mean exactly sum / wsum of equal numbers
        plan.wsum = plan.reduce_host(np.ones((1, n), np.float64))[0][0]
        return plan

    def reduce_host(self, fields: np.ndarray):
        """(sums, means), each (nfield, nreg) float64, of the (nfield, ncol)
        block `fields` (float32 or float64): nmp_region_reduce's tree in numpy,
        operation for operation."""
        fields = np.asarray(fields)
        if fields.ndim != 2 or fields.shape[1] != self.ncol:
            raise ValueError(f"fields must be (nfield, {self.ncol}), not {fields.shape}")
        nf, nchunk, nreg = fields.shape[0], self.nchunk, self.nreg
        ec = self.entry_col.reshape(nchunk, _PER_LANE, _WAVE)
        ew = self.entry_w.reshape(nchunk, _PER_LANE, _WAVE)
        x = np.zeros((nf, nchunk, _WAVE), np.float64)
        with np.errstate(all="ignore"):
            for j in range(_PER_LANE):
                real = ec[:, j] >= 0
                v = fields[:, np.where(real, ec[:, j], 0)].astype(np.float64)
                x = np.where(real, x + v * ew[:, j], x)  # a pad leaves x as it is
            for s in (32, 16, 8, 4, 2, 1):
                x = x[..., :s] + x[..., s:2 * s]
            partial = x[..., 0]
            sums = np.zeros((nf, nreg), np.float64)
            k0, nch = self.region_chunk0[:-1], np.diff(self.region_chunk0)
            for i in range(int(nch.max()) if nreg else 0):
                m = nch > i
                sums[:, m] = sums[:, m] + partial[:, k0[m] + i]
            means = sums / self.wsum
        return sums, means

    def to(self, device) -> "RegionPlan":
        """The plan with its arrays also resident on `device` (what
        Engine.region_reduce takes)."""
        import torch
        dev = torch.device(device)
        if dev.type == "cuda" and dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        t = {k: torch.as_tensor(getattr(self, k), device=dev).contiguous()
             for k in ("entry_col", "entry_w", "region_chunk0", "wsum")}
        return RegionPlan(self.ncol, self.region_id, self.ncolumns, self.entry_col, self.entry_w,
                          self.region_chunk0, self.wsum, t, dev)

    def partial(self, nfield: int):
        """Pass 1's scratch for `nfield` fields on the plan's device, kept with
        the plan: calls that share a plan must be ordered by their streams."""
        import torch
        p = self._partial.get(nfield)
        if p is None:
            p = self._partial[nfield] = torch.empty((nfield, max(self.nchunk, 1)),
                                                    dtype=torch.float64, device=self.device)
        return p


def area_weights(lat_rad: np.ndarray) -> np.ndarray:
    """cos(latitude) in double: the relative area of a regular lat-lon cell."""
    return np.cos(np.asarray(lat_rad, np.float64))


def plan_from_args(regions, region_weights, total: int, lat_rad=None) -> RegionPlan:
    """The plan of the offline driver's `regions` and `region_weights`
    arguments (driver.OfflineDriver) over the run's `total` columns.
    lat_rad: the columns' latitudes where the caller holds all of them (a
    single rank), what region_weights="area" weighs by; None under a process
    group, where "area" needs the global columns' weights as an array."""
    ids = np.asarray(regions)
    if ids.shape != (total,):
        raise ValueError(f"regions must hold one id per column ({total}), not {ids.shape}")
    if isinstance(region_weights, str):
        if region_weights == "equal":
            w = np.ones(total, np.float64)
        elif region_weights == "area" and lat_rad is not None:
            w = area_weights(lat_rad)
        elif region_weights == "area":
            raise ValueError("region_weights='area' under a process group needs the "
                             "global columns' weights as an array")
        else:
            raise ValueError("region_weights must be 'area', 'equal' or an array, not "
                             f"{region_weights!r}")
    else:
        w = np.asarray(region_weights, np.float64)
    return RegionPlan.from_ids(ids, w)
