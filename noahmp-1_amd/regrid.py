"""Forcing on its own grid: regrid plans (nmp_ldasin_regrid) and the elevation
downscaling (nmp_ldasin_downscale), with their numpy restatements.

A `RegridPlan` gives every engine column four source entries -- a source grid
point and a double weight each -- in the layout the kernel reads
(include/noahmp_engine.h: corner and weight, (4, n), entry-major).  The plan
and the values fix the result's bits: `apply_host` restates the kernel
operation for operation, so a host-built block and a device-formed one are the
same bytes.  `RegridPlan.bilinear` builds the plan of a rectilinear source
grid (1-D latitude and longitude axes, e.g. a reanalysis grid).
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from .layout import LDASIN, NLDASIN

QNAN_BITS = np.uint32(0x7FC00000)
# nmp_ldasin_downscale's constants: the reference's GRAV and RAIR
G, RD = 9.80616, 287.04


def nearest_mask(nearest=()) -> int:
    """nmp_ldasin_regrid's nearest_mask from LDASIN variable names (or row
    indices): bit v set = variable v takes its nearest source entry."""
    m = 0
    for v in nearest:
        i = LDASIN.index(v) if isinstance(v, str) else int(v)
        if not 0 <= i < NLDASIN - 1:
            raise ValueError(f"nearest: {v!r} is not one of {LDASIN[:-1]}")
        m |= 1 << i
    return m


@dataclass
class RegridPlan:
    ncol: int               # columns the plan serves
    npts: int               # points of the source grid
    corner: np.ndarray      # (4, ncol) int32 source point of each entry, -1 = masked
    weight: np.ndarray      # (4, ncol) float64
    dev: dict | None = None  # corner and weight as tensors on `device` (to())
    device: object = None

    @classmethod
    def bilinear(cls, src_lat_deg, src_lon_deg, col_lat_deg, col_lon_deg,
                 src_mask=None) -> "RegridPlan":
        """The bilinear plan of a rectilinear source grid for columns at
        (col_lat_deg, col_lon_deg).  src_lat_deg (ny,) ascends or descends,
        src_lon_deg (nx,) ascends; column longitudes are taken modulo 360
        relative to the source's first longitude, and a source whose nx * dlon
        is 360 within 1e-6 degrees wraps from its last column to its first.
        Entries are the cell's corners (j0,i0), (j0,i0+1), (j0+1,i0),
        (j0+1,i0+1) in the source's own index order with weights
        (1-fy)(1-fx), (1-fy)fx, fy(1-fx), fy fx (one double product each);
        src_mask (ny, nx), true = valid: a masked corner gets corner -1 and
        weight 0; the others are divided by their double sum, added in entry
        order.  A column outside the source's hull, or left without a valid
        corner of positive weight, raises ValueError."""
        lat = np.asarray(src_lat_deg, np.float64)
        lon = np.asarray(src_lon_deg, np.float64)
        y = np.asarray(col_lat_deg, np.float64).reshape(-1)
        xl = np.asarray(col_lon_deg, np.float64).reshape(-1)
        if lat.ndim != 1 or lon.ndim != 1 or lat.size < 2 or lon.size < 2:
            raise ValueError("the source grid needs 1-D latitude and longitude axes of >= 2 points")
        if y.shape != xl.shape:
            raise ValueError("column latitudes and longitudes differ in shape")
        ny, nx = int(lat.size), int(lon.size)
        if ny * nx >= 2**29:
            raise ValueError("a regrid plan indexes fewer than 2^29 source points")
        dlat = np.diff(lat)
        if not ((dlat > 0).all() or (dlat < 0).all()) or not (np.diff(lon) > 0).all():
            raise ValueError("source latitudes must be strictly monotonic, longitudes ascending")
        mask = np.ones((ny, nx), bool) if src_mask is None else np.asarray(src_mask, bool)
        if mask.shape != (ny, nx):
            raise ValueError(f"src_mask must be ({ny}, {nx}), not {mask.shape}")
        # latitude: the cell j0 of the source's own order that holds y
        asc = lat[1] > lat[0]
        la = lat if asc else lat[::-1]
        ja = np.clip(np.searchsorted(la, y, side="right") - 1, 0, ny - 2)
        j0 = ja if asc else ny - 2 - ja
        out = (y < la[0]) | (y > la[-1]) | ~np.isfinite(y)
        with np.errstate(all="ignore"):
            fy = (y - lat[j0]) / (lat[j0 + 1] - lat[j0])
        # longitude: degrees east of the source's first column, in [0, 360)
        xs = lon - lon[0]
        x = np.mod(xl - lon[0], 360.0)
        wraps = abs(nx * (xs[-1] / (nx - 1)) - 360.0) <= 1e-6
        i0 = np.clip(np.searchsorted(xs, x, side="right") - 1, 0, nx - 2)
        i1 = i0 + 1
        x1 = xs[i1]
        if wraps:
            last = x >= xs[-1]
            i0 = np.where(last, nx - 1, i0)
            i1 = np.where(last, 0, i1)
            x1 = np.where(last, 360.0, x1)
        else:
            out |= x > xs[-1]
        out |= ~np.isfinite(x)
        with np.errstate(all="ignore"):
            fx = (x - xs[i0]) / (x1 - xs[i0])
        j1 = j0 + 1
        jj = np.stack([j0, j0, j1, j1])
        ii = np.stack([i0, i1, i0, i1])
        w = np.stack([(1.0 - fy) * (1.0 - fx), (1.0 - fy) * fx, fy * (1.0 - fx), fy * fx])
        valid = mask[jj, ii]
        corner = np.where(valid, jj * nx + ii, -1).astype(np.int32)
        w = np.where(valid, w, 0.0)
        s = np.zeros(y.size, np.float64)
        for k in range(4):
            s = s + w[k]
        bad = out | ~(s > 0.0)
        if bad.any():
            raise ValueError(f"{int(bad.sum())} of {y.size} columns lie outside the source grid "
                             f"({int(out.sum())}) or have no valid source point "
                             f"({int((bad & ~out).sum())})")
        return cls(int(y.size), ny * nx, np.ascontiguousarray(corner),
                   np.ascontiguousarray(w / s))

    # ---- numpy restatements -------------------------------------------------------
    def _bad(self) -> np.ndarray:
        """Columns nmp_ldasin_regrid fills with NaN: no valid entry, or a
        corner outside the source grid."""
        return ~(self.corner >= 0).any(0) | (self.corner >= self.npts).any(0)

    def _safe(self) -> np.ndarray:
        return np.where((self.corner >= 0) & (self.corner < self.npts), self.corner, 0)

    def apply_host(self, grids: np.ndarray, nearest=()) -> np.ndarray:
        """nmp_ldasin_regrid in numpy, operation for operation: grids is
        (nvar, npts) fp32 of either byte order (ncio grid_raw's (8, npts)) or
        one row (npts,); returns (nvar, ncol) or (ncol,) float32.  nearest:
        the rows that take their nearest entry -- LDASIN names or row indices
        (for one row: anything true)."""
        g = np.asarray(grids)
        one = g.ndim == 1
        if one:
            g = g[None]
            near = {0} if nearest else set()
        else:
            near = {LDASIN.index(v) if isinstance(v, str) else int(v) for v in nearest}
        if g.ndim != 2 or g.shape[1] != self.npts or g.dtype.kind != "f" or g.dtype.itemsize != 4:
            raise ValueError(f"grids must be fp32 (nvar, {self.npts}) or ({self.npts},), not "
                             f"{g.dtype} {g.shape}")
        bits = np.ascontiguousarray(g.astype(g.dtype.newbyteorder("="), copy=False)).view(np.uint32)
        valid, safe = self.corner >= 0, self._safe()
        out = np.empty((g.shape[0], self.ncol), np.uint32)
        # the nearest entry: largest weight among the valid ones, ties to the lowest k
        ks = np.full(self.ncol, -1)
        wbest = np.zeros(self.ncol, np.float64)
        for k in range(4):
            take = valid[k] & ((ks < 0) | (self.weight[k] > wbest))
            ks = np.where(take, k, ks)
            wbest = np.where(take, self.weight[k], wbest)
        pick = safe[np.maximum(ks, 0), np.arange(self.ncol)]
        with np.errstate(all="ignore"):
            for v in range(g.shape[0]):
                if v in near:
                    out[v] = bits[v, pick]
                    continue
                x = np.zeros(self.ncol, np.float64)
                for k in range(4):
                    val = bits[v, safe[k]].view(np.float32).astype(np.float64)
                    x = np.where(valid[k], x + val * self.weight[k], x)  # a masked entry leaves x
                out[v] = x.astype(np.float32).view(np.uint32)
        out[:, self._bad()] = QNAN_BITS
        out = out.view(np.float32)
        return out[0] if one else out

    def interp_scalar(self, field) -> np.ndarray:
        """A double field on the source grid (e.g. its elevation) at the
        columns, by the plan's entries in double: x = 0; x = x + f_k * w_k for
        the valid entries in order.  NaN where the kernel gives NaN rows."""
        f = np.asarray(field, np.float64).reshape(-1)
        if f.size != self.npts:
            raise ValueError(f"field has {f.size} points, the source grid {self.npts}")
        valid, safe = self.corner >= 0, self._safe()
        x = np.zeros(self.ncol, np.float64)
        with np.errstate(all="ignore"):
            for k in range(4):
                x = np.where(valid[k], x + f[safe[k]] * self.weight[k], x)
        x[self._bad()] = np.nan
        return x

    def to(self, device) -> "RegridPlan":
        """The plan with corner and weight also resident on `device` (what
        Engine.ldasin_regrid takes)."""
        import torch
        dev = torch.device(device)
        if dev.type == "cuda" and dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        t = {k: torch.as_tensor(getattr(self, k), device=dev).contiguous()
             for k in ("corner", "weight")}
        return RegridPlan(self.ncol, self.npts, self.corner, self.weight, t, dev)


def _magnus_arg(t):
    return (17.67 * (t - 273.15)) / (t - 29.65)


def downscale_host(block: np.ndarray, dz, lapse: float) -> np.ndarray:
    """nmp_ldasin_downscale in numpy (a new block; numpy's double exp, which
    may differ from the device's by one ulp): rows T2D, Q2D, PSFC and LWDOWN of
    the fp32 LDASIN block corrected for the elevation difference dz (model
    minus source, m; taken as fp32) with the lapse rate `lapse` (K/m)."""
    b = np.array(block, np.float32, copy=True)
    iT, iQ, iP, iL = (LDASIN.index(v) for v in ("T2D", "Q2D", "PSFC", "LWDOWN"))
    lapse = float(lapse)
    d = np.asarray(dz, np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        t0, q0 = b[iT].astype(np.float64), b[iQ].astype(np.float64)
        p0, lw0 = b[iP].astype(np.float64), b[iL].astype(np.float64)
        t1 = t0 - lapse * d
        tm = 0.5 * (t0 + t1)
        p1 = p0 * np.exp(-(G * d) / (RD * tm))
        q1 = (q0 * np.exp(_magnus_arg(t1) - _magnus_arg(t0))) * (p0 / p1)
        r = t1 / t0
        lw1 = lw0 * ((r * r) * (r * r))
    b[iT], b[iQ], b[iP], b[iL] = (a.astype(np.float32) for a in (t1, q1, p1, lw1))
    return b
