"""Forcing on its own grid, host side (no GPU): the bilinear plan's geometry,
apply_host against the analytic value of a linear field (independent of the
kernel's twin) and against the operation order restated here from
include/noahmp_engine.h alone, masked corners, nearest entries, the elevation
downscaling's numpy form, the forcing-grid file and the reader on a source
grid, and the two new C entries' declaration, export and binding."""
import datetime
import re
import subprocess

import numpy as np
import pytest

from noahmp_amd import layout as L, lib as _lib, ncio
from noahmp_amd.regrid import RegridPlan, downscale_host, nearest_mask
from test_abi_host import _header

T0 = datetime.datetime(2000, 1, 1)
SRC_LAT = np.array([30.0, 31.0, 32.5, 33.0, 35.0])            # 5 x 7, uneven spacing
SRC_LON = np.array([-120.0, -119.0, -118.0, -116.5, -115.0, -114.0, -112.0])


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def columns40(seed=0):
    """40 columns inside the 5 x 7 source's hull: source nodes (corners of the
    hull included), points on cell edges, a longitude given as lon + 360, and
    random interior points."""
    rng = np.random.default_rng(seed)
    lat = list(rng.uniform(30.0, 35.0, 28))
    lon = list(rng.uniform(-120.0, -112.0, 28))
    for j, i in ((0, 0), (4, 6), (2, 3), (0, 6), (4, 0), (1, 5)):  # nodes
        lat.append(SRC_LAT[j]), lon.append(SRC_LON[i])
    for la, lo in ((31.0, -117.25), (34.0, -116.5), (32.5, -112.0), (30.0, -119.5)):  # edges
        lat.append(la), lon.append(lo)
    lat += [33.5, 30.25]
    lon += [-118.5 + 360.0, -113.0 + 360.0]
    return np.array(lat), np.array(lon)


def restated(plan, grids, near=()):
    """nmp_ldasin_regrid as the header words it, column by column in Python
    floats (IEEE double), fp32 through numpy scalars."""
    out = np.empty((grids.shape[0], plan.ncol), np.uint32)
    for c in range(plan.ncol):
        p, w = plan.corner[:, c], plan.weight[:, c]
        if not (p >= 0).any() or (p >= plan.npts).any():
            out[:, c] = 0x7FC00000
            continue
        ks = -1
        for k in range(4):
            if p[k] >= 0 and (ks < 0 or w[k] > w[ks]):
                ks = k
        for v in range(grids.shape[0]):
            if v in near:
                out[v, c] = bits(grids[v])[p[ks]]
                continue
            x = 0.0
            for k in range(4):
                if p[k] >= 0:
                    with np.errstate(all="ignore"):
                        x = x + float(np.float64(grids[v, p[k]]) * np.float64(w[k]))
            out[v, c] = np.float32(x).view(np.uint32)
    return out


# ---- plan geometry -------------------------------------------------------------------
@pytest.mark.parametrize("descending", [False, True])
def test_plan_geometry(descending):
    lat, lon = columns40()
    slat = SRC_LAT[::-1] if descending else SRC_LAT
    plan = RegridPlan.bilinear(slat, SRC_LON, lat, lon)
    assert plan.ncol == 40 and plan.npts == 35
    assert plan.corner.shape == (4, 40) and plan.corner.dtype == np.int32
    assert plan.weight.shape == (4, 40) and plan.weight.dtype == np.float64
    assert (plan.weight >= 0).all()
    s = plan.weight[0] + plan.weight[1] + plan.weight[2] + plan.weight[3]
    assert (np.abs(s - 1.0) <= 2 * np.spacing(1.0)).all()
    # entries are (j0,i0), (j0,i0+1), (j0+1,i0), (j0+1,i0+1) of the source's own order
    j, i = plan.corner // 7, plan.corner % 7
    assert (j[1] == j[0]).all() and (j[2] == j[0] + 1).all() and (j[3] == j[2]).all()
    assert (i[1] == i[0] + 1).all() and (i[2] == i[0]).all() and (i[3] == i[1]).all()
    # every column lies in its cell
    lo, hi = np.minimum(slat[j[0]], slat[j[2]]), np.maximum(slat[j[0]], slat[j[2]])
    assert ((lat >= lo) & (lat <= hi)).all()
    x = np.mod(lon - SRC_LON[0], 360.0) + SRC_LON[0]
    assert ((x >= SRC_LON[i[0]]) & (x <= SRC_LON[i[1]])).all()
    # a column on a node: one weight equal to 1, on that node
    for c in range(28, 34):
        k = int(np.argmax(plan.weight[:, c]))
        assert plan.weight[k, c] == 1.0 and (np.delete(plan.weight[:, c], k) == 0).all()
        assert slat[j[k, c]] == lat[c] and SRC_LON[i[k, c]] == lon[c]
    # a longitude given as lon + 360 lands where lon does
    same = RegridPlan.bilinear(slat, SRC_LON, lat[38:], lon[38:] - 360.0)
    assert np.array_equal(same.corner, plan.corner[:, 38:])
    assert np.array_equal(same.weight, plan.weight[:, 38:])


def test_plan_rejects_columns_without_source():
    lat, lon = columns40()
    with pytest.raises(ValueError, match=r"\b2 of 42 columns"):
        RegridPlan.bilinear(SRC_LAT, SRC_LON, np.append(lat, [35.5, 31.0]),
                            np.append(lon, [-115.0, -111.0]))
    # all four corners masked
    mask = np.ones((5, 7), bool)
    mask[0:2, 0:2] = False
    with pytest.raises(ValueError, match=r"\b1 of 2 columns"):
        RegridPlan.bilinear(SRC_LAT, SRC_LON, [30.5, 34.0], [-119.5, -113.0], mask)
    with pytest.raises(ValueError):
        RegridPlan.bilinear(SRC_LAT, SRC_LON[::-1], [31.0], [-115.0])


def test_global_source_wraps_across_the_date_line():
    slat = np.linspace(-78.75, 78.75, 8)
    slon = -180.0 + 22.5 * np.arange(16)        # 16 x 22.5 = 360: periodic
    lat = np.array([10.0, -33.0, 0.0])
    lon = np.array([170.0, 179.0, -180.0 + 360.0])  # 157.5 -> -180 is the wrapping cell
    plan = RegridPlan.bilinear(slat, slon, lat, lon)
    i = plan.corner % 16
    assert (i[0, :2] == 15).all() and (i[1, :2] == 0).all()
    assert i[0, 2] == 0
    # a field linear in the longitude's sine and cosine interpolates across the seam
    field = np.cos(np.radians(slon))[None, :] + 0.0 * slat[:, None]
    got = plan.interp_scalar(field)
    fx = (lon[:2] - 157.5) / 22.5
    want = (1 - fx) * np.cos(np.radians(157.5)) + fx * np.cos(np.radians(-180.0))
    assert np.allclose(got[:2], want, rtol=0, atol=1e-14)
    # a regional source does not wrap
    with pytest.raises(ValueError):
        RegridPlan.bilinear(slat, slon[:8], [0.0], [0.0])


# ---- apply_host ---------------------------------------------------------------------
def test_apply_host_reproduces_a_linear_field():
    """Independent of the kernel's twin: bilinear weights reproduce a field
    linear in latitude and longitude.  The stored corners are fp32 (<= 0.5 ulp
    each, through a convex combination), the result is rounded once to fp32
    (0.5 ulp) and the double arithmetic adds ~1e-16 relative: 2 fp32 ulps of
    the largest corner magnitude bound the difference."""
    lat, lon = columns40(seed=5)
    a, b, c = 1.25, -0.75, 180.0
    src = (a * SRC_LAT[:, None] + b * SRC_LON[None, :] + c).astype(np.float32)  # ~300
    plan = RegridPlan.bilinear(SRC_LAT, SRC_LON, lat, lon)
    got = plan.apply_host(src.reshape(-1))
    assert got.dtype == np.float32 and got.shape == (40,)
    want = a * lat + b * (np.mod(lon - SRC_LON[0], 360.0) + SRC_LON[0]) + c
    big = np.abs(src.reshape(-1)[plan.corner]).max(0)
    err = np.abs(got.astype(np.float64) - want)
    assert (err <= 2 * np.spacing(big.astype(np.float32)).astype(np.float64)).all(), err.max()
    # and big-endian input (the file's bytes) gives the same bits
    assert np.array_equal(bits(plan.apply_host(src.reshape(-1).astype(">f4"))), bits(got))


def _special_grids(rng, npts=35):
    g = rng.normal(0.0, 50.0, (8, npts)).astype(np.float32)
    g[0, 3], g[1, 4], g[2, 5] = np.nan, -0.0, 1e-41   # a NaN, a negative zero, a denormal
    g[3].view(np.uint32)[7] = 0x7FC12345              # a NaN with a payload
    return g


def test_apply_host_is_the_documented_operation_order():
    rng = np.random.default_rng(2)
    lat, lon = columns40(seed=2)
    mask = rng.random((5, 7)) > 0.15
    mask[0, 0] = mask[4, 6] = mask[2, 3] = mask[0, 6] = mask[4, 0] = mask[1, 5] = True
    ok = []
    for c in range(40):   # keep the columns the mask leaves a source for
        try:
            RegridPlan.bilinear(SRC_LAT, SRC_LON, lat[c:c + 1], lon[c:c + 1], mask)
            ok.append(c)
        except ValueError:
            pass
    plan = RegridPlan.bilinear(SRC_LAT, SRC_LON, lat[ok], lon[ok], mask)
    assert (plan.corner < 0).any() and len(ok) > 30
    g = _special_grids(rng)
    for near in ((), ("RAINRATE", "SWDOWN"), tuple(L.LDASIN[:-1])):
        idx = {L.LDASIN.index(v) for v in near}
        assert nearest_mask(near) == sum(1 << i for i in idx)
        assert np.array_equal(bits(plan.apply_host(g, nearest=near)), restated(plan, g, idx))
    # one row at a time is the same as the block
    assert np.array_equal(bits(plan.apply_host(g[4])), bits(plan.apply_host(g)[4]))
    assert np.array_equal(bits(plan.apply_host(g[3], nearest=True)),
                          bits(plan.apply_host(g, nearest=(3,))[3]))
    with pytest.raises(ValueError):
        plan.apply_host(g[:, :-1])
    with pytest.raises(ValueError):
        nearest_mask(("COSZ",))


def test_masked_corner_is_skipped_not_multiplied():
    mask = np.ones((5, 7), bool)
    mask[1, 2] = False                      # corner (j0+1, i0+1) of the cell below
    plan = RegridPlan.bilinear(SRC_LAT, SRC_LON, [30.4], [-118.7], mask)
    assert plan.corner[3, 0] == -1 and plan.weight[3, 0] == 0.0
    assert (plan.corner[:3, 0] == [1, 2, 8]).all()
    fy, fx = (30.4 - 30.0) / 1.0, (-118.7 + 120.0 - 1.0) / 1.0
    w = np.array([(1 - fy) * (1 - fx), (1 - fy) * fx, fy * (1 - fx)])
    w = w / ((w[0] + w[1]) + w[2])
    assert np.array_equal(plan.weight[:3, 0], w)
    src = np.arange(35, dtype=np.float32) + 270.0
    src[1 * 7 + 2] = np.nan                 # the masked point's value never enters
    got = plan.apply_host(src)
    want = np.float32((0.0 + 271.0 * w[0] + 272.0 * w[1]) + 278.0 * w[2])
    assert np.isfinite(got[0]) and bits(got)[0] == bits(want)
    assert np.isfinite(plan.interp_scalar(src.astype(np.float64))[0])


def test_nearest_ties_and_bits():
    # hand-made plans: equal weights tie to the lowest valid entry
    corner = np.array([[-1, 0, 5], [3, 1, 6], [4, 2, -1], [9, 3, 8]], np.int32)
    weight = np.array([[0.0, 0.25, 0.1], [0.5, 0.25, 0.4], [0.5, 0.25, 0.0], [0.0, 0.25, 0.4]])
    plan = RegridPlan(3, 12, corner, weight)
    src = np.arange(12, dtype=np.float32)
    src.view(np.uint32)[3] = 0x7FC00BAD    # a NaN payload
    src[1] = -0.0
    src[0] = -0.0
    got = bits(plan.apply_host(src, nearest=True))
    assert got[0] == 0x7FC00BAD             # entries 1 and 2 tie: the lower, point 3
    assert got[1] == 0x80000000             # all four tie: entry 0, point 0 = -0.0
    assert got[2] == bits(np.float32(6.0))  # entries 1 and 3 tie: entry 1, point 6
    # no valid entry, and a corner past the grid: quiet-NaN rows
    bad = RegridPlan(2, 12, np.array([[-1, 0], [-1, 1], [-1, 12], [-1, 2]], np.int32),
                     np.full((4, 2), 0.25))
    assert (bits(bad.apply_host(src)) == 0x7FC00000).all()
    assert (bits(bad.apply_host(np.stack([src] * 8), nearest=(5,))) == 0x7FC00000).all()
    assert np.isnan(bad.interp_scalar(src)).all()


# ---- downscaling ----------------------------------------------------------------------
def _block(n, seed=0):
    """A plausible LDASIN block; T2D on a 1/8 K lattice, so that t0 - 6.5 is an
    fp32 value too and the humidity check sees no rounding of the temperature
    (half an fp32 ulp of T alone is ~1e-6 of e_sat)."""
    rng = np.random.default_rng(seed)
    b = np.zeros((L.NLDASIN, n), np.float32)
    b[L.LDASIN.index("T2D")] = np.round(rng.uniform(255.0, 305.0, n) * 8) / 8
    b[L.LDASIN.index("Q2D")] = rng.uniform(5e-4, 1.5e-2, n)
    b[L.LDASIN.index("U2D")] = rng.normal(0, 3, n)
    b[L.LDASIN.index("V2D")] = rng.normal(0, 3, n)
    b[L.LDASIN.index("PSFC")] = rng.uniform(7.5e4, 1.02e5, n)
    b[L.LDASIN.index("RAINRATE")] = rng.uniform(0, 1e-3, n)
    b[L.LDASIN.index("SWDOWN")] = rng.uniform(0, 900, n)
    b[L.LDASIN.index("LWDOWN")] = rng.uniform(200, 420, n)
    b[L.LDASIN.index("COSZ")] = rng.uniform(-1, 1, n)
    return b


def test_downscale_host():
    b = _block(64)
    b[L.LDASIN.index("SWDOWN"), 0] = -0.0
    iT, iQ, iP, iL = (L.LDASIN.index(v) for v in ("T2D", "Q2D", "PSFC", "LWDOWN"))
    same = downscale_host(b, np.zeros(64, np.float32), 0.0065)
    assert same.dtype == np.float32 and np.array_equal(bits(same), bits(b))
    assert 0.0065 * 1000.0 == 6.5
    up = downscale_host(b, np.full(64, 1000.0, np.float32), 0.0065)
    assert np.array_equal(bits(up[iT]), bits((b[iT].astype(np.float64) - 6.5).astype(np.float32)))
    assert (up[iP] < b[iP]).all() and (up[iQ] < b[iQ]).all() and (up[iL] < b[iL]).all()
    for i in range(L.NLDASIN):
        if i not in (iT, iQ, iP, iL):
            assert np.array_equal(bits(up[i]), bits(b[i])), L.LDASIN[i]
    # hypsometric pressure at the layer's mean temperature
    tm = b[iT].astype(np.float64) - 3.25
    assert np.allclose(up[iP], b[iP] * np.exp(-9.80616 * 1000.0 / (287.04 * tm)), rtol=2e-7)
    # relative humidity (q p / e_sat(T), Magnus) recomputed from the outputs

    def rh(x):
        t, q, p = (x[i].astype(np.float64) for i in (iT, iQ, iP))
        return q * p / (0.622 * 611.2 * np.exp(17.67 * (t - 273.15) / (t - 29.65)))
    assert np.allclose(rh(up), rh(b), rtol=1e-6, atol=0)
    # the input is not modified, and down is the other way
    down = downscale_host(b, np.full(64, -500.0, np.float32), 0.0065)
    assert (down[iT] > b[iT]).all() and (down[iP] > b[iP]).all()


# ---- files and reader -----------------------------------------------------------------
def _model_grid():
    lat = 30.5 + 0.5 * np.arange(4)[:, None] + 0.0 * np.arange(6)[None, :]
    lon = -119.0 + 0.75 * np.arange(6)[None, :] + 0.0 * np.arange(4)[:, None]
    mask = np.ones((4, 6), bool)
    mask[1, 2] = mask[3, 0] = False
    return ncio.Grid(lat, lon, mask)


def test_forcing_grid_file_round_trip(tmp_path):
    rng = np.random.default_rng(1)
    mask = rng.random((5, 7)) > 0.2
    fg = ncio.ForcingGrid(SRC_LAT, SRC_LON, hgt=rng.uniform(0, 2000, (5, 7)), mask=mask,
                          hgt_m=rng.uniform(0, 2000, (4, 6)))
    p = str(tmp_path / "forcing_grid.nc")
    ncio.write_forcing_grid(p, fg)
    g = ncio.read_forcing_grid(p)
    assert g.shape == (5, 7) and g.npts == 35
    assert np.array_equal(g.lat, SRC_LAT) and np.array_equal(g.lon, SRC_LON)
    assert np.array_equal(g.hgt, fg.hgt) and np.array_equal(g.hgt_m, fg.hgt_m)
    assert g.mask.dtype == bool and np.array_equal(g.mask, mask)
    bare = str(tmp_path / "bare.nc")
    ncio.write_forcing_grid(bare, ncio.ForcingGrid(SRC_LAT[::-1], SRC_LON))
    g = ncio.read_forcing_grid(bare)
    assert g.hgt is None and g.mask is None and g.hgt_m is None
    assert np.array_equal(g.lat, SRC_LAT[::-1])


def test_reader_on_a_source_grid(tmp_path):
    rng = np.random.default_rng(4)
    grid = _model_grid()
    fg = ncio.ForcingGrid(SRC_LAT, SRC_LON, hgt=rng.uniform(0, 2000, (5, 7)),
                          hgt_m=rng.uniform(0, 2000, (4, 6)))
    every = datetime.timedelta(hours=1)
    forcing = np.zeros((L.NFORCING, 35), np.float32)
    for fld, var in ncio.LDASIN_MAP.items():
        forcing[L.FORCING.index(fld)] = rng.normal(100.0, 30.0, 35)
    indir = tmp_path / "ldasin"
    indir.mkdir()
    ncio.write_ldasin(ncio.ldasin_path(str(indir), T0), fg.as_grid(), forcing, T0, extras=False)
    # a later file lies on the model grid: the wrong shape for this reader
    later = T0 + 2 * every
    ncio.write_ldasin(ncio.ldasin_path(str(indir), later), grid,
                      np.zeros((L.NFORCING, grid.n), np.float32), later, extras=False)
    cols = rng.permutation(grid.n)[:17]
    near = ("RAINRATE",)
    fr = ncio.LdasinForcing(str(indir), grid, T0, every, cols=cols, threads=2, src=fg,
                            nearest=near)
    assert fr.npts == 35 and fr.plan.ncol == 17 and fr.nearest_mask == 1 << 5
    assert fr.ingestible(T0) and not fr.ingestible(later)
    raw = fr.grid_raw(T0)
    assert raw.shape == (8, 35) and raw.dtype == np.dtype(">f4")
    for i, var in enumerate(L.LDASIN[:-1]):
        fld = [k for k, v in ncio.LDASIN_MAP.items() if v == var][-1]  # (PSFC, not SFCPRS)
        assert np.array_equal(bits(raw[i]), bits(forcing[L.FORCING.index(fld)])), var
    want = fr.plan.apply_host(raw, nearest=near)
    blk = np.full((L.NLDASIN, 17), -7.0, np.float32)
    assert fr.block(T0, out=blk) is blk
    assert np.array_equal(bits(blk[:8]), bits(want))
    assert (blk[8] == -7.0).all()                       # COSZ is the caller's
    assert np.array_equal(bits(fr.raw(0, T0)[:8]), bits(want))
    f12 = fr(0, T0)
    assert np.array_equal(bits(f12[L.FORCING.index("SFCTMP")]), bits(want[0]))
    with pytest.raises(ValueError):
        fr.point()
    # the plan is the rank's own columns', and dz the terrain difference there
    lat, lon = grid.columns(grid.lat_deg)[cols], grid.columns(grid.lon_deg)[cols]
    ref = RegridPlan.bilinear(SRC_LAT, SRC_LON, lat, lon)
    assert np.array_equal(fr.plan.corner, ref.corner) and np.array_equal(fr.plan.weight, ref.weight)
    dz = fr.dz()
    assert dz.dtype == np.float32
    assert np.array_equal(dz, (grid.columns(fg.hgt_m)[cols] -
                               ref.interp_scalar(fg.hgt)).astype(np.float32))
    # without src nothing changes: the model-grid file is ingestible and has points
    plain = ncio.LdasinForcing(str(indir), grid, T0, every, cols=cols, threads=1)
    assert plain.plan is None and plain.ingestible(later) and not plain.ingestible(T0)
    assert plain.point().shape == (17,)
    with pytest.raises(ValueError):
        plain.dz()


# ---- ABI --------------------------------------------------------------------------------
def test_regrid_entries_exported(engine_lib):
    decl = set(re.findall(r"^\s*(?:int|int64_t|void\*?|const char\*)\s*(nmp_\w+)\s*\(", _header(),
                          re.M))
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.library_path()], capture_output=True,
                        text=True, check=True).stdout
    exported = set(re.findall(r"\bT (nmp_\w+)$", nm, re.M))
    for name in ("nmp_ldasin_regrid", "nmp_ldasin_downscale"):
        assert name in decl, f"{name} not declared in the header"
        assert name in _lib.EXPORTED_SYMBOLS and name in exported
        assert getattr(engine_lib, name).argtypes is not None, f"{name} not bound in lib.py"
    assert engine_lib.nmp_abi_version() == 8   # additive: the version stays
    assert engine_lib.nmp_ldasin_regrid(None, 1, 1, 1, None, None, None, 0, None, None) == -1
    assert engine_lib.nmp_ldasin_downscale(None, 1, 1, None, 0.0065, None, None) == -1
