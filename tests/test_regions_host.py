"""Region-aggregated output, host side (no GPU): nmp_region_reduce is declared,
exported and bound and refuses bad sizes before any device work; RegionPlan
lays the plan out as the header states it; reduce_host equals the summation
tree restated here (`tree`, written from include/noahmp_engine.h alone) and
stays within the tree's depth of the exact sum; the REGIONS files round-trip;
a REGION grid reaches the right engine columns."""
import ctypes as C
import datetime
import math
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from noahmp_amd import cases, driver, layout as L, lib as _lib, ncio
from noahmp_amd.regions import RegionPlan
from test_abi_host import _enum_values, _header
from test_ncio import bits, grid_for

T0 = datetime.datetime(2000, 1, 1)
CH = 256


def tree(fields, entry_col, entry_w, chunk0, wsum):
    """The header's summation tree: (sums, means), each (nfield, nreg)."""
    nf, nchunk, nreg = fields.shape[0], entry_col.size // CH, chunk0.size - 1
    partial = np.zeros((nf, nchunk))
    sums = np.zeros((nf, nreg))
    with np.errstate(all="ignore"):
        for k in range(nchunk):
            a = np.zeros((nf, 64))                      # lane l starts at +0.0
            for j in range(4):                          # entries l, l+64, l+128, l+192
                e = slice(CH * k + 64 * j, CH * k + 64 * j + 64)
                c, w = entry_col[e], entry_w[e]
                real = c >= 0                           # a pad is skipped
                a[:, real] = a[:, real] + fields[:, c[real]].astype(np.float64) * w[real]
            for s in (32, 16, 8, 4, 2, 1):
                a = a[:, :s] + a[:, s:2 * s]
            partial[:, k] = a[:, 0]
        for r in range(nreg):
            for k in range(chunk0[r], chunk0[r + 1]):   # chunk order, from +0.0
                sums[:, r] = sums[:, r] + partial[:, k]
        return sums, sums / wsum


def test_region_entry_exported(engine_lib):
    """Fails without the feature: the entry, its constant and its binding."""
    decl = set(re.findall(r"^\s*(?:int|int64_t|void\*?|const char\*)\s*(nmp_\w+)\s*\(", _header(),
                          re.M))
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.library_path()], capture_output=True,
                        text=True, check=True).stdout
    exported = set(re.findall(r"\bT (nmp_\w+)$", nm, re.M))
    name = "nmp_region_reduce"
    assert name in decl, f"{name} not declared in the header"
    assert name in _lib.EXPORTED_SYMBOLS and name in exported
    assert getattr(engine_lib, name).argtypes is not None, f"{name} not bound in lib.py"
    assert _enum_values(_header())["NMP_REGION_CHUNK"] == L.REGION_CHUNK == 256
    assert re.search(r"#define NMP_ABI_VERSION 8\b", _header())  # additive: the version stays
    assert engine_lib.nmp_abi_version() == 8


def test_region_reduce_argument_errors(engine_lib):
    """Sizes and pointers are checked before the engine or a device is
    touched: a zeroed block stands in for the handle (never read here)."""
    fake = C.create_string_buffer(1 << 16)
    eng = C.cast(fake, C.c_void_p)
    buf = C.create_string_buffer(4096)
    p = C.cast(buf, C.c_void_p)

    def call(eng=eng, ncol=8, ld=8, nfield=2, fields=p, nchunk=1, ec=p, ew=p, nreg=1, c0=p,
             wsum=p, partial=p, sums=p, means=None):
        return engine_lib.nmp_region_reduce(eng, ncol, ld, nfield, fields, nchunk, ec, ew, nreg,
                                            c0, wsum, partial, sums, means, None)
    E_ARG = -1
    assert call(eng=None) == E_ARG
    assert call(nfield=0) == E_ARG and call(nfield=-3) == E_ARG
    assert call(ld=7) == E_ARG
    assert call(ncol=-1, ld=8) == E_ARG
    assert call(ld=1 << 29) == E_ARG
    assert call(nchunk=-1) == E_ARG and call(nreg=-1) == E_ARG
    for k in ("fields", "ec", "ew", "c0", "wsum", "partial", "sums"):
        assert call(**{k: None}) == E_ARG, k
    # nothing to reduce: success, nothing launched (no pointer is looked at)
    assert call(nchunk=0, fields=None, ec=None, ew=None, partial=None) == 0
    assert call(nreg=0, c0=None, wsum=None, sums=None) == 0
    assert call(nchunk=0, nfield=0) == E_ARG  # sizes are still checked


def _example(n=3000, seed=3):
    """Ids out of order and with gaps, some columns in no region."""
    rng = np.random.default_rng(seed)
    sizes = {7: 1, 40: 63, 3: 64, 12: 65, 0: 255, 9: 256, 21: 257, 5: 1025}
    ids = np.full(n, -1, np.int64)
    free = rng.permutation(n)
    at = 0
    for rid, cnt in sizes.items():
        ids[free[at:at + cnt]] = rid
        at += cnt
    ids[free[at:at + 50]] = -5       # another negative id: also in no region
    w = rng.uniform(0.2, 3.0, n)
    return ids, w, sizes


def test_region_plan_layout():
    ids, w, sizes = _example()
    plan = RegionPlan.from_ids(ids, w)
    want_ids = sorted(sizes)
    assert plan.region_id.tolist() == want_ids           # sorted, unique, 1 / 2 / 4 ... absent
    assert plan.ncolumns.tolist() == [sizes[r] for r in want_ids]
    assert plan.entry_col.dtype == np.int32 and plan.entry_w.dtype == np.float64
    assert plan.region_chunk0.dtype == np.int64 and plan.region_chunk0[0] == 0
    nch = [-(-sizes[r] // CH) for r in want_ids]
    assert np.diff(plan.region_chunk0).tolist() == nch
    assert plan.nchunk == sum(nch) and plan.entry_col.size == plan.nchunk * CH == plan.entry_w.size
    seen = []
    for i, r in enumerate(want_ids):
        e = slice(plan.region_chunk0[i] * CH, plan.region_chunk0[i + 1] * CH)
        c, ww = plan.entry_col[e], plan.entry_w[e]
        cnt = sizes[r]
        mine = np.flatnonzero(ids == r)                   # ascending engine column order
        assert np.array_equal(c[:cnt], mine), r
        assert np.array_equal(bits(ww[:cnt]), bits(w[mine])), r
        assert (c[cnt:] == -1).all() and (bits(ww[cnt:]) == 0).all(), r   # pad: -1 / +0.0
        seen.append(c[:cnt])
    assert np.array_equal(np.sort(np.concatenate(seen)), np.flatnonzero(ids >= 0))
    # wsum: the tree over the weights (a field of ones)
    s, m = tree(np.ones((1, ids.size)), plan.entry_col, plan.entry_w, plan.region_chunk0,
                np.ones(plan.nreg))
    assert np.array_equal(bits(plan.wsum), bits(s[0]))
    # so a field of ones has mean exactly 1
    assert np.array_equal(plan.reduce_host(np.ones((1, ids.size), np.float32))[1],
                          np.ones((1, plan.nreg)))
    # defaults and refusals
    assert np.array_equal(RegionPlan.from_ids(ids).entry_w[RegionPlan.from_ids(ids).entry_col >= 0],
                          np.ones((ids >= 0).sum()))
    empty = RegionPlan.from_ids(np.full(10, -1))
    assert empty.nreg == 0 and empty.nchunk == 0 and empty.region_chunk0.tolist() == [0]
    with pytest.raises(ValueError):
        RegionPlan.from_ids(ids.astype(np.float64))
    with pytest.raises(ValueError):
        RegionPlan.from_ids(ids, w[:-1])


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_reduce_host_equals_the_tree(dt):
    ids, w, sizes = _example()
    n = ids.size
    rng = np.random.default_rng(11)
    f = (rng.normal(size=(5, n)) * np.array([1.0, 1e3, 1e-4, 300.0, 1.0])[:, None]).astype(dt)
    f[4] = np.where(rng.random(n) < 0.3, -999.9, 0.2)      # night-time ALBEDO reduces as it is
    f[0, np.flatnonzero(ids == 12)[5]] = np.nan           # one NaN column in region 12
    f[1, np.flatnonzero(ids == 7)[0]] = -0.0              # the one column of region 7
    plan = RegionPlan.from_ids(ids, w)
    sums, means = plan.reduce_host(f)
    es, em = tree(f, plan.entry_col, plan.entry_w, plan.region_chunk0, plan.wsum)
    assert sums.dtype == means.dtype == np.float64 and sums.shape == (5, plan.nreg)
    assert np.array_equal(bits(sums), bits(es)) and np.array_equal(bits(means), bits(em))
    r12 = plan.region_id.tolist().index(12)
    nan = np.isnan(sums)
    assert nan[0, r12] and nan.sum() == 1 and np.isnan(means[0, r12])
    r7 = plan.region_id.tolist().index(7)
    assert bits(sums[1:2, r7:r7 + 1])[0, 0] == 0          # +0.0 + (-0.0 * w) = +0.0
    # within the tree's depth of the exact sum: 3 adds in the lane, 6 in the
    # butterfly, one per chunk (the product's rounding rides on the first,
    # exact, add), times the unit roundoff, times sum |v w|
    u = 2.0 ** -53
    for fi in range(5):
        for ri, rid in enumerate(plan.region_id):
            if nan[fi, ri]:
                continue
            c = np.flatnonzero(ids == rid)
            prods = [Fraction(float(f[fi, j])) * Fraction(float(w[j])) for j in c]
            exact, mag = sum(prods), sum(abs(p) for p in prods)
            nchunks = -(-c.size // CH)
            bound = (3 + 6 + nchunks) * u * float(mag)
            err = abs(Fraction(float(sums[fi, ri])) - exact)
            assert err <= Fraction(bound), (fi, rid, float(err), bound)
            # math.fsum of the exact products, each as its double head and tail
            hi = [float(p) for p in prods]
            lo = [float(p - Fraction(h)) for p, h in zip(prods, hi)]
            assert all(Fraction(h) + Fraction(t) == p for h, t, p in zip(hi, lo, prods))
            fs = math.fsum(hi + lo)
            assert fs == float(exact)
            assert abs(sums[fi, ri] - fs) <= bound, (fi, rid)


def test_reduce_host_refuses_other_shapes():
    plan = RegionPlan.from_ids(np.array([0, 0, 1]))
    with pytest.raises(ValueError):
        plan.reduce_host(np.zeros((2, 4)))


def test_regions_files_round_trip(tmp_path):
    rng = np.random.default_rng(5)
    rid, ncol = np.array([2, 5, 11]), np.array([7, 300, 1])
    wsum = rng.uniform(1, 9, 3)
    out = tmp_path / "out"
    out.mkdir()
    names = L.DIAG_OUT_ACC
    stack, times = [], []
    for k in range(3):
        t = T0 + datetime.timedelta(hours=3 * (k + 1))
        m = rng.normal(size=(len(names), 3))
        m[3, 1] = np.nan
        m[5, 0] = -0.0
        p = ncio.regions_path(str(out), t)
        assert p.endswith(t.strftime("%Y%m%d%H") + ".REGIONS_DOMAIN1")
        ncio.write_regions(p, rid, ncol, wsum, m, t, names)
        r = ncio.read_regions(p)
        assert r["names"] == list(names) and r["time"] == t
        assert np.array_equal(r["region_id"], rid) and np.array_equal(r["ncolumns"], ncol)
        assert np.array_equal(bits(r["weight"]), bits(wsum))
        assert r["means"].dtype == np.float64 and np.array_equal(bits(r["means"]), bits(m))
        # the same inputs write the same bytes
        q = str(tmp_path / f"again{k}.nc")
        ncio.write_regions(q, rid, ncol, wsum, m, t, names)
        assert open(p, "rb").read() == open(q, "rb").read()
        stack.append(m)
        times.append(t)
    s = ncio.read_regions_series(str(out))
    assert s["times"] == times and s["names"] == list(names)
    assert s["means"].shape == (3, len(names), 3)
    assert np.array_equal(bits(s["means"]), bits(np.stack(stack)))
    assert np.array_equal(s["region_id"], rid)
    # the 16 names by default; always double
    p = str(tmp_path / "d.nc")
    ncio.write_regions(p, rid, ncol, wsum, np.zeros((16, 3), np.float32), T0)
    assert ncio.read_regions(p)["names"] == list(L.DIAG_OUT)
    with pytest.raises(FileNotFoundError):
        ncio.read_regions_series(str(tmp_path / "nowhere"))


def test_region_grid_maps_to_engine_columns(tmp_path, ref_params):
    """REGION(south_north, west_east) -> per-column ids through the land mask
    and the engine's column order; weights from AREA, cos(lat), 1 or an array."""
    cols = cases.make_columns(32, "mixed", ref_params, seed=8)
    grid = grid_for(cols)
    ny, nx = grid.shape
    rng = np.random.default_rng(2)
    reg = rng.integers(-1, 4, size=(ny, nx)).astype(np.int32)   # -1: unassigned
    reg[~grid.mask] = 3                                          # off the land mask: no column
    area = rng.uniform(1.0, 2.0, size=(ny, nx))
    perm = rng.permutation(grid.n)
    a, b = str(tmp_path / "a.nc"), str(tmp_path / "b.nc")
    ncio.write_region_map(a, grid, reg, area)
    ncio.write_region_map(b, grid, reg)
    land = reg.reshape(-1)[grid.index]
    ids, w = driver.region_columns(a, grid, perm, "area")
    assert ids.dtype == np.int64 and np.array_equal(ids, land[perm])
    assert w.dtype == np.float64 and np.array_equal(bits(w), bits(area.reshape(-1)[grid.index][perm]))
    ids2, w2 = driver.region_columns(b, grid, perm, "area")
    assert np.array_equal(ids2, ids)
    assert np.array_equal(bits(w2), bits(np.cos(grid.lat_rad.astype(np.float64))[perm]))
    assert (driver.region_columns(b, grid, perm, "equal")[1] == 1.0).all()
    given = rng.uniform(size=grid.n)
    assert np.array_equal(driver.region_columns(b, grid, perm, given)[1], given[perm])
    ids3, _ = driver.region_columns(b, grid, None, "equal")
    assert np.array_equal(ids3, land)
    # the plan counts only land columns with id >= 0
    plan = RegionPlan.from_ids(ids, w)
    assert plan.ncolumns.sum() == (land >= 0).sum()
    with pytest.raises(ValueError):
        driver.region_columns(b, grid, perm, "volume")
    with pytest.raises(ValueError):
        driver.region_columns(b, grid, perm, given[:-1])
    other = ncio.Grid(np.zeros((3, 3)), np.zeros((3, 3)), np.ones((3, 3), bool))
    with pytest.raises(ValueError):
        ncio.read_region_map(b, other)
