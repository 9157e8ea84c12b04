"""Region-aggregated output on the GPU: nmp_region_reduce against the summation
tree of include/noahmp_engine.h restated here in numpy (`make_plan`, `tree`:
not taken from the code under test), bit for bit, at the tree's edges; and the
offline driver's REGIONS files against that restatement applied to the columns
read back from the run's own LDASOUT files, through --regions-only, a restart
and two ranks.

Bounds: every comparison is on bits except the regions' water budget, whose
bound is derived in test_driver_region_budget_closes."""
import ctypes as C
import glob
import os
from fractions import Fraction

import numpy as np
import pytest
import torch

import noahmp_pkg  # noqa: F401  (spawned ranks re-import this module)
from golden_io import load
from noahmp_amd import config, driver, layout as L, ncio
from noahmp_amd.engine import Engine
from noahmp_amd.params import Params
from noahmp_amd.regions import RegionPlan

pytestmark = pytest.mark.gpu

CH = 256
NCOL, LD = 2000, 2048
SIZES = (1, 63, 64, 65, 255, 256, 257, 1025)   # 1,986 columns; 14 in no region


def ibits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize])


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(ibits(a), ibits(b))


# ---- numpy restatement ---------------------------------------------------------------
def make_plan(ids, w):
    """(region ids, entry_col, entry_w, region_chunk0) as the header lays them out."""
    rids = sorted(set(int(i) for i in ids if i >= 0))
    ec, ew, chunk0 = [], [], [0]
    for r in rids:
        cols = [c for c in range(len(ids)) if ids[c] == r]          # ascending column order
        pad = -len(cols) % CH
        ec += cols + [-1] * pad
        ew += [w[c] for c in cols] + [0.0] * pad
        chunk0.append(len(ec) // CH)
    return (np.array(rids, np.int64), np.array(ec, np.int32), np.array(ew, np.float64),
            np.array(chunk0, np.int64))


def tree(fields, entry_col, entry_w, chunk0, wsum=None):
    """(sums, means) (nfield, nreg) by the header's tree; wsum None: the tree's
    own sum of the weights."""
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
        if wsum is None:
            wsum = tree(np.ones((1, fields.shape[1])), entry_col, entry_w, chunk0,
                        np.ones(nreg))[0][0]
        return sums, sums / wsum


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda:0")


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _engine(precision):
    return Engine(Params.builtin(), L.CASE_NML_OPTIONS, device=0, precision=precision)


def _membership(rng, n=NCOL, sizes=SIZES):
    """Region r (ids 10, 20, ...: gaps) holds sizes[r] columns shuffled over the block."""
    ids = np.full(n, -1, np.int64)
    free, at = rng.permutation(n), 0
    for r, cnt in enumerate(sizes):
        ids[free[at:at + cnt]] = 10 * (r + 1)
        at += cnt
    return ids


def _raw_reduce(eng, fields, ld, ncol, nf, ec, ew, c0, wsum, means=True, stream=None, off=0):
    """nmp_region_reduce through the C ABI; fields: a device tensor whose rows
    are ld apart, read from element `off`."""
    nchunk, nreg = ec.numel() // CH, c0.numel() - 1
    partial = torch.full((nf, max(nchunk, 1)), np.nan, dtype=torch.float64, device="cuda:0")
    sums = torch.full((nf, nreg), np.nan, dtype=torch.float64, device="cuda:0")
    mean = torch.full((nf, nreg), np.nan, dtype=torch.float64, device="cuda:0") if means else None
    s = stream if stream is not None else torch.cuda.current_stream(0)
    fp = C.c_void_p(fields.data_ptr() + off * fields.element_size())
    rc = eng._lib.nmp_region_reduce(eng._h, ncol, ld, nf, fp, nchunk, _ptr(ec), _ptr(ew), nreg,
                                    _ptr(c0), _ptr(wsum), _ptr(partial), _ptr(sums), _ptr(mean),
                                    C.c_void_p(s.cuda_stream))
    assert rc == 0, rc
    return sums, mean


# ---- 1. the kernel ------------------------------------------------------------------
@pytest.mark.parametrize("nfield", [1, 16, 35])
@pytest.mark.parametrize("precision", [4, 8])
def test_region_reduce_is_the_documented_tree(engine_lib, precision, nfield):
    eng = _engine(precision)
    dtype = np.float32 if precision == 4 else np.float64
    rng = np.random.default_rng(100 * precision + nfield)
    ids = _membership(rng)
    assert (ids < 0).sum() == 14
    w = rng.uniform(0.1, 4.0, NCOL)
    scale = 10.0 ** rng.integers(-4, 4, size=(nfield, 1))
    f = np.full((nfield, LD), np.nan, dtype)            # the padding past ncol is never read
    f[:, :NCOL] = (rng.normal(size=(nfield, NCOL)) * scale).astype(dtype)
    nan_col = np.flatnonzero(ids == 40)[7]              # region 40 (65 columns) holds a NaN column
    f[:, nan_col] = np.nan
    f[:, np.flatnonzero(ids == 10)[0]] = -0.0           # the one column of region 10
    f[:, np.flatnonzero(ids == 80)[3]] = -0.0
    outside = np.flatnonzero(ids < 0)
    f[0, outside[0]] = np.nan                           # a NaN in no region reaches no sum
    rids, ec, ew, c0 = make_plan(ids, w)
    assert rids.tolist() == [10 * (r + 1) for r in range(len(SIZES))]
    assert np.diff(c0).tolist() == [1, 1, 1, 1, 1, 1, 2, 5]
    want_s, want_m = tree(f[:, :NCOL], ec, ew, c0)
    wsum = tree(np.ones((1, NCOL)), ec, ew, c0, np.ones(len(rids)))[0][0]
    fd, dec, dew, dc0, dws = _dev(f), _dev(ec), _dev(ew), _dev(c0), _dev(wsum)
    sums, means = _raw_reduce(eng, fd, LD, NCOL, nfield, dec, dew, dc0, dws, means=True)
    sums0, none = _raw_reduce(eng, fd, LD, NCOL, nfield, dec, dew, dc0, dws, means=False)
    torch.cuda.synchronize()
    got_s, got_m = sums.cpu().numpy(), means.cpu().numpy()
    assert none is None and same_bits(sums0.cpu().numpy(), got_s)
    assert same_bits(got_s, want_s) and same_bits(got_m, want_m)
    # NaN in region 40 and only there; -0.0 columns leave +0.0 / an ordinary sum
    nan = np.isnan(got_s)
    assert nan[:, 3].all() and nan.sum() == nfield and np.isnan(got_m[:, 3]).all()
    assert (ibits(got_s[:, 0]) == 0).all()
    # the product plan and the front end give the same plan and the same bits
    plan = RegionPlan.from_ids(ids, w)
    assert np.array_equal(plan.entry_col, ec) and same_bits(plan.entry_w, ew)
    assert np.array_equal(plan.region_chunk0, c0) and same_bits(plan.wsum, wsum)
    s2 = torch.empty((nfield, plan.nreg), dtype=torch.float64, device="cuda:0")
    m2 = torch.empty_like(s2)
    eng.region_reduce(_dev(f[:, :NCOL]), plan.to("cuda:0"), s2, m2)
    torch.cuda.synchronize()
    assert same_bits(s2.cpu().numpy(), want_s) and same_bits(m2.cpu().numpy(), want_m)
    eng.close()


@pytest.mark.parametrize("precision", [4, 8])
def test_region_plan_extremes(engine_lib, precision):
    """One region of every column (8 chunks summed in order) and one region
    per column (2,000 chunks of one entry)."""
    eng = _engine(precision)
    dtype = np.float32 if precision == 4 else np.float64
    rng = np.random.default_rng(precision)
    f = (rng.normal(size=(3, NCOL)) * 250.0).astype(dtype)
    w = rng.uniform(0.5, 1.5, NCOL)
    for ids in (np.zeros(NCOL, np.int64), rng.permutation(NCOL).astype(np.int64)):
        rids, ec, ew, c0 = make_plan(ids, w)
        want_s, want_m = tree(f, ec, ew, c0)
        plan = RegionPlan.from_ids(ids, w).to("cuda:0")
        assert plan.nreg == len(rids) and plan.nchunk == ec.size // CH
        s = torch.empty((3, plan.nreg), dtype=torch.float64, device="cuda:0")
        m = torch.empty_like(s)
        eng.region_reduce(_dev(f), plan, s, m)
        torch.cuda.synchronize()
        assert same_bits(s.cpu().numpy(), want_s) and same_bits(m.cpu().numpy(), want_m)
    # one column per region: sum = +0.0 + v * w, mean = that / (+0.0 + 1 * w)
    order = np.argsort(ids)
    with np.errstate(all="ignore"):
        assert same_bits(s.cpu().numpy(), (f.astype(np.float64) * w)[:, order] + 0.0)
    # an empty plan: nothing launched, nothing written
    empty = RegionPlan.from_ids(np.full(NCOL, -1)).to("cuda:0")
    s0 = torch.empty((3, 0), dtype=torch.float64, device="cuda:0")
    eng.region_reduce(_dev(f), empty, s0)
    torch.cuda.synchronize()
    eng.close()


@pytest.mark.parametrize("precision", [4, 8])
def test_region_reduce_launch_independence(engine_lib, precision):
    """A sub-block (the fields pointer offset by lo, ld unchanged, the plan's
    indices relative to lo) and a stream other than the current one give the
    bits of the restatement, i.e. of a contiguous copy on the current stream."""
    eng = _engine(precision)
    dtype = np.float32 if precision == 4 else np.float64
    rng = np.random.default_rng(7 + precision)
    lo, hi, nf = 37, 1900, 4
    f = (rng.normal(size=(nf, LD)) * 40.0).astype(dtype)
    n = hi - lo
    ids = _membership(rng, n, (1, 300, 513, 700))
    w = rng.uniform(0.1, 4.0, n)
    rids, ec, ew, c0 = make_plan(ids, w)
    sub = np.ascontiguousarray(f[:, lo:hi])
    want_s, want_m = tree(sub, ec, ew, c0)
    wsum = tree(np.ones((1, n)), ec, ew, c0, np.ones(len(rids)))[0][0]
    fd, dec, dew, dc0, dws = _dev(f), _dev(ec), _dev(ew), _dev(c0), _dev(wsum)
    a_s, a_m = _raw_reduce(eng, fd, LD, n, nf, dec, dew, dc0, dws, off=lo)
    b_s, b_m = _raw_reduce(eng, _dev(sub), n, n, nf, dec, dew, dc0, dws)
    side = torch.cuda.Stream(0)
    side.wait_stream(torch.cuda.current_stream(0))
    c_s, c_m = _raw_reduce(eng, fd, LD, n, nf, dec, dew, dc0, dws, stream=side, off=lo)
    torch.cuda.synchronize()
    for s, m in ((a_s, a_m), (b_s, b_m), (c_s, c_m)):
        assert same_bits(s.cpu().numpy(), want_s) and same_bits(m.cpu().numpy(), want_m)
    eng.close()


@pytest.mark.parametrize("sizes", [(31 * CH,), (32 * CH,), (71 * CH - 5,), (70 * CH, 1)],
                         ids=["31chunks", "32chunks", "71chunks", "70chunks+1column"])
def test_region_reduce_long_regions(engine_lib, sizes):
    """Plans that average 32 chunks or more per region take pass 2's
    one-wavefront-per-sum kernel: below the threshold, at it (one partial
    batch of 32), a full batch of 64 plus a tail of 7, and a long region
    beside a one-column one -- the same sequential tree, bit for bit."""
    eng = _engine(4)
    rng = np.random.default_rng(len(sizes) + sizes[0])
    n = sum(sizes) + 9
    ids = _membership(rng, n, sizes)
    w = rng.uniform(0.1, 4.0, n)
    f = (rng.normal(size=(2, n)) * np.array([[1.0], [1e4]])).astype(np.float32)
    rids, ec, ew, c0 = make_plan(ids, w)
    assert np.diff(c0).tolist() == [-(-s // CH) for s in sizes]
    want_s, want_m = tree(f, ec, ew, c0)
    plan = RegionPlan.from_ids(ids, w).to("cuda:0")
    s = torch.empty((2, plan.nreg), dtype=torch.float64, device="cuda:0")
    m = torch.empty_like(s)
    eng.region_reduce(_dev(f), plan, s, m)
    torch.cuda.synchronize()
    assert same_bits(s.cpu().numpy(), want_s) and same_bits(m.cpu().numpy(), want_m)
    eng.close()


def test_region_reduce_front_end_checks(engine_lib):
    eng = _engine(4)
    plan = RegionPlan.from_ids(np.arange(10) % 3).to("cuda:0")
    f = torch.zeros((2, 10), device="cuda:0")
    s = torch.zeros((2, 3), dtype=torch.float64, device="cuda:0")
    with pytest.raises(AssertionError):
        eng.region_reduce(f.double(), plan, s)                       # not the engine's precision
    with pytest.raises(AssertionError):
        eng.region_reduce(f, plan, s.float())                        # sums are double
    with pytest.raises(AssertionError):
        eng.region_reduce(torch.zeros((2, 11), device="cuda:0"), plan, s)  # another block's plan
    with pytest.raises(AssertionError):
        eng.region_reduce(f, RegionPlan.from_ids(np.arange(10) % 3), s)  # not on the device
    with pytest.raises(AssertionError):
        eng.region_reduce(f.t().contiguous().t(), plan, s)           # not contiguous
    eng.close()


# ---- 2. the driver ------------------------------------------------------------------
def _regions_files(outdir):
    return sorted(glob.glob(os.path.join(outdir, "*.REGIONS_DOMAIN1")))


def _ldasout_files(outdir):
    return sorted(glob.glob(os.path.join(outdir, "*.LDASOUT_DOMAIN1")))


@pytest.fixture(scope="module")
def traj():
    return load("traj_casenml.npz")


@pytest.fixture(scope="module")
def case(engine_lib, traj, tmp_path_factory):
    """The small netCDF case of test_gpu_driver.py (the traj_casenml day, 32
    columns) with a REGION / AREA file of 3 regions plus unassigned points, and
    its runs: with regions (16 and 35 fields), without, regions only."""
    from test_gpu_driver import _write_netcdf_case
    tmp = tmp_path_factory.mktemp("regions_case")
    nml, grid = _write_netcdf_case(tmp, traj)
    ny, nx = grid.shape
    rng = np.random.default_rng(21)
    reg = rng.integers(0, 3, size=(ny, nx)).astype(np.int32) * 4 + 2   # ids 2, 6, 10
    reg.reshape(-1)[grid.index[rng.choice(grid.n, 5, replace=False)]] = -1  # unassigned land
    area = rng.uniform(0.5, 2.0, size=(ny, nx))
    regfile = str(tmp / "regions.nc")
    ncio.write_region_map(regfile, grid, reg, area)
    land_ids = reg.reshape(-1)[grid.index].astype(np.int64)
    land_w = area.reshape(-1)[grid.index]
    assert set(land_ids.tolist()) == {-1, 2, 6, 10}
    out = dict(nml=str(nml), grid=grid, regfile=regfile, ids=land_ids, w=land_w, tmp=tmp)
    for key, kw in (("r16", dict(regions=regfile)),
                    ("r35", dict(regions=regfile, accumulate=True)),
                    ("p16", dict()), ("p35", dict(accumulate=True)),
                    ("only35", dict(regions=regfile, accumulate=True, write_grids=False))):
        cfg = config.Config(str(nml))
        cfg.outdir = str(tmp / key)
        drv = driver.OfflineDriver.from_files(cfg, **kw).run()
        assert drv.step_index == 96
        out[key] = dict(outdir=cfg.outdir, perm=drv.perm.copy(), written=list(drv.written),
                        regions_written=list(drv.regions_written))
        drv.engine.close()
    return out


@pytest.mark.parametrize("key,names", [("r16", L.DIAG_OUT), ("r35", L.DIAG_OUT_ACC)])
def test_driver_regions_equal_the_tree_over_ldasout(case, key, names):
    """Every REGIONS file's means are the restated tree over the columns read
    back from the same time's LDASOUT file, in the engine's column order."""
    run, grid = case[key], case["grid"]
    perm = run["perm"]
    rids, ec, ew, c0 = make_plan(case["ids"][perm], case["w"][perm])
    wsum = tree(np.ones((1, grid.n)), ec, ew, c0, np.ones(len(rids)))[0][0]
    rfiles, lfiles = _regions_files(run["outdir"]), _ldasout_files(run["outdir"])
    assert len(rfiles) == len(lfiles) == 8 and rfiles == run["regions_written"]
    assert lfiles == run["written"]
    assert len(names) == (16 if key == "r16" else 35)
    for rf, lf in zip(rfiles, lfiles):
        assert os.path.basename(rf).split(".")[0] == os.path.basename(lf).split(".")[0]
        d = ncio.read_ldasout(lf, grid, names)
        assert d.dtype == np.float32
        want = tree(d[:, perm], ec, ew, c0, wsum)[1]
        r = ncio.read_regions(rf)
        assert r["names"] == list(names)
        assert r["region_id"].tolist() == [2, 6, 10] == rids.tolist()
        assert r["ncolumns"].tolist() == [int((case["ids"] == i).sum()) for i in (2, 6, 10)]
        assert same_bits(r["weight"], wsum)
        assert same_bits(r["means"], want), rf
    s = ncio.read_regions_series(run["outdir"])
    assert s["means"].shape == (8, len(names), 3)


def test_driver_regions_leave_ldasout_bytes_alone(case):
    for with_r, without in (("r16", "p16"), ("r35", "p35")):
        a, b = _ldasout_files(case[with_r]["outdir"]), _ldasout_files(case[without]["outdir"])
        assert len(a) == len(b) == 8
        for x, y in zip(a, b):
            assert os.path.basename(x) == os.path.basename(y)
            assert open(x, "rb").read() == open(y, "rb").read(), x
        assert not _regions_files(case[without]["outdir"])
        assert not case[without]["regions_written"]


def test_driver_regions_only(case, tmp_path):
    only, full = case["only35"], case["r35"]
    assert not _ldasout_files(only["outdir"]) and not only["written"]
    a, b = _regions_files(only["outdir"]), _regions_files(full["outdir"])
    assert len(a) == len(b) == 8
    for x, y in zip(a, b):
        assert os.path.basename(x) == os.path.basename(y)
        assert open(x, "rb").read() == open(y, "rb").read(), x
    cfg = config.Config(case["nml"])
    cfg.outdir = str(tmp_path / "none")
    with pytest.raises(ValueError):
        driver.OfflineDriver.from_files(cfg, write_grids=False)


def test_offline_cli_regions_only(case, tmp_path):
    """noahmp_offline.py --regions FILE --regions-only --accumulate writes the
    driver run's REGIONS bytes and no LDASOUT; --regions-only alone is refused."""
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("noahmp_offline",
                                                  os.path.join(root, "noahmp_offline.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    outdir = config.Config(case["nml"]).outdir
    text = open(case["nml"]).read()
    assert text.count(outdir) == 1
    nml = tmp_path / "cli.nml"
    nml.write_text(text.replace(outdir, str(tmp_path / "cli_out")))
    assert cli.main([str(nml), "--regions", case["regfile"], "--regions-only",
                     "--accumulate"]) == 0
    got, want = _regions_files(str(tmp_path / "cli_out")), _regions_files(case["r35"]["outdir"])
    assert len(got) == len(want) == 8 and not _ldasout_files(str(tmp_path / "cli_out"))
    for x, y in zip(got, want):
        assert open(x, "rb").read() == open(y, "rb").read(), x
    with pytest.raises(SystemExit):
        cli.main([str(nml), "--regions-only"])


def test_driver_regions_after_restart(case, tmp_path):
    """A run restarted mid-way (and mid-interval) writes the uninterrupted
    run's REGIONS bytes."""
    cfg = config.Config(case["nml"])
    cfg.outdir = str(tmp_path / "first")
    kw = dict(regions=case["regfile"], accumulate=True)
    a = driver.OfflineDriver.from_files(cfg, **kw).run(nsteps=40)
    path = str(tmp_path / "RESTART.nc")
    a.save_restart(path)
    a.engine.close()
    cfg.outdir = str(tmp_path / "second")
    b = driver.OfflineDriver.from_files(cfg, init=path, **kw)
    assert b.step_index == 40
    b.run()
    b.engine.close()
    want = _regions_files(case["r35"]["outdir"])
    got = _regions_files(cfg.outdir)
    assert [os.path.basename(f) for f in got] == [os.path.basename(f) for f in want[3:]]
    for x, y in zip(got, want[3:]):
        assert open(x, "rb").read() == open(y, "rb").read(), x


def test_driver_region_budget_closes(case):
    """Per region and interval the area-weighted water budget closes within
    the columns' own bound.  Each column's DSTOR, WBRES and six totals are
    fp32 roundings of doubles that satisfy the identity exactly and the
    identity is linear: nine half-ulp terms at most of the column's largest
    operand, weighted like the means; each of the eight region means carries
    the tree's (3 + 6 + nchunks) 2^-53 sum|v w| / wsum on top.  Derived, not
    measured."""
    run, grid = case["r35"], case["grid"]
    perm = run["perm"]
    names = L.DIAG_OUT_ACC
    rows = [names.index(n) for n in ("DSTOR", "ACCPRCP", "ACCECAN", "ACCETRAN", "ACCEDIR",
                                     "SFCRNOFF", "UGDRNOFF", "WBRES")]
    sign = [1, -1, 1, 1, 1, 1, 1, -1]   # DSTOR - (P - ECAN - ETRAN - EDIR - RSRF - RSUB) - WBRES
    ids, w = case["ids"], case["w"]
    u = 2.0 ** -53
    worst = 0.0
    for rf, lf in zip(_regions_files(run["outdir"]), _ldasout_files(run["outdir"])):
        r = ncio.read_regions(rf)
        d = ncio.read_ldasout(lf, grid, names)[rows].astype(np.float64)   # (8, n) land order
        for ri, rid in enumerate(r["region_id"]):
            c = np.flatnonzero(ids == rid)
            resid = sum(s * Fraction(float(r["means"][row, ri])) for s, row in zip(sign, rows))
            ulp = np.spacing(np.abs(d[:, c]).max(axis=0).astype(np.float32)).astype(np.float64)
            wsum = float(r["weight"][ri])
            cols_bound = float((w[c] * 9.0 * ulp).sum()) / wsum
            nchunks = -(-c.size // CH)
            tree_bound = sum((3 + 6 + nchunks) * u * float((np.abs(d[k, c]) * w[c]).sum()) / wsum
                             for k in range(8))
            assert abs(resid) <= Fraction(cols_bound + tree_bound), (rf, rid, float(resid))
            worst = max(worst, float(abs(resid)) / (cols_bound + tree_bound))
    print(f"largest |residual| / bound over 8 intervals x 3 regions: {worst:.3g}")


# ---- 3. two ranks -------------------------------------------------------------------
def _regions_rank(rank, world, port, nml, regfile):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    drv = driver.OfflineDriver.from_files(config.Config(nml), regions=regfile, accumulate=True)
    assert (drv.region_plan is not None) == (rank == 0)
    drv.run()
    dist.barrier()
    drv.engine.close()
    dist.destroy_process_group()


def test_two_ranks_write_the_single_rank_regions(case):
    """Rank 0 reduces the gathered block with the plan of the global column
    set: its REGIONS files are byte-equal to the single-rank run's."""
    import socket
    import torch.multiprocessing as mp
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    mp.start_processes(_regions_rank, args=(2, port, case["nml"], case["regfile"]), nprocs=2,
                       start_method="spawn")
    multi_dir = config.Config(case["nml"]).outdir
    multi, single = _regions_files(multi_dir), _regions_files(case["r35"]["outdir"])
    assert len(multi) == len(single) == 8
    for a, b in zip(multi, single):
        assert os.path.basename(a) == os.path.basename(b)
        assert open(a, "rb").read() == open(b, "rb").read(), a
    for a, b in zip(_ldasout_files(multi_dir), _ldasout_files(case["r35"]["outdir"])):
        assert open(a, "rb").read() == open(b, "rb").read(), a
