"""Interval extremes on the GPU: nmp_extremes_update / nmp_extremes_output
against their numpy restatement (extremes.update_host / output_host), and the
offline driver with extremes=... against values formed in numpy from the
reference's own trajectory (traj_casenml fixture), bit for bit: beside
accumulation, state output and regions, through restart files, after a spin-up
and on two ranks.

Bounds: every comparison is on bits; the kernels move values and compute only
(T)((double)when * dt), one rounded product and one conversion, which numpy
forms the same way."""
import datetime
import glob
import os

import numpy as np
import pytest
import torch

import noahmp_pkg  # noqa: F401  (spawned ranks re-import this module)
from golden_io import bit_equal, load
from noahmp_amd import cases, config, driver, extremes as X, layout as L, ncio, timeman
from noahmp_amd.engine import ColumnState, Engine
from noahmp_amd.params import Params
from test_gpu_accum import ACC_SHAPES

pytestmark = pytest.mark.gpu

NAN, INF = float("nan"), float("inf")
SPEC = "FSH,TRAD,T2M,RUNSRF:max+tmax,ALBEDO,PRCP:max+tmax,TG,SNEQV,SMC1,STC1"
SERIES = X.parse(SPEC)
NAMES = X.row_names(SERIES)
NEXT = len(NAMES)
assert NEXT == 20


def ibits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize])


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(ibits(a), ibits(b))


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda:0")


def _engine(precision):
    return Engine(Params.builtin(), L.CASE_NML_OPTIONS, device=0, precision=precision)


# ---- 1. the kernels against the restatement ---------------------------------------------
# one series of each kind and three more; the planted columns' values go into
# every series' source row
K_SERIES = [(L.EXT_SRC_DIAG, 3), (L.EXT_SRC_FORCING, 8), (L.EXT_SRC_STATE, 29),
            (L.EXT_SRC_DIAG, 15), (L.EXT_SRC_STATE, 55), (L.EXT_SRC_FORCING, 0)]
K_STATS = [1 | 2, 1 | 4, 15, 8, 2 | 4, 4 | 8]
PLANTED = {
    "tied_max_2_4": [1, 5, 3, 5, 2, 0],
    "nan_then_numbers": [NAN, 2, 1, 3, NAN, 2],
    "numbers_then_nan": [2, 3, NAN, NAN, 1, NAN],
    "all_nan": [NAN] * 6,
    "pzero_then_nzero": [0.0, -0.0, 0.0, -0.0, 0.0, -0.0],
    "nzero_then_pzero": [-0.0, 0.0, -0.0, 0.0, -0.0, 0.0],
    "infinities": [1, INF, 2, INF, -INF, -INF],
    "rising": [1, 2, 3, 4, 5, 6],
    "falling": [6, 5, 4, 3, 2, 1],
}


@pytest.mark.parametrize("ld,lo,hi", ACC_SHAPES + [(1, 0, 1), (70, 69, 70)])
@pytest.mark.parametrize("precision", [4, 8])
def test_kernels_equal_the_restatement(engine_lib, precision, ld, lo, hi):
    eng = _engine(precision)
    dtype = np.float32 if precision == 4 else np.float64
    rng = np.random.default_rng(100 * precision + ld)
    ns = len(K_SERIES)
    nrow = sum(bin(m).count("1") for m in K_STATS)
    val0 = rng.normal(size=(2 * ns, ld)).astype(dtype)
    when0 = rng.integers(-9, 99, size=(2 * ns, ld)).astype(np.int32)
    val, when = _dev(val0), _dev(when0)
    want_v, want_w = val0.copy(), when0.copy()
    out0 = rng.normal(size=(nrow + 3, ld)).astype(dtype)     # a block: the rows are 1..nrow
    col = {name: lo + j for j, name in enumerate(PLANTED) if lo + j < hi}
    assert len(col) == len(PLANTED) or hi - lo == 1
    for k in range(1, 7):
        diag = rng.normal(size=(16, ld)).astype(dtype)
        forcing = rng.normal(size=(12, ld)).astype(dtype)
        state = rng.normal(size=(56, ld)).astype(dtype)
        blocks = {L.EXT_SRC_DIAG: diag, L.EXT_SRC_FORCING: forcing, L.EXT_SRC_STATE: state}
        if k > 1:   # random ties as well: a quarter of the columns repeat the last step's values
            rep = rng.random(ld) < 0.25
            for kind, b in blocks.items():
                b[:, rep] = prev[kind][:, rep]
        prev = {kind: b.copy() for kind, b in blocks.items()}
        for kind, row in K_SERIES:
            for name, c in col.items():
                blocks[kind][row, c] = PLANTED[name][k - 1]
        d, f, s = _dev(diag), _dev(forcing), _dev(state)
        eng.extremes_update(K_SERIES, k, val, when, d, f, s, cols=(lo, hi))
        X.update_host(want_v[:, lo:hi], want_w[:, lo:hi], k, K_SERIES, diag[:, lo:hi],
                      forcing[:, lo:hi], state[:, lo:hi])
        block = _dev(out0)
        eng.extremes_output(K_STATS, 900.0, val, when, block[1:1 + nrow], cols=(lo, hi))
        torch.cuda.synchronize()
        got_v, got_w, got_o = val.cpu().numpy(), when.cpu().numpy(), block.cpu().numpy()
        assert same_bits(got_v[:, lo:hi], want_v[:, lo:hi]), k
        assert np.array_equal(got_w[:, lo:hi], want_w[:, lo:hi]), k
        # outside the range nothing moved; the output left val and when alone
        assert same_bits(got_v[:, :lo], val0[:, :lo]) and same_bits(got_v[:, hi:], val0[:, hi:])
        assert np.array_equal(got_w[:, :lo], when0[:, :lo])
        assert np.array_equal(got_w[:, hi:], when0[:, hi:])
        want_o = X.output_host(want_v[:, lo:hi], want_w[:, lo:hi], K_STATS, 900.0)
        assert same_bits(got_o[1:1 + nrow, lo:hi], want_o), k
        assert same_bits(got_o[0], out0[0]) and same_bits(got_o[1 + nrow:], out0[1 + nrow:])
        assert same_bits(got_o[:, :lo], out0[:, :lo]) and same_bits(got_o[:, hi:], out0[:, hi:])
        # the inputs are read only
        assert same_bits(d.cpu().numpy(), diag) and same_bits(f.cpu().numpy(), forcing)
        assert same_bits(s.cpu().numpy(), state)
    if len(col) == len(PLANTED):   # the restatement itself, on the planted columns
        c = col["tied_max_2_4"]
        assert want_v[0, c] == 5 and want_w[0, c] == 2
        c = col["all_nan"]
        assert np.isnan(want_v[:, c]).all() and (want_w[:, c] == 1).all()
        c = col["numbers_then_nan"]
        assert (want_v[0, c], want_w[0, c], want_v[1, c], want_w[1, c]) == (3, 2, 1, 5)
        assert ibits(want_v[:2, col["pzero_then_nzero"]]).tolist() == [0, 0]
        assert (ibits(want_v[:2, col["nzero_then_pzero"]]) < 0).all()
        assert (want_w[:2, col["nzero_then_pzero"]] == 1).all()
    eng.close()


def test_blocks_no_series_names_may_be_null(engine_lib):
    eng = _engine(4)
    rng = np.random.default_rng(5)
    n = 130
    state = rng.normal(size=(56, n)).astype(np.float32)
    forcing = rng.normal(size=(12, n)).astype(np.float32)
    val = torch.zeros((4, n), device="cuda:0")
    when = torch.zeros((4, n), dtype=torch.int32, device="cuda:0")
    kr = [(L.EXT_SRC_STATE, 37), (L.EXT_SRC_FORCING, 8)]
    eng.extremes_update(kr, 1, val, when, None, _dev(forcing), _dev(state))
    torch.cuda.synchronize()
    assert same_bits(val.cpu().numpy(), np.stack([state[37], state[37], forcing[8], forcing[8]]))
    assert (when.cpu().numpy() == 1).all()
    # refused with nothing enqueued: a missing block a series names, k < 1, a bad kind or row
    from noahmp_amd.lib import NmpError
    before = val.cpu().numpy()
    for kw in (dict(state=None), dict(forcing=None), dict(k=0), dict(kr=[(3, 0), (1, 8)]),
               dict(kr=[(2, 56), (1, 8)])):
        a = dict(kr=kr, k=2, forcing=_dev(forcing + 1), state=_dev(state + 1))
        a.update(kw)
        with pytest.raises(NmpError) as e:
            eng.extremes_update(a["kr"], a["k"], val, when, None, a["forcing"], a["state"])
        assert e.value.code == -1
    for stats, dt in (([0, 1], 900.0), ([1, 16], 900.0), ([1, 1], 0.0), ([1, 1], NAN)):
        with pytest.raises(NmpError) as e:
            eng.extremes_output(stats, dt, val, when, torch.zeros((2, n), device="cuda:0"))
        assert e.value.code == -1
    eng.extremes_update(kr, 3, val, when, None, _dev(forcing), _dev(state), cols=(7, 7))  # ncol 0
    torch.cuda.synchronize()
    assert same_bits(val.cpu().numpy(), before)
    eng.close()


# ---- the driver: shared runs ---------------------------------------------------------------
def _cols(g, state=None, isnow=None):
    return cases.ColumnSet(g["static_f"], g["static_i"], g["state0"] if state is None else state,
                           g["isnow0"] if isnow is None else isnow, *([None] * 7))


def _cfg(tmp_path, sub="out"):
    from test_config import write_case
    cfg = config.Config(write_case(tmp_path))
    cfg.outdir = str(tmp_path / sub)
    return cfg


def _npz_files(outdir):
    return sorted(glob.glob(os.path.join(outdir, "*.LDASOUT.npz")))


def _npz_members(path):
    with np.load(path, allow_pickle=False) as z:
        return {k: (z[k].dtype.str, z[k].shape, z[k].tobytes()) for k in z.files}


def _netcdf_files(outdir):
    return sorted(glob.glob(os.path.join(outdir, "*.LDASOUT_DOMAIN1")))


def _regions_files(outdir):
    return sorted(glob.glob(os.path.join(outdir, "*.REGIONS_DOMAIN1")))


@pytest.fixture(scope="module")
def traj():
    return load("traj_casenml.npz")


def _twin(g, precision, nsteps, state=None, isnow=None):
    """A plain engine run of the fixture's columns: per step the 16 output
    fluxes and the state the step left."""
    eng = _engine(precision)
    dt = torch.float32 if precision == 4 else torch.float64
    cs = ColumnState.from_host(_cols(g, state, isnow), "cuda:0", dt)
    diag = torch.zeros((16, 32), device="cuda:0", dtype=dt)
    t, diags, states = datetime.datetime(2000, 1, 1), [], []
    for k in range(nsteps):
        f = _dev(g["forcing"][k]).to(dt)
        eng.step(cs, f, cases.CASE_NML_ZSOIL, 900.0, timeman.julian(t), timeman.yearlen(t.year),
                 diag, L.DIAG_OUT_LEVEL)
        diags.append(diag.cpu().numpy().copy())
        states.append(cs.state.cpu().numpy().copy())
        t = t + datetime.timedelta(seconds=900)
    eng.close()
    return diags, states


@pytest.fixture(scope="module")
def twin32(engine_lib, traj):
    diags, states = _twin(traj, 4, 96)
    assert bit_equal(states[-1], traj["states"][-1]).all()
    return diags, states


def _ref_step(g, twin32, k):
    """(diag16, forcing, state) of step k from the reference's trajectory, T2M
    (which the reference's argument list does not have) from the twin run."""
    diag = np.stack([twin32[0][k][i] if n == "T2M" else g["diags"][k][L.DIAG_FULL.index(n)]
                     for i, n in enumerate(L.DIAG_OUT)])
    return diag, g["forcing"][k], g["states"][k]


def _want_rows(steps, series=SERIES, dtype=np.float32, k0=1):
    """The extremes rows of an interval from its steps' (diag, forcing, state)."""
    n = steps[0][0].shape[1]
    val, when = np.zeros((2 * len(series), n), dtype), np.zeros((2 * len(series), n), np.int32)
    for k, (d, f, s) in enumerate(steps, k0):
        X.update_host(val, when, k, X.pairs(series), d, f, s)
    return X.output_host(val, when, X.masks(series), 900.0)


@pytest.fixture(scope="module")
def ext_run(engine_lib, traj, tmp_path_factory):
    """The uninterrupted run of the trajectory's 96 steps with SPEC (npz
    output, two ranges of 16 columns) and the same run without the option."""
    tmp = tmp_path_factory.mktemp("ext_run")
    res = {}
    for key, kw in (("ext", dict(extremes=SPEC)), ("plain", dict())):
        cfg = _cfg(tmp, key)
        drv = driver.OfflineDriver(cfg, _cols(traj), forcing=lambda step, t: traj["forcing"][step],
                                   **kw)
        assert [hi - lo for lo, hi in drv.ranges.ranges] == [16, 16]
        drv.run()
        assert drv.step_index == 96
        files = _npz_files(cfg.outdir)
        assert len(files) == 8
        res[key] = dict(files=files, state=drv.cs.state.cpu().numpy(),
                        isnow=drv.cs.isnow.cpu().numpy(), names=list(drv.out_names))
        drv.engine.close()
    return res


# ---- 2. the driver against the reference trajectory ------------------------------------------
def _series_steps(g, twin32, s, j):
    """(12, 32) values of series s over interval j, from the reference's data."""
    blocks = [_ref_step(g, twin32, k) for k in range(12 * j, 12 * j + 12)]
    return np.stack([b[s.kind][s.row] for b in blocks])


def test_reference_data_shows_the_feature(traj, twin32):
    """On the reference's data alone: every series' interval maximum differs
    from the output step's value somewhere, and RUNSRF, PRCP and SNEQV have
    tied maxima (the first-occurrence rule is exercised)."""
    assert not any(np.isnan(traj[k]).any() for k in ("diags", "forcing", "states"))
    for s in SERIES:
        differs, tied = 0, 0
        for j in range(8):
            v = _series_steps(traj, twin32, s, j)
            differs += int((v.max(0) != v[-1]).sum())
            tied += int(((v == v.max(0)).sum(0) > 1).sum())
        print(f"{s.name}: max differs from the output step in {differs} of 256, tied in {tied}")
        assert differs >= 1, s.name
        if s.name in ("RUNSRF", "PRCP", "SNEQV"):
            assert tied >= 1, s.name


def test_driver_extremes_equal_reference_trajectory(ext_run, twin32, traj):
    g = traj
    assert ext_run["ext"]["names"] == L.DIAG_OUT + NAMES
    assert bit_equal(ext_run["ext"]["state"], g["states"][-1]).all()
    assert np.array_equal(ext_run["ext"]["isnow"], g["isnows"][-1])
    assert same_bits(ext_run["ext"]["state"], ext_run["plain"]["state"])
    for j, (fe, fp) in enumerate(zip(ext_run["ext"]["files"], ext_run["plain"]["files"])):
        assert os.path.basename(fe) == os.path.basename(fp)
        with np.load(fe, allow_pickle=False) as z:
            d, fields = z["diag"], str(z["fields"]).split(",")
        with np.load(fp, allow_pickle=False) as z:
            d16 = z["diag"]
        assert fields == L.DIAG_OUT + NAMES and d.shape == (16 + NEXT, 32)
        assert d.dtype == np.float32
        assert same_bits(d[:16], d16), f"file {j}: the output step's fluxes changed"
        steps = [_ref_step(g, twin32, k) for k in range(12 * j, 12 * j + 12)]
        want = _want_rows(steps)
        for i, name in enumerate(NAMES):
            assert same_bits(d[16 + i], want[i]), (j, name)
        for s in SERIES:
            v = _series_steps(g, twin32, s, j)
            if s.stats & L.EXT_MAX:
                assert np.array_equal(d[fields.index(f"{s.name}_MAX")], v.max(0)), (j, s.name)
            if s.stats & L.EXT_MIN:
                assert np.array_equal(d[fields.index(f"{s.name}_MIN")], v.min(0)), (j, s.name)
            if s.stats & L.EXT_TMAX:
                first = np.argmax(v == v.max(0), axis=0)
                assert np.array_equal(d[fields.index(f"{s.name}_TMAX")],
                                      (900.0 * (1 + first)).astype(np.float32)), (j, s.name)


# ---- 3. beside accumulation, state output and regions ------------------------------------------
@pytest.fixture(scope="module")
def case(engine_lib, traj, tmp_path_factory):
    """The trajectory's netCDF case with a region file, run with accumulate,
    state_out and regions, with and without extremes."""
    from test_gpu_driver import _write_netcdf_case
    tmp = tmp_path_factory.mktemp("ext_case")
    nml, grid = _write_netcdf_case(tmp, traj)
    ny, nx = grid.shape
    rng = np.random.default_rng(21)
    reg = rng.integers(0, 3, size=(ny, nx)).astype(np.int32) * 4 + 2
    reg.reshape(-1)[grid.index[rng.choice(grid.n, 5, replace=False)]] = -1
    area = rng.uniform(0.5, 2.0, size=(ny, nx))
    regfile = str(tmp / "regions.nc")
    ncio.write_region_map(regfile, grid, reg, area)
    out = dict(nml=str(nml), grid=grid, regfile=regfile, tmp=tmp,
               ids=reg.reshape(-1)[grid.index].astype(np.int64), w=area.reshape(-1)[grid.index])
    common = dict(accumulate=True, state_out="SOIL_M,SNOW_T", regions=regfile)
    for key, kw in (("with", dict(common, extremes=SPEC)), ("without", common),
                    ("only", dict(extremes=SPEC))):
        cfg = config.Config(str(nml))
        cfg.outdir = str(tmp / key)
        drv = driver.OfflineDriver.from_files(cfg, **kw).run()
        assert drv.step_index == 96
        out[key] = dict(outdir=cfg.outdir, perm=drv.perm.copy(), names=list(drv.out_names))
        drv.engine.close()
    return out


def test_composition_rows_and_regions(case, ext_run):
    from noahmp_amd import stateout
    from noahmp_amd.regions import RegionPlan
    grid, perm = case["grid"], case["with"]["perm"]
    srows = stateout.row_names(stateout.parse_groups("SOIL_M,SNOW_T"))
    names = case["with"]["names"]
    assert names == L.DIAG_OUT + L.BUDGET + NAMES + srows
    assert case["without"]["names"] == L.DIAG_OUT + L.BUDGET + srows
    a, b = _netcdf_files(case["with"]["outdir"]), _netcdf_files(case["without"]["outdir"])
    assert len(a) == len(b) == 8
    plan = RegionPlan.from_ids(case["ids"][perm], case["w"][perm])
    nred = 35 + NEXT + 4
    ra, rb = _regions_files(case["with"]["outdir"]), _regions_files(case["without"]["outdir"])
    assert len(ra) == len(rb) == 8
    for j, (x, y) in enumerate(zip(a, b)):
        dx = ncio.read_ldasout(x, grid, names)
        dy = ncio.read_ldasout(y, grid, case["without"]["names"])
        assert same_bits(dx[:35], dy[:35]), x                  # fluxes and budget rows
        assert same_bits(dx[35 + NEXT:], dy[35:]), x           # state rows
        # the extremes rows are the npz run's, in grid order
        with np.load(ext_run["ext"]["files"][j], allow_pickle=False) as z:
            assert same_bits(dx[35:35 + NEXT], z["diag"][16:]), x
        # the raw bytes too: each variable's grid, fill included
        rx, ry = ncio.read_ldasin(x), ncio.read_ldasin(y)
        assert list(rx) == L.DIAG_OUT + L.BUDGET + NAMES + ["SOIL_M", "SNOW_T"]
        for name in ry:
            assert np.asarray(rx[name]).tobytes() == np.asarray(ry[name]).tobytes(), (x, name)
        # REGIONS: the extremes rows ride along, the fill-capable SNOW_T rows do not
        r, r0 = ncio.read_regions(ra[j]), ncio.read_regions(rb[j])
        assert r["names"] == names[:nred] and r0["names"] == case["without"]["names"][:39]
        want = plan.reduce_host(dx[:nred, perm])[1]
        assert same_bits(r["means"], want), ra[j]
        assert same_bits(r["means"][:35], r0["means"][:35])
        assert same_bits(r["means"][35 + NEXT:], r0["means"][35:])
    # extremes alone on the grid: the same rows after the 16 fluxes
    c = _netcdf_files(case["only"]["outdir"])
    assert case["only"]["names"] == L.DIAG_OUT + NAMES and len(c) == 8
    for j, x in enumerate(c):
        with np.load(ext_run["ext"]["files"][j], allow_pickle=False) as z:
            assert same_bits(ncio.read_ldasout(x, grid, case["only"]["names"]), z["diag"]), x


def _record_steps(drv):
    """Every ranges.step call's (diag_level, the diag block's address)."""
    calls, step = [], drv.ranges.step

    def spy(forcing, zsoil, dt, julian, yearlen, diag=None, diag_level=L.DIAG_NONE, **kw):
        calls.append((diag_level, None if diag is None else diag.data_ptr()))
        return step(forcing, zsoil, dt, julian, yearlen, diag, diag_level, **kw)
    drv.ranges.step = spy
    return calls


def test_steps_between_outputs_keep_their_diag_level(engine_lib, traj, tmp_path):
    ff = lambda step, t: traj["forcing"][step]  # noqa: E731
    # state and forcing series only: the steps between output steps write no fluxes
    drv = driver.OfflineDriver(_cfg(tmp_path, "sf"), _cols(traj), forcing=ff,
                               extremes="PRCP:max+tmax,TG,SNEQV,SMC1,STC1")
    assert drv.block.scratch is None and not drv.extremes.need_diag
    calls = _record_steps(drv)
    drv.run(nsteps=25)
    drv.engine.close()
    assert [c[0] for c in calls] == ([L.DIAG_NONE] * 11 + [L.DIAG_OUT_LEVEL]) * 2 + [L.DIAG_NONE]
    assert all(c[1] is None for c in calls if c[0] == L.DIAG_NONE)
    # a flux series: every step writes its fluxes, between output steps into one scratch block
    drv = driver.OfflineDriver(_cfg(tmp_path, "d"), _cols(traj), forcing=ff, extremes="FSH,TG")
    calls = _record_steps(drv)
    drv.run(nsteps=25)
    scratch, block = drv.block.scratch.data_ptr(), drv.diag.data_ptr()
    drv.engine.close()
    assert [c[0] for c in calls] == [L.DIAG_OUT_LEVEL] * 25
    assert [c[1] for c in calls] == ([scratch] * 11 + [block]) * 2 + [scratch]
    # with accumulation the scratch block is accumulation's: one every-step flux write
    drv = driver.OfflineDriver(_cfg(tmp_path, "da"), _cols(traj), forcing=ff, extremes="FSH,TG",
                               accumulate=True)
    assert not hasattr(drv.extremes, "scratch") and not hasattr(drv.accum, "acc_diag")
    calls = _record_steps(drv)
    drv.run(nsteps=25)
    scratch, block = drv.block.scratch.data_ptr(), drv.diag.data_ptr()
    drv.engine.close()
    assert [c[0] for c in calls] == [L.DIAG_OUT_LEVEL] * 25
    assert [c[1] for c in calls] == ([scratch] * 11 + [block]) * 2 + [scratch]
    # the option off: as ever
    drv = driver.OfflineDriver(_cfg(tmp_path, "off"), _cols(traj), forcing=ff)
    assert drv.extremes is None
    calls = _record_steps(drv)
    drv.run(nsteps=13)
    drv.engine.close()
    assert [c[0] for c in calls] == [L.DIAG_NONE] * 11 + [L.DIAG_OUT_LEVEL] + [L.DIAG_NONE]


# ---- 4. restart inside an interval ---------------------------------------------------------
def test_restart_mid_interval_npz(ext_run, twin32, traj, tmp_path):
    g = traj
    ff = lambda step, t: g["forcing"][step]  # noqa: E731
    a = driver.OfflineDriver(_cfg(tmp_path, "first"), _cols(g), forcing=ff, extremes=SPEC)
    a.run(nsteps=40)
    assert a.extremes.k == 4
    path = str(tmp_path / "r.npz")
    a.save_restart(path)
    a.engine.close()
    with np.load(path) as z:
        assert str(z["ext_spec"]) == X.spec_string(SERIES) and int(z["ext_steps"]) == 4
        assert z["ext_val"].shape == z["ext_when"].shape == (2 * len(SERIES), 32)
    cfg = _cfg(tmp_path, "second")
    b = driver.OfflineDriver(cfg, _cols(g), forcing=ff, extremes=SPEC)
    b.load_restart(path)
    assert b.step_index == 40 and b.extremes.k == 4
    b.run()
    assert bit_equal(b.cs.state.cpu().numpy(), g["states"][-1]).all()
    b.engine.close()
    files = _npz_files(cfg.outdir)
    assert [os.path.basename(f) for f in files] == \
        [os.path.basename(f) for f in ext_run["ext"]["files"][3:]]
    for got, want in zip(files, ext_run["ext"]["files"][3:]):
        assert _npz_members(got) == _npz_members(want), got
    # a restart without the arrays, and one taken with another spec, start a fresh interval
    plain = driver.OfflineDriver(_cfg(tmp_path, "p"), _cols(g), forcing=ff, write=False)
    plain.run(nsteps=40)
    p2 = str(tmp_path / "plain.npz")
    plain.save_restart(p2)
    plain.engine.close()
    assert "ext_val" not in np.load(p2).files
    other = driver.OfflineDriver(_cfg(tmp_path, "o"), _cols(g), forcing=ff, extremes="TG,FSH")
    other.run(nsteps=40)
    p3 = str(tmp_path / "other.npz")
    other.save_restart(p3)
    other.engine.close()
    steps = [_ref_step(g, twin32, k) for k in range(40, 48)]
    want = _want_rows(steps)
    for sub, rpath in (("third", p2), ("fourth", p3)):
        cfg = _cfg(tmp_path, sub)
        c = driver.OfflineDriver(cfg, _cols(g), forcing=ff, extremes=SPEC)
        c.load_restart(rpath)
        assert c.step_index == 40 and c.extremes.k == 0
        c.run(nsteps=8)
        c.engine.close()
        with np.load(_npz_files(cfg.outdir)[0], allow_pickle=False) as z:
            d = z["diag"]
        for i, name in enumerate(NAMES):
            assert same_bits(d[16 + i], want[i]), (sub, name)
        # the times count from the restart: at most 8 steps
        assert (d[16 + NAMES.index("PRCP_TMAX")] <= 8 * 900.0).all()


def test_restart_mid_interval_netcdf(case, twin32, traj, tmp_path):
    grid = case["grid"]
    cfg = config.Config(case["nml"])
    cfg.outdir = str(tmp_path / "first")
    a = driver.OfflineDriver.from_files(cfg, extremes=SPEC).run(nsteps=40)
    path = str(tmp_path / "RESTART.nc")
    a.save_restart(path)
    a.engine.close()
    got = ncio.read_extremes(path, grid)
    assert got is not None and got[2] == 4 and got[3] == X.spec_string(SERIES)
    cfg.outdir = str(tmp_path / "second")
    b = driver.OfflineDriver.from_files(cfg, init=path, extremes=SPEC)
    assert b.step_index == 40 and b.extremes.k == 4
    b.run()
    b.engine.close()
    files, want = _netcdf_files(cfg.outdir), _netcdf_files(case["only"]["outdir"])
    assert [os.path.basename(f) for f in files] == [os.path.basename(f) for f in want[3:]]
    for x, y in zip(files, want[3:]):
        assert open(x, "rb").read() == open(y, "rb").read(), x
    # load_restart of the same file into a constructed driver resumes it as well
    cfg.outdir = str(tmp_path / "third")
    c = driver.OfflineDriver.from_files(cfg, extremes=SPEC)
    c.load_restart(path)
    assert c.step_index == 40 and c.extremes.k == 4
    c.run(nsteps=8)
    c.engine.close()
    x = _netcdf_files(cfg.outdir)
    assert len(x) == 1 and open(x[0], "rb").read() == open(want[3], "rb").read()
    # a run without the option ignores the restart's extra variables
    cfg.outdir = str(tmp_path / "plain")
    p = driver.OfflineDriver.from_files(cfg, init=path, write=False).run()
    assert bit_equal(p.to_grid_order(p.cs.state.cpu().numpy()), traj["states"][-1]).all()
    p.engine.close()
    # a netCDF restart without the variables starts a fresh interval there
    p = driver.OfflineDriver.from_files(cfg, write=False).run(nsteps=40)
    bare = str(tmp_path / "BARE.nc")
    p.save_restart(bare)
    p.engine.close()
    assert ncio.read_extremes(bare, grid) is None
    cfg.outdir = str(tmp_path / "fourth")
    d = driver.OfflineDriver.from_files(cfg, init=bare, extremes=SPEC)
    assert d.step_index == 40 and d.extremes.k == 0
    d.run(nsteps=8)
    d.engine.close()
    x = _netcdf_files(cfg.outdir)
    assert len(x) == 1
    got = ncio.read_ldasout(x[0], grid, L.DIAG_OUT + NAMES)
    want_rows = _want_rows([_ref_step(traj, twin32, k) for k in range(40, 48)])
    for i, name in enumerate(NAMES):
        assert same_bits(got[16 + i], want_rows[i]), name


# ---- 5. spin-up, then the run ---------------------------------------------------------------
def test_spinup_then_run_starts_a_fresh_interval(engine_lib, traj, tmp_path):
    g = traj
    ff = lambda step, t: g["forcing"][step]  # noqa: E731
    a = driver.OfflineDriver(_cfg(tmp_path, "spun"), _cols(g), forcing=ff, extremes=SPEC)
    a.spinup(2, report=False)
    assert a.extremes.k == 0 and a.step_index == 0
    state, isnow = a.cs.state.cpu().numpy(), a.cs.isnow.cpu().numpy()
    assert not bit_equal(state, g["state0"]).all()
    a.run(nsteps=12)
    a.engine.close()
    cfg = _cfg(tmp_path, "fresh")
    b = driver.OfflineDriver(cfg, _cols(g, state, isnow), forcing=ff, extremes=SPEC)
    b.run(nsteps=12)
    b.engine.close()
    fa, fb = _npz_files(str(tmp_path / "spun")), _npz_files(cfg.outdir)
    assert len(fa) == len(fb) == 1
    assert _npz_members(fa[0]) == _npz_members(fb[0])
    # and they are the restatement's on a twin run from the spun-up state
    diags, states = _twin(g, 4, 12, state, isnow)
    want = _want_rows([(diags[k], g["forcing"][k], states[k]) for k in range(12)])
    with np.load(fa[0], allow_pickle=False) as z:
        assert same_bits(z["diag"][16:], want)


# ---- 6. two ranks ---------------------------------------------------------------------------
def _extremes_rank(rank, world, port, nml):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    drv = driver.OfflineDriver.from_files(config.Config(nml), extremes=SPEC)
    assert drv.gather.nfield == 16 + NEXT
    drv.run()
    dist.barrier()
    drv.engine.close()
    dist.destroy_process_group()


def test_two_ranks_write_the_single_rank_files(case):
    import socket
    import torch.multiprocessing as mp
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    mp.start_processes(_extremes_rank, args=(2, port, case["nml"]), nprocs=2, start_method="spawn")
    multi = _netcdf_files(config.Config(case["nml"]).outdir)
    single = _netcdf_files(case["only"]["outdir"])
    assert len(multi) == len(single) == 8
    for a, b in zip(multi, single):
        assert os.path.basename(a) == os.path.basename(b)
        assert open(a, "rb").read() == open(b, "rb").read(), a


# ---- 7. fp64 ---------------------------------------------------------------------------------
def test_fp64_driver_equals_the_restatement(engine_lib, traj, tmp_path):
    g = traj
    cfg = _cfg(tmp_path)
    drv = driver.OfflineDriver(cfg, _cols(g), forcing=lambda step, t: g["forcing"][step],
                               precision=8, extremes=SPEC)
    drv.run(nsteps=12)
    drv.engine.close()
    files = _npz_files(cfg.outdir)
    assert len(files) == 1
    with np.load(files[0], allow_pickle=False) as z:
        d = z["diag"]
    assert d.dtype == np.float64 and d.shape == (16 + NEXT, 32)
    diags, states = _twin(g, 8, 12)
    assert same_bits(d[:16], diags[11])
    steps = [(diags[k], g["forcing"][k].astype(np.float64), states[k]) for k in range(12)]
    want = _want_rows(steps, dtype=np.float64)
    for i, name in enumerate(NAMES):
        assert same_bits(d[16 + i], want[i]), name
    # the values are fp64 values of their own, not widened fp32 ones
    assert (d[16 + NAMES.index("FSH_MAX")].astype(np.float32).astype(np.float64)
            != d[16 + NAMES.index("FSH_MAX")]).any()
