"""The step kernel on the rare physics branches, against the reference Fortran.

tests/golden/branch_*.npz (tests/golden/make_branch_golden.py) are columns on
which the reference itself takes the branches no plausible-climate fixture
reaches (snow caps, sign cases of the snow-layer bookkeeping, the C4 pathway,
a water table inside the soil column, ...); tests/test_branch_golden.py proves
with the marker build of the restatement that they are taken.  With the
default ("ref") math the fp32 kernel must reproduce those columns bit for bit
-- in both occupancy instantiations, in the compiled option sets and in the
run-time-options kernel, at every diagnostics level, through nmp_step,
nmp_run_out and nmp_sflx_columns.  The fp64 kernel is held to the fp64
restatement by the rule of test_single_call_fp64_vs_fp64_oracle.
"""
import numpy as np
import pytest
import torch

from golden_io import (FP64_DIAG_ENV, FP64_STATE_ENV, as_ref_status, bit_equal, check_fp64_rule,
                       column_mismatch, fixture_ensemble, fixture_params, load)
from noahmp_amd import cases, layout as L
from test_branch_golden import SINGLES, traj_julian

pytestmark = pytest.mark.gpu

STATE_NAMES = [f"{n}[{k}]" if w > 1 else n for n, w in L.STATE_FIELDS for k in range(w)]
DEV = "cuda:0"
VARIANTS = ["small", "full"]
FP64_RECORDS = []   # golden_io.check_fp64_rule's records of this session


@pytest.fixture(scope="module")
def engines(engine_lib):
    """Engines per (fixture, precision, launch variant, forced set 0), built
    from the fixture's own table values."""
    yield from engine_cache()


def engine_cache():
    from noahmp_amd.engine import Engine
    from noahmp_amd.params import Params
    cache = {}

    def get(name, precision=4, variant="auto", set0=False):
        key = (name, precision, variant, set0)
        if key not in cache:
            g = load(f"branch_{name}.npz")
            eng = Engine(Params.from_dict(fixture_params(g)),
                         dict(zip(L.OPTION_NAMES, (int(x) for x in g["options"]))), device=0,
                         precision=precision, math="ref")
            assert eng.launch_variant(variant) == variant
            if set0:
                assert eng.option_set(0) == 0 and eng.option_set() == 0
            cache[key] = eng
        return cache[key]
    yield get
    for eng in cache.values():
        eng.close()


def run_single(eng, g, dtype=torch.float32, level=L.DIAG_FULL_LEVEL):
    from noahmp_amd.engine import ColumnState
    cols = cases.ColumnSet(g["static_f"], g["static_i"], g["state0"], g["isnow0"], *([None] * 7))
    cs = ColumnState.from_host(cols, DEV, dtype)
    f = torch.as_tensor(g["forcing"], device=DEV).to(dtype).contiguous()
    diag = None
    if level == L.DIAG_FULL_LEVEL:
        diag = torch.zeros((L.NDIAG_FULL, cs.ncol), dtype=dtype, device=DEV)
    eng.step(cs, f, g["zsoil"], float(g["dt"]), float(g["julian"]), int(g["yearlen"]), diag, level)
    torch.cuda.synchronize()
    return (cs.state.cpu().numpy(), cs.isnow.cpu().numpy(),
            None if diag is None else diag.cpu().numpy(), cs.status.cpu().numpy())


def assert_bit_exact(what, st, isn, dg, status, est, eisn, edg, estatus):
    exact = bit_equal(st, est).all(0) & bit_equal(dg, edg).all(0) & (isn == eisn) & \
        (as_ref_status(status) == estatus)
    _, rep_s = column_mismatch(st, est, 0, 0, STATE_NAMES)
    _, rep_d = column_mismatch(dg, edg, 0, 0, L.DIAG_FULL)
    print(what, "bit-exact columns", exact.mean())
    assert exact.all(), \
        f"{what}: {(~exact).sum()} columns differ from the reference " \
        f"(first {list(np.nonzero(~exact)[0][:8])}): " + "; ".join(rep_s[:8] + rep_d[:8])


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", SINGLES)
def test_branch_single_bit_exact_vs_reference(engines, name, variant):
    """Every column of every branch fixture: state, the 58 outputs, ISNOW and
    status are the reference's bits, on both occupancy kernels of the option
    set the fixture selects (set 1, set 2, run-time options)."""
    g = load(f"branch_{name}.npz")
    eng = engines(name, variant=variant)
    assert eng.option_set() == {"base": 1, "veg2": 2, "combo": 0}[name]
    assert_bit_exact(f"{name}/{variant}", *run_single(eng, g), g["state1"], g["isnow1"], g["diag"],
                     g["status"])


@pytest.mark.parametrize("name", ["base", "veg2"])
def test_branch_run_time_options_kernel_bit_exact(engines, name):
    """The run-time-options kernel (set 0 forced) takes the same branches."""
    g = load(f"branch_{name}.npz")
    assert_bit_exact(f"{name}/set0", *run_single(engines(name, set0=True), g), g["state1"],
                     g["isnow1"], g["diag"], g["status"])


@pytest.mark.parametrize("variant", VARIANTS)
def test_branch_state_independent_of_diag_level(engines, variant):
    """Without diagnostics the kernel skips the 2-m chain; the state bits on the
    branch columns are the same (the property of test_diag_levels_consistent)."""
    g = load("branch_base.npz")
    eng = engines("base", variant=variant)
    full = run_single(eng, g)
    none = run_single(eng, g, level=L.DIAG_NONE)
    assert bit_equal(none[0], full[0]).all() and np.array_equal(none[1], full[1])
    assert np.array_equal(none[3], full[3])
    assert bit_equal(none[0], g["state1"]).all()


@pytest.mark.parametrize("variant", VARIANTS)
def test_branch_trajectory_steps_bit_exact(engines, variant):
    """8 nmp_step calls over the snow columns whose layers combine in step 1:
    bit-exact at every step."""
    from noahmp_amd.engine import ColumnState
    g = load("branch_traj.npz")
    eng = engines("base", variant=variant)
    cols = cases.ColumnSet(g["static_f"], g["static_i"], g["state0"], g["isnow0"], *([None] * 7))
    cs = ColumnState.from_host(cols, DEV)
    F = torch.as_tensor(g["forcing"], device=DEV).contiguous()
    diag = torch.zeros((L.NDIAG_FULL, cs.ncol), device=DEV)
    for s in range(F.shape[0]):
        eng.step(cs, F[s], g["zsoil"], float(g["dt"]), traj_julian(g, s), int(g["yearlen"]), diag,
                 L.DIAG_FULL_LEVEL)
        torch.cuda.synchronize()
        assert_bit_exact(f"traj/{variant} step {s}", cs.state.cpu().numpy(),
                         cs.isnow.cpu().numpy(), diag.cpu().numpy(), cs.status.cpu().numpy(),
                         g["states"][s], g["isnows"][s], g["diags"][s], g["statuses"][s])


def test_branch_trajectory_run_out_bit_exact(engines):
    """The same 8 steps in one nmp_run_out launch with out_every = 1: every
    step's outputs in its ring slot and the final state, bit-exact."""
    from noahmp_amd.engine import ColumnState
    g = load("branch_traj.npz")
    eng = engines("base")
    cols = cases.ColumnSet(g["static_f"], g["static_i"], g["state0"], g["isnow0"], *([None] * 7))
    cs = ColumnState.from_host(cols, DEV)
    F = torch.as_tensor(g["forcing"], device=DEV).contiguous()
    nsteps = F.shape[0]
    ring = torch.full((nsteps, L.NDIAG_FULL, cs.ncol), float("nan"), device=DEV)
    eng.run(cs, F, g["zsoil"], float(g["dt"]), float(g["julian0"]), int(g["yearlen"]), nsteps,
            ring, L.DIAG_FULL_LEVEL, out_every=1)
    torch.cuda.synchronize()
    ring = ring.cpu().numpy()
    for s in range(nsteps):
        bad = ~bit_equal(ring[s], g["diags"][s])
        assert not bad.any(), (s, [L.DIAG_FULL[f] for f in np.nonzero(bad.any(1))[0]][:8],
                               list(np.nonzero(bad.any(0))[0][:8]))
    assert (g["statuses"] == 0).all()   # so the run's status word is 0 whatever it keeps
    assert_bit_exact("traj/run_out end", cs.state.cpu().numpy(), cs.isnow.cpu().numpy(),
                     ring[-1], cs.status.cpu().numpy(), g["states"][-1], g["isnows"][-1],
                     g["diags"][-1], g["statuses"][-1])


def test_branch_sflx_columns_bit_exact(engines):
    """nmp_sflx_columns (the reference's calling sequence on host records) on
    the branch columns."""
    g = load("branch_base.npz")
    r = L.sflx_records(g["state0"], g["isnow0"], g["static_f"], g["static_i"], g["forcing"],
                       g["zsoil"], g["dt"], g["julian"], g["yearlen"])
    engines("base").sflx_columns(r)
    st, isn, dg, status = L.soa_from_records(r)
    assert_bit_exact("base/sflx_columns", st, isn, dg, status, g["state1"], g["isnow1"], g["diag"],
                     g["status"])


def fp64_branch_records(get, port, name, pool):
    """A branch fixture through both fp64 occupancy kernels, every column held
    to the fixture's restatement ensemble (golden_io.check_fp64_rule)."""
    g = load(f"branch_{name}.npz")
    (est, eisn, edg, estat, _, _), discrete, q = fixture_ensemble(port, f"branch_{name}.npz")
    for variant in VARIANTS:
        st, isn, dg, status = run_single(get(name, precision=8, variant=variant), g, torch.float64)
        check_fp64_rule(f"branch_{name}/{variant}",
                        [(st, est, STATE_NAMES, FP64_STATE_ENV), (dg, edg, L.DIAG_FULL, FP64_DIAG_ENV)],
                        isn, status, eisn, estat, discrete, q, pool)


@pytest.mark.parametrize("name", SINGLES)
def test_branch_fp64_vs_fp64_oracle(engines, oracle_port, name):
    """fp64 engine vs the fp64 restatement on every column of the branch
    fixtures, both occupancy kernels, by the rule of tests/test_gpu_parity.py's
    module docstring: a column no member of the restatement's ensemble moves
    across a loop exit, ISNOW or status is held to 1e-9 max(1, 2 q) (1 + |x|).
    These columns sit on fp32 thresholds by design; that the fp32 and fp64
    marker masks differ on some is no excuse between two fp64 computations,
    so none is left out."""
    fp64_branch_records(engines, oracle_port, name, FP64_RECORDS)
