"""The step kernel at other soil layerings and time steps, against the reference Fortran.

zsoil[4] and dt are launch-wide run-time arguments, and every other fixture
uses case.nml's layering with dt 900 or 1800 s.  tests/golden/layers_*.npz
(tests/golden/make_layers_golden.py) hold groups of at most 80 columns, each
one launch with its own (zsoil, dt, yearlen, julian): thin, deep, uniform and
centimetre layerings at dt 60 to 10800 s, and three layerings with a thickness
outside [2^-20, 2^20] m, where the fp32 option-set kernels put every
soil-water division on IEEE (sflx_kernel.hip, soil_ok).  With the default
("ref") math the fp32 kernel must reproduce every column bit for bit -- in
both occupancy instantiations, in the compiled option sets and in the
run-time-options kernel, with and without diagnostics, through nmp_step,
nmp_step_binned, nmp_run_out and nmp_sflx_columns.  The fp64 kernels are held
to the fp64 restatement by golden_io.check_fp64_rule; the generator kept no
column the restatement's ensemble marks discrete, so none may be spent.
"""
import numpy as np
import pytest
import torch

from golden_io import (FP64_DIAG_ENV, FP64_STATE_ENV, bit_equal, check_fp64_rule, fixture_ensemble,
                       fixture_params, layer_group, load)
from noahmp_amd import cases, layout as L
from test_gpu_branches import DEV, STATE_NAMES, VARIANTS, assert_bit_exact, run_single
from test_layers_golden import NGROUPS, SINGLES, TRAJ_GROUPS, traj_julian

pytestmark = pytest.mark.gpu

GROUPS = list(range(1, NGROUPS + 1))
OPTION_SET = {"base": 1, "veg2": 2, "combo": 0}
FP64_RECORDS = []   # golden_io.check_fp64_rule's records of this session


@pytest.fixture(scope="module")
def engines(engine_lib):
    """Engines per (fixture, precision, launch variant, forced set 0)."""
    from noahmp_amd.engine import Engine
    from noahmp_amd.params import Params
    cache = {}

    def get(name, precision=4, variant="auto", set0=False):
        key = (name, precision, variant, set0)
        if key not in cache:
            g = load(f"layers_{name}.npz")
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


def group_of(name, group):
    g = layer_group(load(f"layers_{name}.npz"), group)
    assert g["isnow0"].size <= 80
    return g


def expected(g):
    return g["state1"], g["isnow1"], g["diag"], g["status"]


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("group", GROUPS)
@pytest.mark.parametrize("name", SINGLES)
def test_layers_single_bit_exact_vs_reference(engines, name, group, variant):
    """Every column of every group: state, the 58 outputs, ISNOW and status
    are the reference's bits, on both occupancy kernels of the option set the
    fixture selects (set 1, set 2, run-time options)."""
    g = group_of(name, group)
    eng = engines(name, variant=variant)
    assert eng.option_set() == OPTION_SET[name]
    assert_bit_exact(f"layers_{name}/{group}/{variant}", *run_single(eng, g), *expected(g))


@pytest.mark.parametrize("group", GROUPS)
@pytest.mark.parametrize("name", ["base", "veg2"])
def test_layers_run_time_options_kernel_bit_exact(engines, name, group):
    """The run-time-options kernel (set 0 forced) divides by the layer
    thicknesses on IEEE at every layering: the same bits."""
    g = group_of(name, group)
    assert_bit_exact(f"layers_{name}/{group}/set0", *run_single(engines(name, set0=True), g),
                     *expected(g))


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("group", GROUPS)
@pytest.mark.parametrize("name", ["base", "veg2"])
def test_layers_no_diagnostics_build_bit_exact(engines, name, group, variant):
    """DIAG_NONE runs the build compiled without diagnostics (separately for
    sets 1 and 2): state, ISNOW and status are the reference's bits."""
    g = group_of(name, group)
    eng = engines(name, variant=variant)
    assert eng.option_set() == OPTION_SET[name]
    st, isn, dg, status = run_single(eng, g, level=L.DIAG_NONE)
    assert dg is None   # nothing to compare: the stored outputs stand in for them below
    assert_bit_exact(f"layers_{name}/{group}/{variant}/nodiag", st, isn, g["diag"], status,
                     *expected(g))


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("group", TRAJ_GROUPS)
def test_layers_trajectory_steps_bit_exact(engines, group, variant):
    """16 nmp_step calls at dt 300 and 10800 s on the thin, cm and deep
    layerings: bit-exact at every step."""
    from noahmp_amd.engine import ColumnState
    g = layer_group(load("layers_traj.npz"), group)
    eng = engines("base", variant=variant)
    cols = cases.ColumnSet(g["static_f"], g["static_i"], g["state0"], g["isnow0"], *([None] * 7))
    cs = ColumnState.from_host(cols, DEV)
    F = torch.as_tensor(g["forcing"], device=DEV).contiguous()
    diag = torch.zeros((L.NDIAG_FULL, cs.ncol), device=DEV)
    assert F.shape[0] == 16
    for s in range(F.shape[0]):
        eng.step(cs, F[s], g["zsoil"], float(g["dt"]), traj_julian(g, s), int(g["yearlen"]), diag,
                 L.DIAG_FULL_LEVEL)
        torch.cuda.synchronize()
        assert_bit_exact(f"layers_traj/{group}/{variant} step {s}", cs.state.cpu().numpy(),
                         cs.isnow.cpu().numpy(), diag.cpu().numpy(), cs.status.cpu().numpy(),
                         g["states"][s], g["isnows"][s], g["diags"][s], g["statuses"][s])


@pytest.mark.parametrize("group", TRAJ_GROUPS)
def test_layers_trajectory_run_out_bit_exact(engines, group):
    """The same 16 steps in one nmp_run_out launch with out_every = 1: every
    step's outputs in its ring slot and the end state, bit-exact."""
    from noahmp_amd.engine import ColumnState
    g = layer_group(load("layers_traj.npz"), group)
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
    assert_bit_exact(f"layers_traj/{group}/run_out end", cs.state.cpu().numpy(),
                     cs.isnow.cpu().numpy(), ring[-1], cs.status.cpu().numpy(), g["states"][-1],
                     g["isnows"][-1], g["diags"][-1], g["statuses"][-1])


@pytest.mark.parametrize("group", [1, 6])
def test_layers_sflx_columns_bit_exact(engines, group):
    """nmp_sflx_columns (the reference's calling sequence on host records,
    which carry zsoil and dt) on the thin layering at dt 60 s and on the
    layering with a bottom layer thicker than 2^20 m."""
    g = group_of("base", group)
    r = L.sflx_records(g["state0"], g["isnow0"], g["static_f"], g["static_i"], g["forcing"],
                       g["zsoil"], g["dt"], g["julian"], g["yearlen"])
    engines("base").sflx_columns(r)
    assert_bit_exact(f"layers_base/{group}/sflx_columns", *L.soa_from_records(r), *expected(g))


def test_layers_binned_order_bit_exact(engines):
    """One nmp_step_binned launch in reversed column order on the thin
    layering at dt 10800 s (the group whose sub-steps double): the same bits."""
    from noahmp_amd.engine import ColumnState
    g = group_of("base", 2)
    eng = engines("base")
    cols = cases.ColumnSet(g["static_f"], g["static_i"], g["state0"], g["isnow0"], *([None] * 7))
    cs = ColumnState.from_host(cols, DEV)
    n = cs.ncol
    f = torch.as_tensor(g["forcing"], device=DEV).contiguous()
    diag = torch.zeros((L.NDIAG_FULL, n), device=DEV)
    order = torch.flip(torch.arange(n, dtype=torch.int32, device=DEV), (0,)).contiguous()
    cost = torch.full((n,), 255, dtype=torch.uint8, device=DEV)
    eng.step(cs, f, g["zsoil"], float(g["dt"]), float(g["julian"]), int(g["yearlen"]), diag,
             L.DIAG_FULL_LEVEL, order=order, cost=cost)
    torch.cuda.synchronize()
    assert_bit_exact("layers_base/2/binned", cs.state.cpu().numpy(), cs.isnow.cpu().numpy(),
                     diag.cpu().numpy(), cs.status.cpu().numpy(), *expected(g))


@pytest.mark.parametrize("group", GROUPS)
@pytest.mark.parametrize("name", SINGLES)
def test_layers_fp64_vs_fp64_oracle(engines, oracle_port, name, group):
    """Both fp64 occupancy kernels against the fp64 restatement on every
    column of every group, by golden_io.check_fp64_rule as
    tests/test_gpu_branches.py uses it.  A group has at most 80 columns, so
    the rule's cap on discrete columns leaves none to spend."""
    fname = f"layers_{name}.npz"
    g = group_of(name, group)
    (est, eisn, edg, estat, _, _), discrete, q = fixture_ensemble(oracle_port, fname, group)
    for variant in VARIANTS:
        st, isn, dg, status = run_single(engines(name, precision=8, variant=variant), g,
                                         torch.float64)
        check_fp64_rule(f"layers_{name}/{group}/{variant}",
                        [(st, est, STATE_NAMES, FP64_STATE_ENV), (dg, edg, L.DIAG_FULL, FP64_DIAG_ENV)],
                        isn, status, eisn, estat, discrete, q, FP64_RECORDS)
