"""The no-diagnostics instantiations of the fp32 step kernel.

A launch at NMP_DIAG_NONE of a compiled option set (1: case.nml options, 2: the
same with opt_veg = 2), at full occupancy, runs a kernel compiled without the
diagnostics (sflx_kernel.hip kNoDiag): no 2-m chain, no TRAD, no
diagnostic-only value.  It must leave the reference's state bit for bit, and
nothing an output step after it needs may be missing.  Every other launch --
an output level, the half-occupancy ("small") kernel, the run-time-options
kernel -- runs the kernels it ran before.

The fixture sizes select the half-occupancy kernel by themselves, so every
test here pins the launch variant.
"""
import dataclasses

import numpy as np
import pytest
import torch

from golden_io import as_ref_status, bit_equal, fixture_tags, load, single_names
from noahmp_amd import cases, layout as L

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CASE = [L.CASE_NML_OPTIONS[k] for k in L.OPTION_NAMES]
VEG2 = [2 if k == "opt_veg" else L.CASE_NML_OPTIONS[k] for k in L.OPTION_NAMES]
LEVELS = {"none": (L.DIAG_NONE, 0), "out": (L.DIAG_OUT_LEVEL, L.NDIAG_OUT),
          "full": (L.DIAG_FULL_LEVEL, L.NDIAG_FULL)}


def compiled_set(options):
    """The compiled option set of `options` (sflx_kernel.hip kOptionSet), or 0."""
    o = [int(x) for x in options]
    return 1 if o == CASE else 2 if o == VEG2 else 0


@pytest.fixture(scope="module")
def engines(engine_lib):
    """Engines by (options, table tags, launch variant, forced set 0), closed at
    the end of the module."""
    from noahmp_amd.engine import Engine
    from noahmp_amd.params import Params
    cache, tables = {}, {}

    def get(options, tags=("STAS", "USGS"), variant="full", generic=False):
        key = (tuple(int(x) for x in options), tuple(tags), variant, generic)
        if key not in cache:
            if tags not in tables:
                tables[tags] = Params.builtin(*tags)
            e = Engine(tables[tags], dict(zip(L.OPTION_NAMES, key[0])), device=0, precision=4)
            assert e.launch_variant(variant) == variant
            if generic:
                assert e.option_set(0) == 0
            else:
                assert e.option_set() == compiled_set(options)
            cache[key] = e
        return cache[key]
    yield get
    for e in cache.values():
        e.close()


def out_from_full(full):
    """The 16 NMP_DIAG_OUT rows from the 58 NMP_DIAG_FULL rows of a fixture:
    15 are FULL rows; T2M is the tile blend FVEG*T2MV + (1-FVEG)*T2MB of the
    kernel's aggregation (func.f90:1246-1282), T2MB alone without canopy, in
    fp32 without contraction as the kernel forms it."""
    full = np.asarray(full, np.float32)
    fveg, t2mv, t2mb = (full[L.DIAG_FULL.index(n)] for n in ("FVEG", "T2MV", "T2MB"))
    with np.errstate(invalid="ignore"):
        blend = fveg * t2mv + (np.float32(1.0) - fveg) * t2mb
    rows = [np.where(fveg > 0, blend, t2mb) if n == "T2M" else full[L.DIAG_FULL.index(n)]
            for n in L.DIAG_OUT]
    return np.stack(rows).astype(np.float32)


def column_state(g):
    from noahmp_amd.engine import ColumnState
    cols = cases.ColumnSet(g["static_f"], g["static_i"], g["state0"], g["isnow0"], *([None] * 7))
    return ColumnState.from_host(cols, DEV)


def step_at(eng, cs, f, zsoil, dt, jul, yl, level):
    lvl, nd = LEVELS[level]
    d = torch.zeros((nd, cs.ncol), device=DEV) if nd else None
    eng.step(cs, f, zsoil, dt, jul, yl, d, lvl)
    return d


# ---- single call against the reference fixtures -----------------------------
# variant "full" at "none": the new kernels for the fixtures of set 1 and set 2
# (the case.nml ones, the table variants, "fatal"; "veg2"), HEAD's run-time-
# options kernel for the rest; "out"/"full" and "small" are HEAD's kernels
@pytest.mark.parametrize("variant,level", [("full", "none"), ("full", "out"), ("full", "full"),
                                           ("small", "none")])
@pytest.mark.parametrize("name", single_names())
def test_single_call_vs_reference(engines, name, variant, level):
    g = load(f"single_{name}.npz")
    eng = engines(g["options"], tags=fixture_tags(g), variant=variant)
    cs = column_state(g)
    d = step_at(eng, cs, torch.as_tensor(g["forcing"], device=DEV).contiguous(), g["zsoil"],
                float(g["dt"]), float(g["julian"]), int(g["yearlen"]), level)
    torch.cuda.synchronize()
    st, isn, status = cs.state.cpu().numpy(), cs.isnow.cpu().numpy(), cs.status.cpu().numpy()
    assert st.shape[0] == 56
    ok = bit_equal(st, g["state1"]).all(0) & (isn == g["isnow1"]) & \
        (as_ref_status(status) == g["status"])
    if level != "none":
        exp = g["diag"] if level == "full" else out_from_full(g["diag"])
        ok &= bit_equal(d.cpu().numpy(), exp).all(0)
    assert ok.all(), f"{name} {variant} {level}: {(~ok).sum()} of {ok.size} columns differ"


def test_fixtures_reach_both_new_kernels():
    """The single-call fixtures above hold both compiled option sets."""
    sets = {compiled_set(load(f"single_{n}.npz")["options"]) for n in single_names()}
    assert {1, 2} <= sets


# ---- trajectory: NONE, NONE, OUT repeated ------------------------------------
@pytest.mark.parametrize("name", ["snow", "casenml"])
def test_trajectory_none_none_out(engines, name):
    """The reference trajectories stepped NONE, NONE, OUT, ...: the state after
    every step the fixture keeps is the reference's, and so are the 16
    diagnostics of every OUT step the fixture keeps -- a step that skipped the
    2-m chain leaves nothing the next output step needs."""
    g = load(f"traj_{name}.npz")
    assert compiled_set(g["options"]) == 1
    eng = engines(g["options"], variant="full")
    cs = column_state(g)
    F = torch.as_tensor(g["forcing"], device=DEV).contiguous()
    dt, ke, yl, nstep = float(g["dt"]), int(g["keep_every"]), int(g["yearlen"]), F.shape[0]
    d = torch.zeros((L.NDIAG_OUT, cs.ncol), device=DEV)
    states, diags = {}, {}
    for s in range(nstep):
        out = s % 3 == 2
        jul = float(g["julian0"]) + s * dt / 86400.0
        eng.step(cs, F[s], g["zsoil"], dt, jul, yl, d if out else None,
                 L.DIAG_OUT_LEVEL if out else L.DIAG_NONE)
        if (s + 1) % ke == 0:  # the fixture's record k = (s + 1) / ke - 1
            k = (s + 1) // ke - 1
            states[k] = (cs.state.clone(), cs.isnow.clone())
            if out:
                diags[k] = d.clone()
    torch.cuda.synchronize()
    assert len(states) == nstep // ke and len(diags) >= 20
    for k, (st, isn) in states.items():
        ok = bit_equal(st.cpu().numpy(), g["states"][k]).all(0) & \
            (isn.cpu().numpy() == g["isnows"][k])
        assert ok.all(), f"{name} record {k}: {(~ok).sum()} columns' state differ"
    for k, dd in diags.items():
        ok = bit_equal(dd.cpu().numpy(), out_from_full(g["diags"][k]))
        assert ok.all(), f"{name} record {k}: diagnostics {np.nonzero(~ok.all(1))[0]} differ"


# ---- kernel to kernel ----------------------------------------------------------
N_K2K = 333  # two workgroups, the second one full wave and one of 13 lanes


@pytest.fixture(scope="module")
def k2k_reference(engines):
    """8 steps (NONE, OUT alternating) of 333 mixed columns through the
    run-time-options kernel (set 0, unchanged code), per opt_veg: computed
    once, shared, not modified.  Snow and no snow, canopy and bare ground, day
    and night (the longitudes)."""
    from noahmp_amd.engine import ColumnState
    from noahmp_amd.params import Params
    done = {}

    def get(opt_veg):
        if opt_veg not in done:
            opts = CASE if opt_veg == 1 else VEG2
            tab = Params.builtin().as_dict()
            cols = cases.make_columns(N_K2K, "mixed", tab, seed=21, julian=95.0)
            # "mixed" draws vegetated types only: every 7th column bare ground
            vt = cols.static_i[L.STATIC_I.index("VEGTYP")]
            vt[::7] = tab["isbarren"]
            F = [torch.as_tensor(cases.forcing_step(cols, 95.0 + s / 48.0, 365, s, seed=21),
                                 device=DEV) for s in range(8)]
            eng = engines(opts, variant="full", generic=True)
            cs = ColumnState.from_host(cols, DEV)
            diags = []
            for s in range(8):
                d = step_at(eng, cs, F[s], cases.CASE_NML_ZSOIL, 1800.0, 95.0 + s / 48.0, 365,
                            "out" if s % 2 else "none")
                if d is not None:
                    diags.append(d)
            torch.cuda.synchronize()
            # the set holds snow and no snow, canopy and bare ground, day and night
            assert (cols.isnow < 0).any() and (cols.isnow == 0).any()
            assert (vt == tab["isbarren"]).any() and (vt != tab["isbarren"]).any()
            cosz = np.stack([f[L.FORCING.index("COSZ")].cpu().numpy() for f in F])
            assert (cosz > 0).any() and (cosz <= 0).any()
            done[opt_veg] = (cols, F, cs, diags)
        return done[opt_veg]
    return get


@pytest.mark.parametrize("shards", [1, 2])
@pytest.mark.parametrize("cpw", [64, 8])
@pytest.mark.parametrize("opt_veg", [1, 2])
def test_new_kernels_equal_runtime_options_kernel(engines, k2k_reference, opt_veg, cpw, shards):
    from noahmp_amd.engine import ColumnState, StreamShards
    cols, F, ref_cs, ref_diags = k2k_reference(opt_veg)
    eng = engines(CASE if opt_veg == 1 else VEG2, variant="full")
    assert eng.option_set() == opt_veg
    eng.set_cols_per_wave(cpw)
    try:
        cs = ColumnState.from_host(cols, DEV)
        sh = StreamShards(eng, cs, shards)
        diags = []
        for s in range(8):
            lvl, nd = LEVELS["out" if s % 2 else "none"]
            d = torch.zeros((nd, N_K2K), device=DEV) if nd else None
            sh.step(F[s], cases.CASE_NML_ZSOIL, 1800.0, 95.0 + s / 48.0, 365, d, lvl)
            if d is not None:
                diags.append(d)
        sh.join()
        torch.cuda.synchronize()
    finally:
        eng.set_cols_per_wave(0)
    bits = lambda t: t.view(torch.int32)
    assert torch.equal(bits(cs.state), bits(ref_cs.state))
    assert torch.equal(cs.isnow, ref_cs.isnow) and torch.equal(cs.status, ref_cs.status)
    assert len(diags) == 4
    for k, (x, y) in enumerate(zip(diags, ref_diags)):
        assert torch.equal(bits(x), bits(y)), f"OUT step {2 * k + 1}"


# ---- domain fallback: the DivRef copy of the loops in the new kernels ---------
@pytest.mark.parametrize("opt_veg", [1, 2])
def test_domain_fallback_at_level_none(engines, opt_veg):
    """The columns test_gpu_parity's domain-fallback test pushes outside the
    range proof's domain (wind of 150-400 m/s, surface pressure of 2.5e4 Pa, a
    canopy wet fraction of 1e-20, CO2 of 0.5 Pa, EAH of 1e-5 Pa, on every third
    column) re-run their Newton loops with IEEE division: stepped at
    NMP_DIAG_NONE the new kernel's state equals the run-time-options kernel's."""
    from noahmp_amd.engine import ColumnState
    from noahmp_amd.params import Params
    n = 4096
    cols = cases.make_columns(n, "mixed", Params.builtin().as_dict(), seed=31, julian=180.0)
    f = cases.forcing_step(cols, 180.3, 366, 0, seed=31).copy()
    st = cols.state.copy()
    rng = np.random.default_rng(7)
    which = np.where(np.arange(n) % 3 == 0, rng.choice([0, 1, 2, 3, 4], n), -1)
    fi = L.FORCING.index
    f[fi("UU"), which == 0] = rng.uniform(150.0, 400.0, (which == 0).sum()).astype(np.float32)
    f[fi("SFCPRS"), which == 1] = np.float32(2.5e4)
    f[fi("PSFC"), which == 1] = np.float32(2.5e4)
    st[L.s("FWET").start, which == 2] = np.float32(1e-20)
    f[fi("CO2AIR"), which == 3] = np.float32(0.5)
    st[L.s("EAH").start, which == 4] = np.float32(1e-5)
    cols = dataclasses.replace(cols, state=st)
    opts = CASE if opt_veg == 1 else VEG2
    res = []
    for generic in (False, True):
        eng = engines(opts, variant="full", generic=generic)
        cs = ColumnState.from_host(cols, DEV)
        eng.step(cs, torch.as_tensor(f, device=DEV), cases.CASE_NML_ZSOIL, 1800.0, 180.3, 366)
        torch.cuda.synchronize()
        res.append(cs)
    bits = lambda t: t.view(torch.int32)
    bad = (bits(res[0].state) != bits(res[1].state)).any(0)
    assert not bool(bad.any()), f"{int(bad.sum())} columns' state differ"
    assert torch.equal(res[0].isnow, res[1].isnow) and torch.equal(res[0].status, res[1].status)
