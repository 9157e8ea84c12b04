"""Pin the rare physics branches of the C restatement to the reference Fortran.

tests/golden/branch_*.npz (tests/golden/make_branch_golden.py) hold columns
edited so that the reference itself takes the branches no plausible-climate
fixture reaches: snow caps, the sign cases of the snow-layer bookkeeping, the
C4 pathway, a water table inside the soil column.  The bar is the one of
test_oracle_golden.py: bit-exact.  The branch-marker build of the restatement
(port.step_branches) proves that each fixture really executes the branches it
declares, so a fixture cannot silently stop covering them.
"""
import numpy as np
import pytest

from golden_io import TIE_FRAC, as_ref_status, bit_equal, fixture_params, load, load_params
from noahmp_amd import layout as L

SINGLES = ["base", "veg2", "combo"]
MIN_HITS = 4

# Sites of port.BRANCH_SITES that no fixture pins, each with the reason
# (line numbers: the reference's core/module_noahmp_func.f90).
NOT_PINNED = {
    "vege_flux_cah2_small":
        "dead: CAH2 = FV*KARMAN/(log((2+Z0H)/Z0H) - FH2) (:2948).  sfcdif1 keeps FH2 <= 0.9 of "
        "that log and >= -5 (MOZ <= 1, :3432), and FV = UR*KARMAN/(log((ZLVL-ZPD)/Z0M) - FM) with "
        "UR >= 1 (:1041) and FM >= -5; sfcdif2 keeps USTAR >= 0.07 (:3605, :3664).  No finite fp32 "
        "log makes the quotient < 1e-5.",
    "bare_flux_ehb2_small": "dead: the same bound for EHB2 (:3245).",
    "frh2o_flerchinger":
        "left out: the Newton loop (:4560) converged for all 2.4e6 random (soil type, T down to "
        "200 K and to within 1e-3 K of TFRZ, SMC, SH2O) inputs tried with the shipped soil tables, "
        "as an earlier search of 4e5 did (test_gpu_routines.py); the fallback (:4588) was never "
        "taken.",
    "phasechange_imelt_reset":
        "dead: IMELT = 1 only with STC >= TFRZ (:4391, :4400), so HM = (STC-TFRZ)/FACT >= 0 "
        "(:4408); IMELT = 2 only with STC < TFRZ (:4394), so HM < 0.  Neither reset (:4412, :4416) "
        "can fire.",
    "phasechange_below_supercool":
        "dead for SH2O <= SMC: XM < 0 needs IMELT = 2, which needs MLIQ > SUPERCOOL (:4394), and "
        "WMASS0 = MICE + MLIQ >= MLIQ (:4454).",
    "combine_negative_soilice":
        "dead: soilice = max(0, SMC - SH2O) on entry to the water routines (:414); snowh2o resets "
        "a negative value at once (:5728, :5750) before it calls combine, and combine's own update "
        "is clamped at 0 (:5293).  soilice(1) < 0 at :5322 cannot happen.",
    "co2flux_rtmass_negative":
        "dead for RTMASS >= 0: NPPR >= -RSROOT (:6910) and RTTOVR = 2e-8*RTMASS, so one step "
        "removes a fraction ~1e-5 of RTMASS; :6989 needs a negative root mass on input.",
    "sflx_unknown_opt_veg": "dead through the engine: nmp_init rejects an opt_veg outside 1..5 (:377).",
}


def step_args(g, precision=4):
    return (fixture_params(g), tuple(g["options"]), g["zsoil"], float(g["dt"]), int(g["yearlen"]),
            float(g["julian"]), g["state0"], g["isnow0"], g["static_f"], g["static_i"],
            g["forcing"])


def traj_julian(g, s):
    """Day of step s in fp32 arithmetic, as the engine's time loop advances it."""
    return float(g["julian0"] + np.float32(s) * g["dt"] / np.float32(86400.0))


def site_bits(port, mask, site):
    return ((mask >> np.uint32(port.BRANCH_SITES.index(site))) & 1).astype(bool)


@pytest.mark.parametrize("name", SINGLES)
def test_branch_single_bit_exact(oracle_port, name):
    g = load(f"branch_{name}.npz")
    st, isn, dg, status = oracle_port.step(*step_args(g))
    assert np.isfinite(g["state1"]).all() and np.isfinite(g["diag"]).all()
    assert (g["status"] == 0).all()
    assert np.array_equal(as_ref_status(status), g["status"])
    assert np.array_equal(isn, g["isnow1"])
    bad = ~bit_equal(st, g["state1"])
    assert not bad.any(), (list(np.nonzero(bad.any(1))[0]), list(np.nonzero(bad.any(0))[0][:8]))
    bad = ~bit_equal(dg, g["diag"])
    assert not bad.any(), ([L.DIAG_FULL[f] for f in np.nonzero(bad.any(1))[0]],
                           list(np.nonzero(bad.any(0))[0][:8]))


def test_branch_trajectory_bit_exact(oracle_port):
    g = load("branch_traj.npz")
    P = load_params()
    opts, dt, ylen = tuple(g["options"]), float(g["dt"]), int(g["yearlen"])
    st, isn = g["state0"], g["isnow0"]
    assert g["isnow0"].size <= 64 and g["forcing"].shape[0] == 8 and int(g["keep_every"]) == 1
    for s in range(8):
        jul = traj_julian(g, s)
        st, isn, dg, status = oracle_port.step(P, opts, g["zsoil"], dt, ylen, jul, st, isn,
                                               g["static_f"], g["static_i"], g["forcing"][s])
        assert bit_equal(st, g["states"][s]).all(), f"state diverged at step {s}"
        assert np.array_equal(isn, g["isnows"][s]), s
        assert bit_equal(dg, g["diags"][s]).all(), f"diag diverged at step {s}"
        assert np.array_equal(as_ref_status(status), g["statuses"][s]), s
    # the packs keep changing their layering after the first step's combines
    assert (g["isnows"][0] != g["isnow0"]).sum() >= 8
    assert (g["isnows"][1:] != g["isnows"][:-1]).any()


@pytest.mark.parametrize("name", SINGLES)
def test_branch_sites_are_executed(oracle_port, name):
    """Every site the fixture declares is executed by at least MIN_HITS of its
    columns (one column can sit on a tie), by the stats build that is
    bit-identical to the oracle; and the fp32 and fp64 builds disagree on the
    site mask (a threshold tie) in at most TIE_FRAC of the columns."""
    g = load(f"branch_{name}.npz")
    n = g["isnow0"].size
    assert n <= 512
    *o32, m32 = oracle_port.step_branches(*step_args(g), precision=4)
    assert bit_equal(o32[0], g["state1"]).all() and bit_equal(o32[2], g["diag"]).all()
    assert np.array_equal(m32, g["mask32"])
    *o64, m64 = oracle_port.step_branches(*step_args(g), precision=8)
    assert np.array_equal(m64, g["mask64"])
    sites = [str(s) for s in g["sites"]]
    assert sites and set(sites) <= set(oracle_port.BRANCH_SITES)
    hits = {s: int(site_bits(oracle_port, m32, s).sum()) for s in sites}
    print(name, n, "columns;", hits, "fp32/fp64 mask ties:", int((m32 != m64).sum()))
    assert all(h >= MIN_HITS for h in hits.values()), hits
    assert (m32 != m64).sum() <= TIE_FRAC * n
    if "combine_middle_layer" in sites:  # both neighbour choices, not only the upper one
        lower = site_bits(oracle_port, m32, "combine_middle_layer") & \
            ~site_bits(oracle_port, m32, "combine_middle_layer_upper_neighbour")
        assert lower.sum() >= MIN_HITS, int(lower.sum())


def test_branch_sites_union_covers_the_table(oracle_port):
    """Every marked site is pinned by some fixture, or listed in NOT_PINNED
    with its reason -- and never both."""
    declared = set()
    for name in SINGLES:
        declared |= {str(s) for s in load(f"branch_{name}.npz")["sites"]}
    assert not declared & set(NOT_PINNED), declared & set(NOT_PINNED)
    assert declared | set(NOT_PINNED) == set(oracle_port.BRANCH_SITES), \
        set(oracle_port.BRANCH_SITES) ^ (declared | set(NOT_PINNED))
    assert all(isinstance(r, str) and len(r) > 20 for r in NOT_PINNED.values())
    # the three fixtures select the three kernel specialisations
    opts = {name: tuple(load(f"branch_{name}.npz")["options"]) for name in SINGLES}
    base = L.options_tuple(L.CASE_NML_OPTIONS)
    assert opts["base"] == base
    assert opts["veg2"] == L.options_tuple(dict(L.CASE_NML_OPTIONS, opt_veg=2))
    assert sum(a != b for a, b in zip(opts["combo"], base)) == 4


def test_branch_fixture_has_a_c4_table():
    g = load("branch_veg2.npz")
    P = fixture_params(g)
    stock = load_params()
    assert (np.asarray(P["c3c4"]) == 2).sum() >= 3 and (np.asarray(stock["c3c4"]) != 2).all()
    for k in stock:   # nothing else differs from the shipped table
        if k != "c3c4":
            assert bit_equal(np.asarray(P[k]), np.asarray(stock[k])).all(), k
    c4 = np.isin(g["static_i"][L.STATIC_I.index("VEGTYP")], np.nonzero(P["c3c4"] == 2)[0] + 1)
    assert (c4 & (g["diag"][L.DIAG_FULL.index("PSN")] > 0)).sum() >= MIN_HITS


@pytest.mark.parametrize("name", ["base", "combo"])
def test_branch_fixture_regenerates_from_the_reference(name):
    """Where the reference is built: the stored outputs are what the reference
    computes from the stored inputs."""
    import ref
    if not ref.available():
        pytest.skip("reference oracle not built (oracle/_ref)")
    g = load(f"branch_{name}.npz")
    ref.configure(tuple(g["options"]))
    st, isn, dg, status = ref.step(g["zsoil"], float(g["dt"]), int(g["yearlen"]),
                                   float(g["julian"]), g["state0"], g["isnow0"], g["static_f"],
                                   g["static_i"], g["forcing"])
    assert bit_equal(st, g["state1"]).all() and bit_equal(dg, g["diag"]).all()
    assert np.array_equal(isn, g["isnow1"]) and np.array_equal(status, g["status"])


def test_branch_c4_fixture_regenerates_from_the_reference():
    """branch_veg2.npz, the only fixture that pins the C4 pathway and the
    b >= 0 root: the reference, reading the edited table, reproduces the stored
    table values and outputs from the stored inputs.  The reference keeps its
    tables in process-global arrays, so this runs the generator's --check
    entry in a process of its own."""
    import os
    import subprocess
    import sys

    import ref
    if not ref.available():
        pytest.skip("reference oracle not built (oracle/_ref)")
    gen = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                       "make_branch_golden.py")
    r = subprocess.run([sys.executable, gen, "--check", "veg2"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "reproduced by the reference" in r.stdout


def test_branch_trajectory_regenerates_from_the_reference():
    """Where the reference is built: its 8 steps from the stored start and
    forcing give every stored step."""
    import ref
    if not ref.available():
        pytest.skip("reference oracle not built (oracle/_ref)")
    g = load("branch_traj.npz")
    ref.configure(tuple(g["options"]))
    st, isn = g["state0"], g["isnow0"]
    for s in range(g["forcing"].shape[0]):
        st, isn, dg, status = ref.step(g["zsoil"], float(g["dt"]), int(g["yearlen"]),
                                       traj_julian(g, s), st, isn, g["static_f"], g["static_i"],
                                       g["forcing"][s])
        assert bit_equal(st, g["states"][s]).all() and bit_equal(dg, g["diags"][s]).all(), s
        assert np.array_equal(isn, g["isnows"][s]) and np.array_equal(status, g["statuses"][s]), s
