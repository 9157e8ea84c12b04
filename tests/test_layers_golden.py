"""Pin the C restatement to the reference Fortran at other soil layerings and time steps.

tests/golden/layers_*.npz (tests/golden/make_layers_golden.py) hold groups of
columns, each group one launch with its own (zsoil, dt, yearlen, julian): thin,
deep, uniform and centimetre layerings at dt from 60 to 10800 s, and three
degenerate layerings whose thicknesses lie outside [2^-20, 2^20] m, where the
fp32 kernel's soil-water divisions leave their shared reciprocals for IEEE
division.  The bar is the one of test_oracle_golden.py: bit-exact.
tests/test_gpu_layers.py holds the kernels to the same files.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from golden_io import (GOLDEN, as_ref_status, bit_equal, fixture_step_args, layer_group,
                       layer_groups, load)
from noahmp_amd import layout as L

SINGLES = ["base", "veg2", "combo"]
NGROUPS = 8
TRAJ_GROUPS = [1, 2, 3]
DEGENERATE = (6, 7, 8)
CASE_NML_ZSOIL = (-0.1, -0.4, -1.0, -2.0)


def traj_julian(g, s):
    """Day of step s in fp32 arithmetic, as the engine's time loop advances it."""
    return float(g["julian0"] + np.float32(s) * g["dt"] / np.float32(86400.0))


def soil_window_ok(zsoil):
    """sflx_kernel.hip's launch-uniform soil_ok: every layer thickness and
    every two-layer span, formed in fp32 as the kernel forms them, lies in
    [2^-20, 2^20]."""
    z = np.asarray(zsoil, np.float32)
    assert z.dtype == np.float32 and z.shape == (4,)
    lo, hi = np.float32(2.0 ** -20), np.float32(2.0 ** 20)
    ok = True
    for k in range(4):
        den = -z[0] if k == 0 else z[k - 1] - z[k]
        ok &= bool(lo <= abs(den) <= hi)
        if k < 3:
            tmp = -z[1] if k == 0 else z[k - 1] - z[k + 1]
            ok &= bool(lo <= abs(tmp) <= hi)
    return ok


@pytest.mark.parametrize("group", range(1, NGROUPS + 1))
@pytest.mark.parametrize("name", SINGLES)
def test_layers_single_bit_exact(oracle_port, name, group):
    g = layer_group(load(f"layers_{name}.npz"), group)
    st, isn, dg, status = oracle_port.step(*fixture_step_args(g))
    assert np.array_equal(as_ref_status(status), g["status"])
    assert np.array_equal(isn, g["isnow1"])
    bad = ~bit_equal(st, g["state1"])
    assert not bad.any(), (list(np.nonzero(bad.any(1))[0]), list(np.nonzero(bad.any(0))[0][:8]))
    bad = ~bit_equal(dg, g["diag"])
    assert not bad.any(), ([L.DIAG_FULL[f] for f in np.nonzero(bad.any(1))[0]],
                           list(np.nonzero(bad.any(0))[0][:8]))


@pytest.mark.parametrize("group", TRAJ_GROUPS)
def test_layers_trajectory_bit_exact(oracle_port, group):
    g = layer_group(load("layers_traj.npz"), group)
    args = fixture_step_args(dict(g, julian=g["julian0"]))
    P, opts, zs, dt, ylen = args[:5]
    st, isn = g["state0"], g["isnow0"]
    assert g["forcing"].shape[0] == 16 and int(g["keep_every"]) == 1
    for s in range(16):
        st, isn, dg, status = oracle_port.step(P, opts, zs, dt, ylen, traj_julian(g, s), st, isn,
                                               g["static_f"], g["static_i"], g["forcing"][s])
        assert bit_equal(st, g["states"][s]).all(), f"state diverged at step {s}"
        assert np.array_equal(isn, g["isnows"][s]), s
        assert bit_equal(dg, g["diags"][s]).all(), f"diag diverged at step {s}"
        assert np.array_equal(as_ref_status(status), g["statuses"][s]), s


@pytest.mark.parametrize("name", SINGLES)
def test_layers_single_structure(name):
    g = load(f"layers_{name}.npz")
    assert layer_groups(g) == list(range(1, NGROUPS + 1))
    assert g["zsoil"].shape == (NGROUPS, 4) and g["zsoil"].dtype == np.float32
    for key in ("dt", "yearlen", "julian"):
        assert g[key].shape == (NGROUPS,), key
    n = g["group"].size
    assert g["state0"].shape == (L.NSTATE, n) and g["diag"].shape == (L.NDIAG_FULL, n)
    counts = [int((g["group"] == k).sum()) for k in layer_groups(g)]
    assert sum(counts) == n and all(64 <= c <= 80 for c in counts), counts
    assert (np.diff(g["group"]) >= 0).all()       # the groups are contiguous runs
    assert len({tuple(z) for z in g["zsoil"].tolist()}) >= 4
    assert len(set(g["dt"].tolist())) >= 4
    assert set(g["yearlen"].tolist()) == {365, 366}
    assert (g["zsoil"] < 0).all() and (np.diff(g["zsoil"], axis=1) < 0).all()
    # groups 6 to 8 lie outside the kernel's window, every other group inside it and
    # off case.nml's layering and time step
    for k in layer_groups(g):
        inside = soil_window_ok(g["zsoil"][k - 1])
        assert inside == (k not in DEGENERATE), (k, g["zsoil"][k - 1])
        if inside:
            assert tuple(g["zsoil"][k - 1]) != tuple(np.float32(CASE_NML_ZSOIL))
            assert float(g["dt"][k - 1]) != 1800.0
    assert np.isfinite(g["state1"]).all() and np.isfinite(g["diag"]).all()
    assert (g["status"] == 0).all()
    assert os.path.getsize(os.path.join(GOLDEN, f"layers_{name}.npz")) < 400 * 1024
    # every ZSNSO soil interface is the group's layering under the column's layered snow
    for k in layer_groups(g):
        q = layer_group(g, k)
        z = q["state0"][L.s("ZSNSO")]
        h = np.where(q["isnow0"] < 0, q["state0"][L.si("SNOWH")], 0.0)
        assert np.allclose(z[3:], q["zsoil"][:, None].astype(np.float64) - h[None, :], rtol=1e-6,
                           atol=1e-7), k


def test_layers_fixtures_select_the_three_kernel_sets():
    opts = {name: tuple(load(f"layers_{name}.npz")["options"]) for name in SINGLES}
    assert opts["base"] == L.options_tuple(L.CASE_NML_OPTIONS)
    assert opts["veg2"] == L.options_tuple(dict(L.CASE_NML_OPTIONS, opt_veg=2))
    assert opts["combo"] == L.options_tuple(dict(
        L.CASE_NML_OPTIONS, opt_veg=4, opt_run=4, opt_rad=2, opt_sfc=2, opt_stc=2, opt_frz=2))
    assert tuple(load("layers_traj.npz")["options"]) == opts["base"]


def test_layers_reach_the_substep_doubling_and_snow(oracle_port):
    """The edits the generator makes are still there: group 2 (thin layers,
    dt 10800) doubles the soil-water sub-steps on some columns, and the thin
    and cm groups carry layered snow."""
    it = oracle_port.STAT_LOOPS.index("soilwater sub-steps")
    for name in SINGLES:
        g = load(f"layers_{name}.npz")
        *_, trips = oracle_port.step_stats(*fixture_step_args(layer_group(g, 2)))
        assert (trips[:, it] == 6).sum() >= 4 and (trips[:, it] == 3).sum() >= 4, name
        for k in (1, 2, 5):
            assert (layer_group(g, k)["isnow0"] < 0).sum() >= 8, (name, k)


def test_layers_trajectory_structure():
    g = load("layers_traj.npz")
    assert layer_groups(g) == TRAJ_GROUPS
    assert [int((g["group"] == k).sum()) for k in TRAJ_GROUPS] == [32, 32, 32]
    assert g["dt"].tolist() == [10800.0, 300.0, 10800.0]
    assert (g["yearlen"] == 365).all() and (g["julian0"] == 360.0).all()
    assert np.isfinite(g["states"]).all() and np.isfinite(g["diags"]).all()
    assert (g["statuses"] == 0).all()
    for k in TRAJ_GROUPS:
        q = layer_group(g, k)
        assert soil_window_ok(q["zsoil"])
        assert traj_julian(q, 15) + float(q["dt"]) / 86400.0 <= 365.0   # inside the year
        snow = (q["isnow0"] < 0) | (q["state0"][L.si("SNEQV")] > 0)
        assert 8 <= snow.sum() <= 24, (k, int(snow.sum()))               # snow and snow-free


def _need_ref():
    import ref
    if not ref.available():
        pytest.skip("reference oracle not built (oracle/_ref)")
    return ref


@pytest.mark.parametrize("name", SINGLES + ["traj"])
def test_layers_fixture_regenerates_from_the_reference(name):
    """Where the reference is built: the stored outputs are what the reference
    computes from the stored inputs, group by group (and step by step).  The
    reference keeps its options in process-global variables, so this runs the
    generator's --check entry in a process of its own."""
    _need_ref()
    gen = os.path.join(GOLDEN, "make_layers_golden.py")
    r = subprocess.run([sys.executable, gen, "--check", name], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "reproduced by the reference" in r.stdout
