"""Generate tests/golden/layers_*.npz from the REFERENCE Fortran: the step at
other soil layerings and time steps than run/case.nml's.

zsoil[4] and dt are launch-wide run-time arguments of the engine, and every
other fixture uses one layering, (-0.1, -0.4, -1.0, -2.0), with dt 900 or
1800 s.  The fixtures written here hold several *groups*; each group is one
launch with its own (zsoil, dt, yearlen, julian).  Inputs AND outputs are the
reference's; the fp32 restatement (oracle/noahmp_oracle.c) must reproduce
them bit for bit before a file is written.

Fixture format (tests/golden_io.py layer_group(g, k) returns group k = 1..G as
a single-call fixture): zsoil (G, 4), dt (G,), yearlen (G,), julian (G,) [the
trajectory: julian0 (G,)], group (ncol,) = each column's group number 1..G,
options, and the per-column arrays of a single-call fixture (state0, isnow0,
static_f, static_i, forcing, state1, isnow1, diag, status) or of
branch_traj.npz (forcing, states, isnows, diags, statuses with a leading step
axis).  The tables are the shipped STAS / USGS ones.

  layers_base.npz    case.nml options (compiled kernel set 1)
  layers_veg2.npz    opt_veg=2 (set 2)
  layers_combo.npz   opt_veg=4 opt_run=4 opt_rad=2 opt_sfc=2 opt_stc=2 opt_frz=2
                     (run-time-options set 0); opt_run=4's DZTOT loop ends
                     differently on a column shallower or deeper than 2 m
  layers_traj.npz    16 steps, every step saved, case.nml options

Groups of each single-step file (KEEP columns each: one full wave and a ragged
one), from a pool of "mixed" columns made for the group's layering:

  group  layering                        dt     yearlen, julian
  1      thin    (-0.05,-0.2,-0.5,-1.5)  60     365, 364.9
  2      thin                            10800  366, 0.0
  3      deep    (-0.1,-0.5,-1.5,-3.0)   600    365, 200.3
  4      uniform (-0.25,-0.5,-0.75,-1)   3600   365, 20.3
  5      cm      (-0.02,-0.08,-0.3,-1)   60     366, 366.0
  6      (-0.1,-0.4,-1.0,-2.2e6)         1800   366, 180.3   bottom layer > 2^20 m
  7      (-0.1,-0.4,-1.0,-1.0-2^-21)     1800   365, 180.3   bottom layer < 2^-20 m
  8      (-2^-21,-0.4,-1.0,-2.0)         1800   366, 180.3   top layer < 2^-20 m

Groups 6 to 8 lie outside the window in which the fp32 kernel divides by the
layer thicknesses through shared reciprocals (sflx_kernel.hip, soil_ok), so
their launches run every such division on IEEE.  In the thin and cm groups a
quarter of the pool gets heavy rain (10 to 40 mm/h, which reaches the
soil-water sub-step doubling at the long step) and a quarter a replaced snow
pack (compaction and ageing at the unusual dt).

Groups of layers_traj.npz (32 columns each, snow and snow-free, 365-day year,
from day 360.0; the day of step s is formed in fp32 as the engine's time loop
forms it):

  group  layering  dt     steps
  1      thin      10800  16
  2      cm        300    16
  3      deep      10800  16

Columns kept: the reference leaves every value finite with status 0 (the
trajectory: at every step); and, in the single-step files, port.step_ensemble
does not mark the column discrete and the fp32 and fp64 restatements agree on
ISNOW, so the fp64 tests have no ties to excuse.  A group that ends with
fewer than MIN_KEEP columns is an error.

usage (needs the reference sources; see make_golden.py):
  make -C oracle ref port && python tests/golden/make_layers_golden.py [base veg2 combo traj]
  python tests/golden/make_layers_golden.py --check veg2   # stored outputs == the reference's
"""
from __future__ import annotations

import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import noahmp_pkg  # noqa: E402,F401
import port  # noqa: E402
import ref  # noqa: E402
from golden_io import as_ref_status, layer_group, layer_groups, perturb_bounds  # noqa: E402
from noahmp_amd import cases  # noqa: E402
from noahmp_amd import layout as L  # noqa: E402

TFRZ = 273.15
POOL = 224         # columns drawn per group
KEEP = 80          # columns kept per group: one full wave and a ragged one
MIN_KEEP = 64
F = L.FORCING.index

LAYERINGS = {
    "casenml": (-0.1, -0.4, -1.0, -2.0),
    "thin": (-0.05, -0.2, -0.5, -1.5),
    "deep": (-0.1, -0.5, -1.5, -3.0),
    "uniform": (-0.25, -0.5, -0.75, -1.0),
    "cm": (-0.02, -0.08, -0.3, -1.0),
    "thick_bottom": (-0.1, -0.4, -1.0, -2.2e6),
    "thin_bottom": (-0.1, -0.4, -1.0, -1.0 - 2.0 ** -21),
    "thin_top": (-2.0 ** -21, -0.4, -1.0, -2.0),
}
# (layering, dt, yearlen, julian)
GROUPS = [
    ("thin", 60.0, 365, 364.9),
    ("thin", 10800.0, 366, 0.0),
    ("deep", 600.0, 365, 200.3),
    ("uniform", 3600.0, 365, 20.3),
    ("cm", 60.0, 366, 366.0),
    ("thick_bottom", 1800.0, 366, 180.3),
    ("thin_bottom", 1800.0, 365, 180.3),
    ("thin_top", 1800.0, 366, 180.3),
]
EDITED = ("thin", "cm")   # layerings whose pools get heavy rain and snow packs
OPTIONS = {
    "base": dict(),
    "veg2": dict(opt_veg=2),
    "combo": dict(opt_veg=4, opt_run=4, opt_rad=2, opt_sfc=2, opt_stc=2, opt_frz=2),
}
SEED = {"base": 701, "veg2": 702, "combo": 703, "traj": 704}
# (layering, dt); 365-day year, from day TRAJ_JULIAN0
TRAJ_GROUPS = [("thin", 10800.0), ("cm", 300.0), ("deep", 10800.0)]
TRAJ_STEPS, TRAJ_KEEP, TRAJ_YEARLEN, TRAJ_JULIAN0 = 16, 32, 365, 360.0


def zsoil_of(name):
    return np.asarray(LAYERINGS[name], np.float32)


def opts_with(**kw):
    d = dict(L.CASE_NML_OPTIONS)
    d.update(kw)
    return L.options_tuple(d)


def traj_julian(julian0, dt, s):
    """Day of step s in fp32 arithmetic, as the engine's time loop (nmp_run_out) advances it."""
    return float(np.float32(julian0) + np.float32(s) * np.float32(dt) / np.float32(86400.0))


# ---- column edits ---------------------------------------------------------------
def set_snow(cols, i, layers, zsoil):
    """Replace column i's snow pack (make_branch_golden.set_snow for any
    layering): layers = [(dz, ice, liq, T)] from the top; [] removes the pack."""
    st = cols.state
    k = len(layers)
    cols.isnow[i] = -k
    for name in ("SNICE", "SNLIQ"):
        st[L.s(name), i] = 0.0
    st[L.s("STC")][:3, i] = 0.0
    zs = st[L.s("ZSNSO")]
    zs[:3, i] = 0.0
    acc = 0.0
    for p, (dz, ice, liq, t) in enumerate(layers):
        j = 3 - k + p
        acc -= dz
        zs[j, i] = acc
        st[L.s("SNICE")][j, i] = ice
        st[L.s("SNLIQ")][j, i] = liq
        st[L.s("STC")][j, i] = t
    h = -acc
    zs[3:, i] = zsoil - np.float32(h)
    st[L.si("SNOWH"), i] = h
    st[L.si("SNEQV"), i] = sum(l[1] + l[2] for l in layers)
    st[L.si("SNEQVO"), i] = st[L.si("SNEQV"), i]
    if k:
        st[L.si("TG"), i] = min(layers[0][3], TFRZ)
        st[L.si("TAUSS"), i] = 0.5
    else:
        st[L.si("TAUSS"), i] = 0.0


def r_heavy_rain(c, f, i, rng, zsoil):
    """10 to 40 mm/h of rain on snow-free ground."""
    set_snow(c, i, [], zsoil)
    f[F("PRCP"), i] = rng.uniform(10.0, 40.0) / 3600.0
    f[F("SFCTMP"), i] = max(f[F("SFCTMP"), i], rng.uniform(276.0, 290.0))
    c.state[L.si("TG"), i] = max(c.state[L.si("TG"), i], TFRZ + 0.5)


def r_snow_pack(c, f, i, rng, zsoil):
    """One to three layers; fresh and light to old and dense, some near melting."""
    k = int(rng.integers(1, 4))
    dz = [rng.uniform(0.026, 0.05), rng.uniform(0.05, 0.2), rng.uniform(0.1, 0.4)][:k]
    warm = rng.uniform() < 0.4
    lay = []
    for p in range(k):
        rho = rng.uniform(60.0, 400.0)
        t = TFRZ - rng.uniform(0.0, 0.3) if warm else rng.uniform(250.0, 272.5)
        lay.append((dz[p], rho * dz[p], rng.uniform(0.0, 0.04) * rho * dz[p] if warm else 0.0, t))
    set_snow(c, i, lay, zsoil)


def make_pool(P, seed, layering, julian, n=POOL):
    zs = zsoil_of(layering)
    cols = cases.make_columns(n, "mixed", P, seed=seed, julian=julian, zsoil=zs)
    f = cases.forcing_random(cols, seed=seed).astype(np.float64)
    if layering in EDITED:
        cols.state = cols.state.astype(np.float64)
        rng = np.random.Generator(np.random.PCG64(seed + 1))
        for i in range(n):
            if i % 4 == 1:
                r_heavy_rain(cols, f, i, rng, zs)
            elif i % 4 == 3:
                r_snow_pack(cols, f, i, rng, zs)
        cols.state = cols.state.astype(np.float32)
    return cols, f.astype(np.float32)


def same_bits(a, b):
    return (np.asarray(a).view(np.int32) == np.asarray(b).view(np.int32)).all(0)


def save(name, **arrays):
    path = os.path.join(HERE, name)
    np.savez_compressed(path, **arrays)
    print("wrote", path, os.path.getsize(path) // 1024, "KB")


def single(name):
    options = opts_with(**OPTIONS[name])
    ref.configure(options)
    P = ref.dump_params()
    bounds = perturb_bounds()
    out = {k: [] for k in ("state0", "isnow0", "static_f", "static_i", "forcing", "state1",
                           "isnow1", "diag", "status", "group")}
    for gi, (layering, dt, yearlen, julian) in enumerate(GROUPS, start=1):
        zs = zsoil_of(layering)
        julian = float(np.float32(julian))   # as stored
        cols, f = make_pool(P, SEED[name] * 100 + gi, layering, julian)
        args = (zs, dt, yearlen, julian, cols.state, cols.isnow, cols.static_f, cols.static_i, f)
        st, isn, dg, status = ref.step(*args)
        pst, pisn, pdg, pstatus, trips = port.step_stats(P, options, *args)
        same = same_bits(pst, st) & same_bits(pdg, dg) & (pisn == isn) & (as_ref_status(pstatus) == status)
        base, discrete, q = port.step_ensemble(P, options, *args, bounds)
        finite = np.isfinite(st).all(0) & np.isfinite(dg).all(0) & (status == 0)
        good = finite & ~discrete & (base[1] == isn)
        keep = np.nonzero(good)[0][:KEEP]
        sub = trips[keep, port.STAT_LOOPS.index("soilwater sub-steps")]
        print(f"{name} group {gi} ({layering}, dt {dt:g}): restatement == reference in "
              f"{int(same.sum())}/{POOL}; finite with status 0: {int(finite.sum())}; discrete "
              f"{int(discrete.sum())}; usable {int(good.sum())}; kept {keep.size}, "
              f"{int((isn[keep] < 0).sum())} with snow layers, soil-water sub-steps "
              f"{dict(zip(*(x.tolist() for x in np.unique(sub, return_counts=True))))}")
        if keep.size < MIN_KEEP:
            raise SystemExit(f"{name}: group {gi} ends with {keep.size} usable columns")
        if not same[keep].all():
            raise SystemExit(f"{name}: group {gi}: the fp32 restatement differs from the "
                             f"reference in kept columns {keep[~same[keep]][:8].tolist()}")
        for k, a in (("state0", cols.state), ("isnow0", cols.isnow), ("static_f", cols.static_f),
                     ("static_i", cols.static_i), ("forcing", f), ("state1", st), ("isnow1", isn),
                     ("diag", dg), ("status", status)):
            out[k].append(a[..., keep])
        out["group"].append(np.full(keep.size, gi, np.int32))
    save(f"layers_{name}.npz", options=np.array(options, np.int32),
         zsoil=np.stack([zsoil_of(g[0]) for g in GROUPS]),
         dt=np.array([g[1] for g in GROUPS], np.float32),
         yearlen=np.array([g[2] for g in GROUPS], np.int32),
         julian=np.array([g[3] for g in GROUPS], np.float32),
         **{k: np.concatenate(v, axis=-1) for k, v in out.items()})


def trajectory():
    options = opts_with(**OPTIONS["base"])
    ref.configure(options)
    P = ref.dump_params()
    out = {k: [] for k in ("state0", "isnow0", "static_f", "static_i", "forcing", "states",
                           "isnows", "diags", "statuses", "group")}
    for gi, (layering, dt) in enumerate(TRAJ_GROUPS, start=1):
        zs = zsoil_of(layering)
        seed = SEED["traj"] * 100 + gi
        cols, _ = make_pool(P, seed, layering, TRAJ_JULIAN0)
        st, isn = cols.state, cols.isnow
        good = np.ones(POOL, bool)
        Fs, S, I, D, ST = [], [], [], [], []
        for s in range(TRAJ_STEPS):
            jul = traj_julian(TRAJ_JULIAN0, dt, s)
            assert jul + dt / 86400.0 <= TRAJ_YEARLEN
            fs = cases.forcing_step(cols, jul, TRAJ_YEARLEN, s, seed=seed)
            st, isn, dg, status = ref.step(zs, dt, TRAJ_YEARLEN, jul, st, isn, cols.static_f,
                                           cols.static_i, fs)
            good &= np.isfinite(st).all(0) & np.isfinite(dg).all(0) & (status == 0)
            Fs.append(fs), S.append(st), I.append(isn), D.append(dg), ST.append(status)
        # snow and snow-free mixed: half of each where the pool has them
        snow = good & ((cols.isnow < 0) | (cols.state[L.si("SNEQV")] > 0))
        a, b = np.nonzero(snow)[0], np.nonzero(good & ~snow)[0]
        na = min(a.size, max(TRAJ_KEEP // 2, TRAJ_KEEP - b.size))
        keep = np.sort(np.concatenate([a[:na], b[:TRAJ_KEEP - na]]))
        if keep.size < TRAJ_KEEP:
            raise SystemExit(f"traj: group {gi} ends with {keep.size} usable columns")
        Fs, S, I, D, ST = (np.stack(x)[..., keep] for x in (Fs, S, I, D, ST))
        # the fp32 restatement over the kept columns, from its own state
        pst, pisn = cols.state[:, keep], cols.isnow[keep]
        for s in range(TRAJ_STEPS):
            pst, pisn, pdg, pstatus = port.step(P, options, zs, dt, TRAJ_YEARLEN,
                                                traj_julian(TRAJ_JULIAN0, dt, s), pst, pisn,
                                                cols.static_f[:, keep], cols.static_i[:, keep],
                                                Fs[s])
            if not (same_bits(pst, S[s]).all() and same_bits(pdg, D[s]).all()
                    and np.array_equal(pisn, I[s]) and np.array_equal(as_ref_status(pstatus), ST[s])):
                raise SystemExit(f"traj: group {gi}: the fp32 restatement differs from the "
                                 f"reference at step {s}")
        print(f"traj group {gi} ({layering}, dt {dt:g}): usable {int(good.sum())}/{POOL}; kept "
              f"{keep.size}, {na} with snow; layer changes per step",
              [int((x != y).sum()) for x, y in zip([cols.isnow[keep]] + list(I[:-1]), I)])
        for k, v in (("state0", cols.state[:, keep]), ("isnow0", cols.isnow[keep]),
                     ("static_f", cols.static_f[:, keep]), ("static_i", cols.static_i[:, keep]),
                     ("forcing", Fs), ("states", S), ("isnows", I), ("diags", D),
                     ("statuses", ST), ("group", np.full(keep.size, gi, np.int32))):
            out[k].append(v)
    G = len(TRAJ_GROUPS)
    save("layers_traj.npz", options=np.array(options, np.int32), keep_every=np.int32(1),
         zsoil=np.stack([zsoil_of(g[0]) for g in TRAJ_GROUPS]),
         dt=np.array([g[1] for g in TRAJ_GROUPS], np.float32),
         yearlen=np.full(G, TRAJ_YEARLEN, np.int32), julian0=np.full(G, TRAJ_JULIAN0, np.float32),
         **{k: np.concatenate(v, axis=-1) for k, v in out.items()})


def check(name):
    """Run the reference on the stored inputs of layers_<name>.npz, group by
    group, and compare with the stored outputs."""
    with np.load(os.path.join(HERE, f"layers_{name}.npz")) as z:
        g = {k: z[k] for k in z.files}
    ref.configure(tuple(int(x) for x in g["options"]))

    def differs(what, got, exp):
        for (a, b), key in zip(zip(got, exp), ("state", "ISNOW", "diag", "status")):
            if not (np.asarray(a).view(np.int32) == np.asarray(b).view(np.int32)).all():
                raise SystemExit(f"layers_{name}: {what}: {key} differs from the reference")

    for k in layer_groups(g):
        q = layer_group(g, k)
        if "states" in q:
            st, isn = q["state0"], q["isnow0"]
            for s in range(q["forcing"].shape[0]):
                st, isn, dg, status = ref.step(
                    q["zsoil"], float(q["dt"]), int(q["yearlen"]),
                    traj_julian(q["julian0"], q["dt"], s), st, isn, q["static_f"], q["static_i"],
                    q["forcing"][s])
                differs(f"group {k} step {s}", (st, isn, dg, status),
                        (q["states"][s], q["isnows"][s], q["diags"][s], q["statuses"][s]))
        else:
            got = ref.step(q["zsoil"], float(q["dt"]), int(q["yearlen"]), float(q["julian"]),
                           q["state0"], q["isnow0"], q["static_f"], q["static_i"], q["forcing"])
            differs(f"group {k}", got, (q["state1"], q["isnow1"], q["diag"], q["status"]))
    print(f"layers_{name}: {g['group'].size} columns in {g['zsoil'].shape[0]} groups "
          "reproduced by the reference")


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--check":
        check(sys.argv[2])
        sys.exit(0)
    if len(sys.argv) == 3 and sys.argv[1] == "--one":
        trajectory() if sys.argv[2] == "traj" else single(sys.argv[2])
        sys.exit(0)
    # the reference keeps its options in process-global variables: one process per fixture
    for g in (sys.argv[1:] or ["base", "veg2", "combo", "traj"]):
        subprocess.run([sys.executable, __file__, "--one", g], check=True)
