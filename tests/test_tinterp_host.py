"""Forcing between input times, host side (no GPU): the two C entries'
declaration, export, binding and argument rules, the numpy twin
(tinterp.interp_host) against the operation order restated here from
include/noahmp_engine.h alone and against its stated properties, the size of
the three SWDOWN schemes' error on a clear-sky field, the feed's refusals and
the weights."""
import datetime
import re
import subprocess

import numpy as np
import pytest

from noahmp_amd import feeds, layout as L, lib as _lib, timeman, tinterp
from test_abi_host import _header
from test_regrid_host import _block, bits

V, F = L.LDASIN.index, L.FORCING.index
RAIN, SW = 1 << V("RAINRATE"), 1 << V("SWDOWN")
N = 1031
# forcing row of each of the 8 file variables
FROW = {"T2D": "SFCTMP", "Q2D": "Q2", "U2D": "UU", "V2D": "VV", "PSFC": "PSFC",
        "RAINRATE": "PRCP", "SWDOWN": "SOLDN", "LWDOWN": "LWDN"}


def same(a, b):
    """Bit for bit, a NaN equal to any NaN of the same place."""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))).all())


def blocks(n=N, seed=0):
    """Two plausible blocks whose COSZ rows hold days, nights, sunrises below
    the floor and exact zeros, and the step's COSZ row."""
    rng = np.random.default_rng(seed)
    b0, b1 = _block(n, seed), _block(n, seed + 100)
    czt = rng.uniform(-1, 1, n).astype(np.float32)
    for k, row in enumerate((b0[V("COSZ")], b1[V("COSZ")], czt)):
        row[k:60:3] = rng.uniform(-0.02, 0.049, len(row[k:60:3]))  # below the floor
        row[60 + k:90:3] = 0.0
    night = b0[V("COSZ")] <= 0
    b0[V("SWDOWN"), night] = 0.0
    b1[V("SWDOWN"), b1[V("COSZ")] <= 0] = 0.0
    return b0, b1, czt


# ---- ABI --------------------------------------------------------------------------------
def test_interp_entries_exported(engine_lib):
    decl = set(re.findall(r"^\s*(?:int|int64_t|void\*?|const char\*)\s*(nmp_\w+)\s*\(", _header(),
                          re.M))
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.library_path()], capture_output=True,
                        text=True, check=True).stdout
    exported = set(re.findall(r"\bT (nmp_\w+)$", nm, re.M))
    for name in ("nmp_ldasin_cosz", "nmp_forcing_from_ldasin_interp"):
        assert name in decl, f"{name} not declared in the header"
        assert name in _lib.EXPORTED_SYMBOLS and name in exported
        assert getattr(engine_lib, name).argtypes is not None, f"{name} not bound in lib.py"
    assert re.search(r"#define NMP_ABI_VERSION 8\b", _header())
    assert engine_lib.nmp_abi_version() == 8   # additive: the version stays


def test_interp_entries_refuse_bad_arguments_without_an_engine(engine_lib):
    """Every refused case, with NULL handles (no device is touched)."""
    def interp(ncol=1, ld=1, w1=0.5, mask=RAIN, zen=1, floor=0.05):
        return engine_lib.nmp_forcing_from_ldasin_interp(None, ncol, ld, None, None, w1, mask, zen,
                                                         floor, None, 0.0, 1.0, 0.0, None, None)
    assert interp() == -1
    assert interp(ld=0) == -1                                   # ld < ncol
    assert interp(w1=0.0) == -1 and interp(w1=0.25) == -1       # NULL blocks, geo, forcing
    for w1 in (1.0, -0.25, 1.5, float("nan"), float("inf")):
        assert interp(w1=w1) == -1
    assert interp(mask=1 << V("COSZ")) == -1 and interp(mask=1 << 31) == -1
    for floor in (0.0, -0.1, 1.5, float("nan")):
        assert interp(floor=floor) == -1
    assert interp(ncol=0, ld=0) == -1                           # no engine
    assert engine_lib.nmp_ldasin_cosz(None, 1, 1, None, 0.0, 1.0, 0.0, None, None) == -1
    assert engine_lib.nmp_ldasin_cosz(None, 1, 0, None, 0.0, 1.0, 0.0, None, None) == -1
    # the twin refuses the same values
    b0, b1, czt = blocks(8)
    for kw in (dict(w1=1.0), dict(w1=-0.5), dict(w1=float("nan")), dict(hold_mask=1 << V("COSZ")),
               dict(cosz_floor=0.0), dict(cosz_floor=1.5), dict(cosz_floor=float("nan"))):
        args = dict(w1=0.5, hold_mask=RAIN, sw_zenith=True, cosz_floor=0.05)
        args.update(kw)
        with pytest.raises(ValueError):
            tinterp.interp_host(b0, b1, cosz_t=czt, **args)
    tinterp.interp_host(b0, b1, 0.5, czt, RAIN, False, 0.0)     # the floor is not looked at
    with pytest.raises(ValueError):
        tinterp.hold_mask(("COSZ",))
    assert tinterp.hold_mask(("RAINRATE", "SWDOWN")) == RAIN | SW == tinterp.hold_mask((5, 6))


# ---- the twin ---------------------------------------------------------------------------
def restated(b0, b1, w1, czt, mask, zen, floor):
    """nmp_forcing_from_ldasin_interp as the header words it, column by column
    in Python floats (IEEE double), fp32 through numpy scalars."""
    f32 = np.float32
    n = b0.shape[1]
    out = np.empty((L.NFORCING, n), np.float32)
    w0 = 1.0 - w1
    with np.errstate(all="ignore"):
        for c in range(n):
            r = {}
            for name in L.LDASIN[:-1]:
                v = V(name)
                a = float(b0[v, c])
                if w1 == 0.0 or (mask >> v) & 1:
                    r[name] = b0[v, c]
                elif zen and name == "SWDOWN":
                    cz0, cz1 = float(b0[V("COSZ"), c]), float(b1[V("COSZ"), c])
                    m0 = cz0 if cz0 > floor else floor
                    m1 = cz1 if cz1 > floor else floor
                    k0 = float(np.float64(a) / np.float64(m0))
                    k1 = float(np.float64(b1[v, c]) / np.float64(m1))
                    k = k0 * w0 + k1 * w1
                    ct = float(czt[c])
                    r[name] = f32(ct * k if ct > 0 else 0.0)
                else:
                    r[name] = f32(a * w0 + float(b1[v, c]) * w1)
            for name, fld in FROW.items():
                out[F(fld), c] = r[name]
            out[F("SFCPRS"), c] = r["PSFC"]
            out[F("COSZ"), c] = czt[c]
            out[F("CO2AIR"), c] = f32(395.0e-6 * float(r["PSFC"]))
            out[F("O2AIR"), c] = f32(0.209 * float(r["PSFC"]))
    return out


def test_interp_host_is_the_documented_operation_order():
    b0, b1, czt = blocks(200, seed=3)
    b0[V("T2D"), 3], b1[V("Q2D"), 4], b0[V("SWDOWN"), 5] = np.nan, np.nan, -0.0
    b1[V("COSZ"), 6], czt[7] = np.nan, np.nan
    for w1 in (0.0, 2.0 ** -20, 1 / 3, 0.5, 1 - 2.0 ** -20):
        for mask in (0, RAIN, RAIN | SW, 0xFF):
            for zen in (True, False):
                got = tinterp.interp_host(b0, b1, w1, czt, mask, zen, 0.05)
                assert got.dtype == np.float32 and got.shape == (L.NFORCING, 200)
                assert same(got, restated(b0, b1, w1, czt, mask, zen, 0.05)), (w1, mask, zen)


def test_twin_properties():
    b0, b1, czt = blocks()
    nan1 = np.full_like(b1, np.nan)
    # w1 = 0: block 0's variables, whatever block 1 holds (or None)
    for blk1 in (nan1, None):
        got = tinterp.interp_host(b0, blk1, 0.0, czt, RAIN, True, 0.05)
        for var, fld in FROW.items():
            assert np.array_equal(bits(got[F(fld)]), bits(b0[V(var)])), var
        assert np.array_equal(bits(got[F("COSZ")]), bits(czt))
        assert np.array_equal(bits(got[F("SFCPRS")]), bits(b0[V("PSFC")]))
    for w1 in (2.0 ** -20, 0.25, 1 / 3, 0.5, 11 / 12, 1 - 2.0 ** -20):
        got = tinterp.interp_host(b0, b1, w1, czt, RAIN, True, 0.05)
        for var in ("T2D", "Q2D", "U2D", "V2D", "PSFC", "LWDOWN"):   # between the end points
            lo, hi = np.minimum(b0[V(var)], b1[V(var)]), np.maximum(b0[V(var)], b1[V(var)])
            assert ((got[F(FROW[var])] >= lo) & (got[F(FROW[var])] <= hi)).all(), (var, w1)
        assert np.array_equal(bits(got[F("PRCP")]), bits(b0[V("RAINRATE")]))   # held
        sw = got[F("SOLDN")]
        assert (sw >= 0).all() and (sw[~(czt > 0)] == 0).all() and (sw[czt > 0] > 0).any()
        allheld = tinterp.interp_host(b0, nan1, w1, czt, 0xFF, True, 0.05)
        for var, fld in FROW.items():
            assert np.array_equal(bits(allheld[F(fld)]), bits(b0[V(var)])), var
        # SWDOWN held or plain does not read the COSZ rows
        for mask, zen in ((RAIN | SW, True), (RAIN, False)):
            x0, x1 = b0.copy(), b1.copy()
            x0[V("COSZ")] = x1[V("COSZ")] = np.nan
            assert same(tinterp.interp_host(x0, x1, w1, czt, mask, zen, 0.05),
                        tinterp.interp_host(b0, b1, w1, czt, mask, zen, 0.05))
    # where both end points are darker than the floor and the files' SWDOWN is 0: 0
    dark = (b0[V("COSZ")] <= 0) & (b1[V("COSZ")] <= 0)
    assert dark.any()
    assert (tinterp.interp_host(b0, b1, 0.5, czt, RAIN, True, 0.05)[F("SOLDN")][dark] == 0).all()


def test_a_nan_stays_in_its_row_and_column():
    b0, b1, czt = blocks()
    czt[:] = np.abs(czt) + np.float32(0.1)
    clean = tinterp.interp_host(b0, b1, 0.25, czt, RAIN, True, 0.05)
    assert np.isfinite(clean).all()
    derived = {"PSFC": ("SFCPRS", "PSFC", "CO2AIR", "O2AIR")}
    for j, var in enumerate(L.LDASIN[:-1]):
        for which in (0, 1):
            if which == 1 and var == "RAINRATE":
                continue   # held: block 1's row is not read
            x = [b0.copy(), b1.copy()]
            x[which][V(var), 10 + j] = np.nan
            got = tinterp.interp_host(x[0], x[1], 0.25, czt, RAIN, True, 0.05)
            bad = np.argwhere(np.isnan(got))
            rows = {F(f) for f in derived.get(var, (FROW[var],))}
            assert {int(r) for r, _ in bad} == rows and {int(c) for _, c in bad} == {10 + j}, var
            keep = np.ones_like(got, bool)
            keep[:, 10 + j] = False
            assert np.array_equal(bits(got[keep]), bits(clean[keep]))
    # a NaN in block 1's held row, or in an end point's COSZ, leaks nowhere
    x1 = b1.copy()
    x1[V("RAINRATE"), 3] = x1[V("COSZ"), 4] = np.nan
    assert np.isfinite(tinterp.interp_host(b0, x1, 0.25, czt, RAIN, True, 0.05)).all()
    czt[5] = np.nan   # the step's own COSZ: its row, and SWDOWN = 0
    got = tinterp.interp_host(b0, b1, 0.25, czt, RAIN, True, 0.05)
    assert np.isnan(got[F("COSZ"), 5]) and got[F("SOLDN"), 5] == 0.0
    assert np.isnan(got).sum() == 1


# ---- the size of the schemes' error ---------------------------------------------------------
def test_clear_sky_swdown_error_of_the_three_schemes():
    """sw = S max(cz, 0) on 4,000 columns within +-60 degrees latitude, 3-hourly
    files (end points rounded to fp32), 900 s steps, four days of the year.
    Where both end points are at or above the floor and the sun is up the
    zenith scheme returns S czt to two fp32 roundings (the end point's SWDOWN,
    then the result: relative 2 x 2^-24; the double operations add ~1e-16):
    bound 2^-22.  Over all samples the three schemes' mean absolute errors are
    ordered, whatever their size."""
    n, S, floor = 4000, 1000.0, 0.05
    rng = np.random.default_rng(11)
    lat, lon = np.radians(rng.uniform(-60, 60, n)), np.radians(rng.uniform(-180, 180, n))
    sc = (np.sin(lat), np.cos(lat))
    every, dt = datetime.timedelta(hours=3), datetime.timedelta(seconds=900)

    def block(t):
        b = np.zeros((L.NLDASIN, n), np.float32)
        b[V("COSZ")] = tinterp.cosz_row_host(lat, lon, t, sc)
        b[V("SWDOWN")] = (S * np.maximum(b[V("COSZ")].astype(np.float64), 0.0)).astype(np.float32)
        return b
    err = {"held": 0.0, "linear": 0.0, "zenith": 0.0}
    worst, count = 0.0, 0
    for day in ((3, 21), (6, 21), (9, 23), (12, 21)):
        t0 = datetime.datetime(2001, *day)
        b1 = block(t0)
        for _ in range(8):
            b0, b1 = b1, block(t0 + every)
            for k in range(12):
                t = t0 + k * dt
                w1 = tinterp.weights(t, t0, every)[1]
                czt = tinterp.cosz_row_host(lat, lon, t, sc)
                truth = S * np.maximum(czt.astype(np.float64), 0.0)
                zen = tinterp.interp_host(b0, b1, w1, czt, RAIN, True, floor)[F("SOLDN")]
                lin = tinterp.interp_host(b0, b1, w1, czt, RAIN, False, floor)[F("SOLDN")]
                err["held"] += np.abs(b0[V("SWDOWN")] - truth).sum()
                err["linear"] += np.abs(lin - truth).sum()
                err["zenith"] += np.abs(zen - truth).sum()
                ok = (b0[V("COSZ")] >= floor) & (b1[V("COSZ")] >= floor) & (czt > 0)
                if w1 != 0.0 and ok.any():
                    rel = np.abs(zen[ok] - truth[ok]) / truth[ok]
                    worst = max(worst, float(rel.max()))
                count += n
            t0 = t0 + every
    mae = {k: v / count for k, v in err.items()}
    print(f"clear-sky SWDOWN MAE (W/m2): held {mae['held']:.1f}, linear {mae['linear']:.1f}, "
          f"zenith {mae['zenith']:.1f}; zenith's worst relative error above the floor "
          f"{worst / 2.0 ** -24:.2f} x 2^-24")
    assert worst <= 2.0 ** -22
    assert mae["zenith"] < mae["linear"] < mae["held"]


# ---- the feed's choice and the weights --------------------------------------------------------
class _Files:
    """What feed_kind asks of a file provider."""
    plan = None

    def raw(self, *a):
        raise AssertionError("no file is read")
    grid_raw = raw


def test_feed_kind_interp():
    fr = _Files()
    assert feeds.feed_kind(fr) == "ldasin-ingest" and feeds.feed_kind(fr, interp=False) == \
        "ldasin-ingest"
    assert feeds.feed_kind(fr, interp=True) == "ldasin-interp"
    assert feeds.feed_kind(fr, ingest=False, interp=True) == "ldasin-interp"
    fr.plan, fr.dz = object(), lambda: None
    assert feeds.feed_kind(fr) == "ldasin-regrid"
    assert feeds.feed_kind(fr, interp=True) == "ldasin-interp"
    assert feeds.feed_kind(fr, downscale=True, interp=True) == "ldasin-interp"
    with pytest.raises(ValueError, match="interp"):
        feeds.feed_kind(fr, cosz="host", interp=True)
    with pytest.raises(ValueError, match="interp"):
        feeds.feed_kind(fr, ldasin_upload=False, interp=True)
    with pytest.raises(ValueError, match="interp"):
        feeds.feed_kind(lambda k, t: None, interp=True)          # no files
    with pytest.raises(ValueError, match="interp"):
        feeds.feed_kind("device", interp=True)
    with pytest.raises(ValueError, match="interp"):
        feeds.feed_kind(feeds.DeviceSyntheticForcing(np.zeros((L.NCLIM, 1))), interp=True)
    with pytest.raises(ValueError, match="interp"):
        feeds.feed_kind(None, interp=True)
    # without interp the other paths are as before
    assert feeds.feed_kind(fr, cosz="host") == "ldasin-step"
    assert feeds.feed_kind("device") == "device-synth" and feeds.feed_kind(None) == "host"


def test_weights():
    t0, every = datetime.datetime(2000, 1, 1, 9), datetime.timedelta(hours=3)
    assert tinterp.weights(t0, t0, every) == (1.0, 0.0)
    assert tinterp.weights(t0 + every / 2, t0, every) == (0.5, 0.5)
    w0, w1 = tinterp.weights(t0 + every - datetime.timedelta(seconds=900), t0, every)
    assert w1 == 9900.0 / 10800.0 and w0 == 1.0 - w1 and w1 < 1.0
    for bad in (t0 + every, t0 - datetime.timedelta(seconds=1)):
        with pytest.raises(ValueError):
            tinterp.weights(bad, t0, every)
    # the COSZ row is timeman.cosz's, rounded once
    lat, lon = np.radians([40.0, -33.0]), np.radians([-105.0, 151.0])
    t = datetime.datetime(2001, 6, 21, 18, 15)
    want = timeman.cosz(lat, lon, timeman.julian(t), 365).astype(np.float32)
    assert np.array_equal(bits(tinterp.cosz_row_host(lat, lon, t)), bits(want))
