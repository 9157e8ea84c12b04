"""Spin-up, host side (no GPU): the numpy restatements of nmp_state_drift and
nmp_drift_reduce (spinup.tracked_host, drift_host, reduce_host) equal a second
restatement written here from the header's text alone with plain Python loops,
bit for bit; parse_tol; and the header, the bindings and the layout mirrors of
the two entries."""
import re
import subprocess

import numpy as np
import pytest

from noahmp_amd import layout as L, lib as _lib, spinup
from test_abi_host import _enum_values, _header
from test_stateout_host import ibits, make_columns, same_bits

NCOLS = [1, 63, 64, 65, 255, 256, 257, 777]
QNAN = 0x7ff8000000000000


# ---- the second restatement: the header's text, one column at a time -----------------
def header_tracked(state, isnow, static_i):
    T = state.dtype.type
    S = L.STATE_OFF
    IST = L.STATIC_I.index("IST")
    n = isnow.shape[0]
    out = np.full((13, n), T(-77), T)
    with np.errstate(all="ignore"):
        for c in range(n):
            st = [T(v) for v in state[:, c]]
            isn = int(isnow[c])
            STC, Z, SMC = st[S["STC"][0]:][:7], st[S["ZSNSO"][0]:][:7], st[S["SMC"][0]:][:4]
            one = lambda name: st[S[name][0]]  # noqa: E731
            for i in range(4):
                out[i, c] = SMC[i]
                out[4 + i, c] = STC[3 + i]
            out[8, c], out[9, c], out[10, c] = one("SNEQV"), one("WA"), one("ZWT")
            if int(static_i[IST, c]) != 1:
                w = T(0)
            else:
                w = ((one("CANLIQ") + one("CANICE")) + one("SNEQV")) + one("WA")
                for i in range(1, 5):
                    zb = Z[i + 2]
                    dz = -zb if i == isn + 1 else Z[i + 1] - zb
                    w = w + (SMC[i - 1] * dz) * T(1000)
            out[11, c] = w
            out[12, c] = ((((one("LFMASS") + one("RTMASS")) + one("STMASS")) + one("WOOD"))
                          + one("STBLCP")) + one("FASTCP")
    return out


def header_drift(now, snap):
    T = now.dtype.type
    n = now.shape[1]
    out = np.full((7, n), T(-77), T)
    with np.errstate(all="ignore"):
        for c in range(n):
            for g, k in ((0, 0), (1, 4)):
                x = [T(abs(T(now[k + i, c] - snap[k + i, c]))) for i in range(4)]
                m = x[0]
                for i in (1, 2, 3):
                    m = x[i] if (x[i] > m or x[i] != x[i]) else m
                out[g, c] = m
            for g, k in ((2, 8), (3, 9), (4, 10), (5, 11), (6, 12)):
                out[g, c] = T(abs(T(now[k, c] - snap[k, c])))
    return out


def header_reduce(drift, tol, weight):
    """(max, arg, wsum, count, wtot) by the header's definitions, in loops."""
    D = np.float64
    n = drift.shape[1]
    w = [D(1.0)] * n if weight is None else [D(v) for v in weight]
    nchunk = -(-n // 256)
    mx, arg, wsum, count = [], [], [], []

    def tree(term):
        total = D(0.0)
        for k in range(nchunk):
            a = np.zeros(64, D)
            for lane in range(64):
                x = D(0.0)
                for j in range(4):
                    c = 256 * k + lane + 64 * j
                    if c >= n or w[c] == 0.0:
                        continue
                    x = x + term(c)
                a[lane] = x
            for s in (32, 16, 8, 4, 2, 1):
                a = a[:s] + a[s:2 * s]
            total = total + a[0]
        return total

    with np.errstate(all="ignore"):
        for g in range(7):
            d = [D(v) for v in drift[g]]
            live = [c for c in range(n) if w[c] != 0.0]
            nans = [c for c in live if d[c] != d[c]]
            if not live:
                mx.append(D(0.0))
                arg.append(-1)
            elif nans:
                mx.append(np.array([QNAN], np.uint64).view(D)[0])
                arg.append(nans[0])
            else:
                m = max(d[c] for c in live)
                mx.append(m)
                arg.append(min(c for c in live if d[c] == m))
            count.append(sum(1 for c in live if not (d[c] <= tol[g])))
            wsum.append(tree(lambda c: d[c] * w[c]))
        wtot = tree(lambda c: w[c])
    return (np.array(mx, D), np.array(arg, np.int64), np.array(wsum, D), np.array(count, np.int64),
            D(wtot))


def planted(dtype, n, seed=0):
    """(drift rows (7, n), weight (n,), tol) from two make_columns states, with
    the cases the header's definitions turn on planted where n has room: a NaN
    drift, a tie for the max (the lowest index must win), a weight-0 column
    holding the largest drift (and a NaN under weight 0), an IST != 1 column."""
    m = max(n, 32)                                         # (make_columns plants up to column 23)
    s0, i0, si = make_columns(dtype, n=m, seed=seed)
    s1, i1, _ = make_columns(dtype, n=m, seed=seed + 100)
    a = spinup.tracked_host(s0[:, :n], i0[:n], si[:, :n])
    b = spinup.tracked_host(s1[:, :n], i1[:n], si[:, :n])
    d = spinup.drift_host(b, a)
    rng = np.random.default_rng(seed)
    w = rng.uniform(0.2, 1.0, n)
    G = L.DRIFT_GROUPS.index
    if n >= 63:
        big = dtype(d[G("SNEQV")].max() * 2)
        d[G("SNEQV"), [40, 17, 61]] = big                  # a tie: 17 must win
        d[G("WA"), 50] = dtype(1e9)                        # the largest, but skipped
        d[G("ZWT"), 50] = np.nan                           # a NaN, but skipped
        w[50] = 0.0
        d[G("TWS"), [33, 9]] = np.nan                      # NaNs: 9 must win
        w[3] = 0.0
    if n >= 257:
        d[G("SOIL_T"), [256, 100]] = dtype(d[G("SOIL_T")].max() * 3)   # a tie across chunks
        d[G("SOIL_M"), n - 1] = dtype(5.0)                 # the max in the last, padded chunk
        w[200:230] = 0.0                                   # a padded run inside a full chunk
    tol = np.array([np.median(d[g][np.isfinite(d[g])]) for g in range(7)], np.float64)
    tol[G("SOIL_M")] = np.inf
    tol[G("CARBON")] = 0.0
    return d, w, tol


def check_result(res, want):
    mx, arg, wsum, count, wtot = want
    assert same_bits(res.max, mx), (res.max, mx)
    assert np.array_equal(res.arg, arg) and res.arg.dtype == np.int64, (res.arg, arg)
    assert same_bits(res.wsum, wsum), (res.wsum, wsum)
    assert np.array_equal(res.count, count), (res.count, count)
    assert same_bits(np.float64(res.wtot), np.float64(wtot))


# ---- the twins -----------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_tracked_and_drift_equal_the_header_restatement(dtype):
    s0, i0, si = make_columns(dtype, n=48, seed=1)
    s1, i1, _ = make_columns(dtype, n=48, seed=2)
    assert set(si[L.STATIC_I.index("IST")].tolist()) == {1, 2}
    a, b = spinup.tracked_host(s0, i0, si), spinup.tracked_host(s1, i1, si)
    assert a.dtype == np.dtype(dtype) and a.shape == (13, 48)
    assert same_bits(a, header_tracked(s0, i0, si)) and same_bits(b, header_tracked(s1, i1, si))
    # TWS is 0 off soil, the water storage elsewhere; CTOT carries the NaN pools
    from test_stateout_host import np_storage
    assert same_bits(a[L.TRACKED["TWS"]], np_storage(s0, i0, si))
    assert (ibits(a[L.TRACKED["TWS"]])[si[L.STATIC_I.index("IST")] == 2] == 0).all()
    assert np.isnan(a[L.TRACKED["CTOT"]][[4, 10, 13]]).all()
    # a NaN in one soil layer sticks whatever layer it is in
    for layer in range(4):
        b2 = b.copy()
        b2[L.TRACKED["STC"] + layer, 7] = np.nan
        d = spinup.drift_host(b2, a)
        assert same_bits(d, header_drift(b2, a))
        assert np.isnan(d[L.DRIFT_GROUPS.index("SOIL_T"), 7])
        assert not np.isnan(d[L.DRIFT_GROUPS.index("SOIL_M"), 7])
    d = spinup.drift_host(b, a)
    assert d.dtype == np.dtype(dtype) and same_bits(d, header_drift(b, a))
    assert np.isnan(d[L.DRIFT_GROUPS.index("CARBON")][[4, 10, 13]]).all()
    assert (d[~np.isnan(d)] >= 0).all()
    assert (ibits(spinup.drift_host(a, a))[~np.isnan(d)] == 0).all()      # no drift: +0.0


@pytest.mark.parametrize("weighted", [True, False], ids=["weights", "no-weights"])
@pytest.mark.parametrize("n", NCOLS)
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_reduce_equals_the_header_restatement(dtype, n, weighted):
    d, w, tol = planted(dtype, n, seed=n)
    w = w if weighted else None
    res = spinup.reduce_host(d, tol, w)
    check_result(res, header_reduce(d, tol, w))
    G = L.DRIFT_GROUPS.index
    if n >= 63:
        assert res.arg[G("SNEQV")] == 17 and res.arg[G("TWS")] == 9
        assert ibits(res.max)[G("TWS")] == QNAN and res.count[G("TWS")] >= 2
        if weighted:
            assert res.arg[G("WA")] != 50 and res.max[G("WA")] < 1e9
            assert not np.isnan(res.max[G("ZWT")]) and not np.isnan(res.wsum[G("ZWT")])
        else:
            assert res.arg[G("WA")] == 50 and np.isnan(res.max[G("ZWT")])
    if n >= 257:
        assert res.arg[G("SOIL_T")] == 100 and res.arg[G("SOIL_M")] == n - 1
    assert res.count[G("SOIL_M")] == 0                      # tol = inf
    assert same_bits(res.mean, res.wsum / np.float64(res.wtot))


def test_reduce_without_an_unskipped_column():
    d, _, tol = planted(np.float32, 65)
    res = spinup.reduce_host(d, tol, np.zeros(65))
    check_result(res, header_reduce(d, tol, np.zeros(65)))
    assert (res.arg == -1).all() and (ibits(res.max) == 0).all() and not res.count.any()
    assert res.wtot == 0.0 and np.isnan(res.mean).all() and res.converged


# ---- parse_tol ------------------------------------------------------------------------
def test_parse_tol():
    inf = np.inf
    t = spinup.parse_tol("SOIL_M=0.001,SOIL_T=0.01")
    assert t.dtype == np.float64 and t.tolist() == [0.001, 0.01, inf, inf, inf, inf, inf]
    assert spinup.parse_tol(" CARBON = 1e-3 , ZWT=0 ").tolist() == [inf] * 4 + [0.0, inf, 1e-3]
    assert spinup.parse_tol({"TWS": 2}).tolist() == [inf] * 5 + [2.0, inf]
    assert spinup.parse_tol([1, 2, 3, 4, 5, 6, inf]).tolist() == [1, 2, 3, 4, 5, 6, inf]
    assert spinup.parse_tol("WA=inf")[3] == inf
    for bad in ("", ",", "SOIL_M", "NOPE=1", "soil_m=1", "SOIL_M=-1", "SOIL_M=nan", "SOIL_M=x",
                "SOIL_M=1,SOIL_M=2", "SOIL_M=", {"NOPE": 1}, {"WA": -0.5}, {"WA": float("nan")},
                [1, 2, 3], [1, 2, 3, 4, 5, 6, -7]):
        with pytest.raises(ValueError):
            spinup.parse_tol(bad)


def test_record_and_bytes():
    r = spinup.SpinupRecord(2, [0.0, float("nan")], [3, -1], [0.5, float("inf")], [0, 4],
                            [1.0, float("inf")])
    assert not r.converged and spinup.SpinupRecord(1, count=[0] * 7).converged
    j = r.as_json()
    assert j["loop"] == 2 and j["max"] == [0.0, "nan"] and j["tol"] == [1.0, "inf"]
    import json
    assert json.loads(json.dumps(j, allow_nan=False)) == j
    b4, b8 = spinup.algorithmic_bytes(4), spinup.algorithmic_bytes(8)
    assert b4["state_drift"] == (24 + 13 + 13 + 7) * 4 + 8 and b8["drift_reduce"] == 7 * 8 + 8
    assert b4["state_drift_snapshot"] == (24 + 13) * 4 + 8


# ---- header, ABI ----------------------------------------------------------------------
def test_header_enums_equal_layout(engine_lib):
    text = _header()
    e = _enum_values(text)
    for name, row in L.TRACKED.items():
        assert e[f"NMP_K_{name}"] == row, name
    assert sum(1 for k in e if k.startswith("NMP_K_")) == len(L.TRACKED) == 7
    assert e["NMP_NTRACKED"] == L.NTRACKED == 13
    for g, name in enumerate(L.DRIFT_GROUPS):
        assert e[f"NMP_G_{name}"] == g, name
    assert sum(1 for k in e if k.startswith("NMP_G_")) == L.NDRIFT == e["NMP_NDRIFT"] == 7
    assert e["NMP_DRIFT_CHUNK"] == L.DRIFT_CHUNK == 256
    assert e["NMP_DRIFT_SCRATCH"] == L.DRIFT_SCRATCH == 29
    assert set(L.DRIFT_UNITS) == set(L.DRIFT_GROUPS)
    assert re.search(r"#define NMP_ABI_VERSION 8\b", text)          # additive: the version stays
    assert engine_lib.nmp_abi_version() == 8
    # the function table at the top and the section that defines the results
    assert re.search(r"nmp_state_drift,\s+no counterpart", text)
    assert re.search(r"\*\s+nmp_drift_reduce\s", text)
    assert "Spin-up drift" in text and "0x7ff8000000000000" in text
    for word in ("out_max", "out_arg", "out_count", "out_wsum", "out_wtot", "NMP_DRIFT_CHUNK = 256"):
        assert word in text, word


def test_entries_exported_and_bound(engine_lib):
    decl = set(re.findall(r"^\s*(?:int|int64_t|void\*?|const char\*)\s*(nmp_\w+)\s*\(", _header(),
                          re.M))
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.library_path()], capture_output=True,
                        text=True, check=True).stdout
    exported = set(re.findall(r"\bT (nmp_\w+)$", nm, re.M))
    for name, nargs in (("nmp_state_drift", 11), ("nmp_drift_reduce", 13)):
        assert name in decl and name in _lib.EXPORTED_SYMBOLS and name in exported
        assert len(getattr(engine_lib, name).argtypes) == nargs
    # a NULL engine is refused before any device is touched
    assert engine_lib.nmp_state_drift(None, 1, 1, None, None, None, None, 1, None, 1, None) == -1
    assert engine_lib.nmp_drift_reduce(None, 1, 1, None, None, None, None, None, None, None, None,
                                       None, None) == -1
    from noahmp_amd import build
    assert "drift.hip" in build.SOURCES
