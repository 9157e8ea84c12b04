"""State output, host side (no GPU): the header's NMP_X_* groups equal
layout.STATE_OUT, the entry is exported and bound, the numpy twin
(stateout.state_output_host) equals a second restatement written here from the
header's text alone with plain Python loops, bit for bit, and the LDASOUT
writers carry layered state variables (and still write today's bytes without
them)."""
import datetime
import re
import subprocess
import types

import numpy as np
import pytest

from noahmp_amd import cases, layout as L, lib as _lib, ncio, stateout
from noahmp_amd.params import Params
from test_abi_host import _enum_values, _header

T0 = datetime.datetime(2000, 1, 1)
FILL = float(ncio.FILL)
NCOL = 48


def ibits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize])


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(ibits(a), ibits(b))


def make_columns(dtype, n=NCOL, ld=None, seed=0):
    """(state (56, ld), isnow, static_i (6, ld)) whose first n columns cover
    ISNOW 0..-3, IST 1 and 2, a VEGTYP with nroot == 0 (16), snow layers of
    zero mass, NaN carbon pools and SOILTYP / VEGTYP outside their tables."""
    ld = n if ld is None else ld
    rng = np.random.default_rng(seed)
    state = (rng.random(size=(L.NSTATE, ld)) * 0.5 + 0.05).astype(dtype)
    z = -np.cumsum(rng.random(size=(7, ld)) * 0.4 + 0.01, axis=0)
    state[L.s("ZSNSO")] = z.astype(dtype)
    state[L.s("STC")] = (250.0 + 40.0 * rng.random(size=(7, ld))).astype(dtype)
    state[L.s("SNICE")] = (rng.random(size=(3, ld)) * 60.0).astype(dtype)
    state[L.s("SNLIQ")] = (rng.random(size=(3, ld)) * 6.0).astype(dtype)
    state[L.si("SNEQV")] = (rng.random(ld) * 80.0).astype(dtype)
    state[L.si("WA")] = (4000.0 + rng.random(ld) * 2000.0).astype(dtype)
    isnow = (-(np.arange(ld) % 4)).astype(np.int32)                 # 0, -1, -2, -3, ...
    static_i = np.ones((L.NSTATIC_I, ld), np.int32)
    static_i[L.STATIC_I.index("IST")] = np.where(np.arange(ld) % 5 == 3, 2, 1)
    static_i[L.STATIC_I.index("VEGTYP")] = rng.integers(1, 28, ld)
    static_i[L.STATIC_I.index("SOILTYP")] = rng.integers(1, 20, ld)
    V, S = L.STATIC_I.index("VEGTYP"), L.STATIC_I.index("SOILTYP")
    static_i[V, [2, 9, 16]] = 16                                    # nroot == 0
    static_i[V, 11] = 15                                            # nroot == 4
    static_i[S, 5], static_i[S, 14], static_i[S, 23] = 0, 31, -7    # outside the soil table
    static_i[V, 6], static_i[V, 21] = 28, 0                         # outside the veg table
    # zero-mass snow: column 1 (isnow -1) its only layer, column 2 (isnow -2) one of two,
    # column 7 (isnow -3) all three
    for c, layers in ((1, (2,)), (2, (1,)), (7, (0, 1, 2))):
        for k in layers:
            state[L.si("SNICE") + k, c] = 0
            state[L.si("SNLIQ") + k, c] = 0
    state[L.si("LFMASS"):L.si("FASTCP") + 1, [4, 10]] = np.nan      # NaN carbon pools (H13)
    state[L.si("WOOD"), 13] = np.nan
    assert isnow[1] == -1 and isnow[2] == -2 and isnow[7] == -3
    return state, isnow, static_i


# ---- the second restatement: the header's text, one column at a time ---------------
def header_twin(state, isnow, static_i, smcmax_tab, nroot_tab, groups, fill):
    T = state.dtype.type
    D = np.float64
    nan = T(np.nan)
    S = L.STATE_OFF
    IST, VEG, SOIL = (L.STATIC_I.index(k) for k in ("IST", "VEGTYP", "SOILTYP"))
    widths = [w for _, w, _ in L.STATE_OUT]
    n = isnow.shape[0]
    out = np.full((sum(w for g, w in enumerate(widths) if groups >> g & 1), n), T(-77), T)
    with np.errstate(all="ignore"):
        for c in range(n):
            st = [T(v) for v in state[:, c]]
            isn = int(isnow[c])
            STC, Z = st[S["STC"][0]:][:7], st[S["ZSNSO"][0]:][:7]
            SNICE, SNLIQ = st[S["SNICE"][0]:][:3], st[S["SNLIQ"][0]:][:3]
            SH2O, SMC = st[S["SH2O"][0]:][:4], st[S["SMC"][0]:][:4]
            one = lambda name: st[S[name][0]]  # noqa: E731
            dz = []
            for i in range(1, 5):
                zb = Z[i + 2]
                dz.append(-zb if i == isn + 1 else Z[i + 1] - zb)
            active = [k >= isn + 3 for k in range(3)]
            rows = {}
            rows[0], rows[1], rows[2] = list(SMC), list(SH2O), list(STC[3:7])
            for g, name in enumerate(["SNEQV", "SNOWH", "TG", "TV", "LAI", "SAI", "ZWT", "WA"]):
                rows[3 + g] = [one(name)]
            rows[11] = [one("CANLIQ") + one("CANICE")]
            rows[12] = [T(isn)]
            x = T(0)
            for k in range(3):
                if active[k]:
                    x = x + SNLIQ[k]
            rows[13] = [x]
            if int(static_i[IST, c]) != 1:
                w = T(0)
            else:
                w = ((one("CANLIQ") + one("CANICE")) + one("SNEQV")) + one("WA")
                for i in range(4):
                    w = w + (SMC[i] * dz[i]) * T(1000)
            rows[14] = [w]
            styp = int(static_i[SOIL, c])
            if 1 <= styp <= len(smcmax_tab):
                num, den = D(0.0), D(0.0)
                for i in range(4):
                    num = num + D(SMC[i]) * D(dz[i])
                    den = den + D(np.float32(smcmax_tab[styp - 1])) * D(dz[i])
                rows[15] = [T(num / den)]
            else:
                rows[15] = [nan]
            vtyp = int(static_i[VEG, c])
            if 1 <= vtyp <= len(nroot_tab):
                nroot = int(nroot_tab[vtyp - 1])
                num, den = D(0.0), D(0.0)
                for i in range(1, 5):
                    if i <= nroot:
                        num = num + D(SMC[i - 1]) * D(dz[i - 1])
                        den = den + D(dz[i - 1])
                rows[16] = [T(0) if nroot < 1 else T(num / den)]
            else:
                rows[16] = [nan]
            rows[17] = [one(p) for p in ("LFMASS", "RTMASS", "STMASS", "WOOD", "STBLCP", "FASTCP")]
            f = T(fill)
            rows[18] = [STC[k] if active[k] else f for k in range(3)]
            zs = []
            for k in range(3):
                if not active[k]:
                    zs.append(f)
                elif k == isn + 3:
                    zs.append(-Z[k])
                else:
                    zs.append(Z[k - 1] - Z[k])
            rows[19] = zs
            num, den = D(0.0), D(0.0)
            for k in range(3):
                if active[k]:
                    m = D(SNICE[k] + SNLIQ[k])
                    num = num + m * D(STC[k])
                    den = den + m
            rows[20] = [f if isn == 0 or den == 0 else T(num / den)]
            k = 0
            for g in range(len(widths)):
                if groups >> g & 1:
                    assert len(rows[g]) == widths[g]
                    for v in rows[g]:
                        out[k, c] = v
                        k += 1
    return out


def np_storage(state, isnow, static_i):
    """The column water storage as tests/test_gpu_accum.py restates it
    (BEG_WB / END_WB in the arrays' own precision); 0 off soil."""
    T = state.dtype.type
    one = lambda name, k=0: state[L.STATE_OFF[name][0] + k]  # noqa: E731
    w = ((one("CANLIQ") + one("CANICE")) + one("SNEQV")) + one("WA")
    for iz in range(1, 5):
        zb = one("ZSNSO", iz + 2)
        dz = np.where(isnow + 1 == iz, -zb, one("ZSNSO", iz + 1) - zb)
        w = w + (one("SMC", iz - 1) * dz) * T(1000)
    return np.where(static_i[L.STATIC_I.index("IST")] == 1, w, T(0))


@pytest.fixture(scope="module")
def tables():
    return Params.builtin().as_dict()


# ---- header, ABI -------------------------------------------------------------------
def test_header_groups_equal_layout(engine_lib):
    text = _header()
    e = _enum_values(text)
    for g, (name, _, _) in enumerate(L.STATE_OUT):
        assert e[f"NMP_X_{name}"] == g, name
    assert e["NMP_NXGROUP"] == L.NXGROUP == 21
    assert sum(1 for k in e if k.startswith("NMP_X_")) == L.NXGROUP
    m = re.search(r"#define NMP_X_WIDTHS \{([^}]*)\}", text)
    widths = [int(v) for v in m.group(1).split(",")]
    assert widths == [w for _, w, _ in L.STATE_OUT]
    nofill = int(re.search(r"#define NMP_NXROWS_NOFILL (\d+)", text).group(1))
    assert nofill == L.NXROWS_NOFILL == sum(w for _, w, f in L.STATE_OUT if not f) == 32
    assert int(re.search(r"#define NMP_NXROWS (\d+)", text).group(1)) == L.NXROWS == sum(widths)
    # the groups that can hold the fill value are the last ones
    flags = [f for _, _, f in L.STATE_OUT]
    assert flags == sorted(flags) and flags.count(True) == 3
    assert re.search(r"#define NMP_ABI_VERSION 8\b", text)          # additive: the version stays
    assert engine_lib.nmp_abi_version() == 8
    assert re.search(r"nmp_state_output\s+no counterpart", text)


def test_entry_exported_and_bound(engine_lib):
    decl = set(re.findall(r"^\s*(?:int|int64_t|void\*?|const char\*)\s*(nmp_\w+)\s*\(", _header(),
                          re.M))
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.library_path()], capture_output=True,
                        text=True, check=True).stdout
    exported = set(re.findall(r"\bT (nmp_\w+)$", nm, re.M))
    name = "nmp_state_output"
    assert name in decl and name in _lib.EXPORTED_SYMBOLS and name in exported
    assert engine_lib.nmp_state_output.argtypes is not None
    # refused before any device is touched
    assert engine_lib.nmp_state_output(None, 1, 1, None, None, None, 1, -9999.0, None, 1, None) == -1
    from noahmp_amd import build
    assert "stateout.hip" in build.SOURCES


# ---- the twin ----------------------------------------------------------------------
MASKS = [stateout.ALL, 1 << 15 | 1 << 16, 1 << 0 | 1 << 13 | 1 << 19, 1 << 20]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_twin_equals_the_header_restatement(tables, dtype):
    state, isnow, static_i = make_columns(dtype)
    assert set(isnow.tolist()) == {0, -1, -2, -3}
    assert set(static_i[L.STATIC_I.index("IST")].tolist()) == {1, 2}
    assert tables["nroot"][15] == 0 and tables["nroot"][14] == 4
    for mask in MASKS:
        got = stateout.state_output_host(state, isnow, static_i, tables, mask, FILL, dtype)
        want = header_twin(state, isnow, static_i, tables["smcmax"], tables["nroot"], mask, FILL)
        assert got.shape[0] == len(stateout.rows(mask))
        for k, (name, layer) in enumerate(stateout.rows(mask)):
            assert same_bits(got[k], want[k]), (hex(mask), name, layer)
    full = stateout.state_output_host(state, isnow, static_i, tables, stateout.ALL, FILL, dtype)
    names = stateout.row_names(stateout.ALL)
    row = lambda n: full[names.index(n)]  # noqa: E731
    nan32 = ibits(np.array([np.nan], dtype))[0]
    # outside the tables: quiet NaN in exactly that row; nroot == 0: +0.0
    assert (ibits(row("SOILSAT"))[[5, 14, 23]] == nan32).all()
    assert (ibits(row("ROOT_M"))[[6, 21]] == nan32).all()
    assert np.isnan(row("SOILSAT")).sum() == 3 and np.isnan(row("ROOT_M")).sum() == 2
    assert (ibits(row("ROOT_M"))[[2, 9, 16]] == 0).all()
    # fill: inactive layers, no snow, a snow pack of zero mass; nowhere in the no-fill rows
    f = dtype(FILL)
    assert (row("SNOWT_AVG")[isnow == 0] == f).all() and row("SNOWT_AVG")[1] == f
    assert row("SNOWT_AVG")[7] == f and row("SNOWT_AVG")[2] != f
    for k in range(3):
        inactive = k < isnow + 3
        assert (row(f"SNOW_T_{k + 1}")[inactive] == f).all()
        assert (row(f"SNOW_Z_{k + 1}")[inactive] == f).all()
        assert (row(f"SNOW_Z_{k + 1}")[~inactive] > 0).all()
    assert not (full[:L.NXROWS_NOFILL] == f).any()
    assert np.isnan(row("LFMASS")[[4, 10]]).all() and np.isnan(row("WOOD")[13])
    assert same_bits(row("SOIL_T_1"), state[L.si("STC") + 3])


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_tws_is_the_water_storage(tables, dtype):
    state, isnow, static_i = make_columns(dtype, seed=3)
    got = stateout.state_output_host(state, isnow, static_i, tables,
                                     stateout.parse_groups("TWS"), FILL, dtype)
    assert got.shape == (1, NCOL)
    assert same_bits(got[0], np_storage(state, isnow, static_i))
    assert (ibits(got[0])[static_i[L.STATIC_I.index("IST")] == 2] == 0).all()


def test_parse_groups_and_rows():
    assert stateout.parse_groups("all") == stateout.ALL == (1 << 21) - 1
    assert stateout.parse_groups("SOIL_M,SNEQV") == 1 | 1 << 3
    assert stateout.parse_groups(["SNEQV", "SOIL_M"]) == 1 | 1 << 3
    assert stateout.parse_groups(" SNOW_T , CARBON ") == 1 << 18 | 1 << 17
    for bad in ("", ",", "SOIL_M,NOPE", "soil_m", [], ["ALL"]):
        with pytest.raises(ValueError):
            stateout.parse_groups(bad)
    for bad in (0, 1 << 21, -1):
        with pytest.raises(ValueError):
            stateout.rows(bad)
    r = stateout.rows(stateout.parse_groups("SOIL_M,SNOW_T,SNEQV,CARBON"))
    assert r == ([("SOIL_M", k) for k in range(4)] + [("SNEQV", None)] +
                 [(p, None) for p in L.CARBON_POOLS] + [("SNOW_T", k) for k in range(3)])
    assert len(stateout.rows(stateout.ALL)) == L.NXROWS
    assert stateout.nofill_rows(stateout.ALL) == L.NXROWS_NOFILL
    assert stateout.nofill_rows(stateout.parse_groups("SNOW_T,SNEQV")) == 1
    names = stateout.row_names(stateout.ALL)
    assert len(set(names)) == L.NXROWS and not set(names) & set(L.DIAG_OUT_ACC)
    v = stateout.variables(L.DIAG_OUT + names)
    assert [x[0] for x in v[:16]] == L.DIAG_OUT and all(x[3] is None for x in v[:16])
    assert ("SOIL_M", 16, 4, "soil_layers_stag") in v and ("SNOW_Z", 16 + 35, 3, "snow_layers") in v
    assert sum(x[2] for x in v) == 16 + L.NXROWS


# ---- LDASOUT -----------------------------------------------------------------------
def _grid(ref_params, seed=8):
    from test_ncio import grid_for
    cols = cases.make_columns(32, "mixed", ref_params, seed=seed)
    return grid_for(cols)


def test_header_without_state_rows_is_the_present_one(tmp_path, ref_params):
    grid = _grid(ref_params)
    for names in (L.DIAG_OUT, L.DIAG_OUT_ACC):
        diag = np.random.default_rng(2).normal(size=(len(names), 32)).astype(np.float32)
        a = str(tmp_path / "a.nc")
        ncio.write_ldasout(a, grid, diag, T0, names=names)        # the scipy path
        raw = open(a, "rb").read()
        hdr = ncio.ldasout_header(grid, "f4", T0, names)
        assert raw.startswith(hdr) and len(raw) == len(hdr) + len(names) * 40 * 4
        assert b"soil_layers_stag" not in hdr and b"snow_layers" not in hdr
    assert ncio.ldasout_header(grid, "f4", T0) == ncio.ldasout_header(grid, "f4", T0, L.DIAG_OUT)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_layered_state_variables(tmp_path, ref_params, tables, dtype):
    from scipy.io import netcdf_file
    grid = _grid(ref_params)
    ny, nx = grid.shape
    mask = stateout.parse_groups("SOIL_M,SNOW_T,SNEQV,CARBON")
    names = L.DIAG_OUT + stateout.row_names(mask)
    assert len(names) == 16 + 14
    state, isnow, static_i = make_columns(dtype, n=32)
    rng = np.random.default_rng(5)
    block = np.concatenate([rng.normal(size=(16, 32)).astype(dtype),
                            stateout.state_output_host(state, isnow, static_i, tables, mask,
                                                       FILL, dtype)])
    full = np.stack([grid.scatter(block[i], np.asarray(ncio.FILL, dtype)).reshape(-1)
                     for i in range(len(names))]).astype(np.dtype(dtype).newbyteorder(">"))
    a, b = str(tmp_path / "a.nc"), str(tmp_path / "b.nc")
    ncio.write_ldasout(a, grid, block, T0, names=names)
    ncio.write_ldasout_grids(b, grid, full, T0, names=names)
    assert open(a, "rb").read() == open(b, "rb").read()
    f = netcdf_file(b, "r", mmap=False)
    try:
        assert f.dimensions["soil_layers_stag"] == 4 and f.dimensions["snow_layers"] == 3
        assert list(f.variables) == (L.DIAG_OUT + ["SOIL_M", "SNEQV"] + L.CARBON_POOLS +
                                     ["SNOW_T"])
        assert f.variables["SOIL_M"].dimensions == ("Time", "soil_layers_stag", "south_north",
                                                    "west_east")
        assert f.variables["SOIL_M"].shape == (1, 4, ny, nx)
        assert f.variables["SNOW_T"].dimensions == ("Time", "snow_layers", "south_north",
                                                    "west_east")
        assert f.variables["SNOW_T"].shape == (1, 3, ny, nx)
        assert f.variables["SNEQV"].shape == f.variables["WOOD"].shape == (1, ny, nx)
        for name in ("SOIL_M", "SNOW_T", "SNEQV", "WOOD", "FSA"):
            assert f.variables[name]._FillValue == ncio.FILL
        sm, snt = np.array(f.variables["SOIL_M"][0]), np.array(f.variables["SNOW_T"][0])
        for k in range(4):      # layer-major: layer k of the variable is row SOIL_M_<k+1>
            assert same_bits(grid.columns(sm[k]).astype(dtype), state[L.si("SMC") + k])
            assert (sm[k][~grid.mask] == ncio.FILL).all()
        for k in range(3):
            want = np.where(k >= isnow + 3, state[L.si("STC") + k], dtype(FILL))
            assert same_bits(grid.columns(snt[k]).astype(dtype), want)
    finally:
        f.close()
    assert same_bits(ncio.read_ldasout(b, grid, names), block)
    assert same_bits(ncio.read_ldasout(b, grid), block[:16])


def test_2gib_refusal_counts_the_state_rows():
    grid = types.SimpleNamespace(shape=(4096, 4096))       # 64 MiB per fp32 grid
    assert len(ncio.ldasout_header(grid, "f4", T0)) > 0    # 16 fields: 1 GiB
    names = L.DIAG_OUT + stateout.row_names(stateout.ALL)  # 55 grids: 3.4 GiB
    with pytest.raises(ValueError, match="2 GiB"):
        ncio.ldasout_header(grid, "f4", T0, names)
    # 31 grids fit, 32 do not: the layered variables' bytes are counted
    fit = L.DIAG_OUT + stateout.row_names(stateout.parse_groups("SOIL_M,SOIL_W,SOIL_T,SNOW_T"))
    assert len(fit) == 31 and len(ncio.ldasout_header(grid, "f4", T0, fit)) > 0
    with pytest.raises(ValueError, match="2 GiB"):
        ncio.ldasout_header(grid, "f4", T0, fit + ["SNEQV"])
