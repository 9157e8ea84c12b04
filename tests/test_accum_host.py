"""Accumulated output, host side (no GPU): the three C-ABI entries are
exported and bound, layout.py's ACC / BUDGET lists equal the header's enums,
the LDASOUT writers carry the 35 fields of an accumulating run (and still
write today's bytes by default), and the netCDF state file round-trips an
interval's accumulation state without changing what read_state returns."""
import datetime
import re
import subprocess

import numpy as np

from noahmp_amd import cases, layout as L, lib as _lib, ncio
from test_abi_host import _enum_values, _header
from test_ncio import bits, grid_for

T0 = datetime.datetime(2000, 1, 1)
ENTRIES = ("nmp_accumulate", "nmp_water_storage", "nmp_accum_finish")


def test_accum_entries_exported(engine_lib):
    decl = set(re.findall(r"^\s*(?:int|int64_t|void\*?|const char\*)\s*(nmp_\w+)\s*\(", _header(),
                          re.M))
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.library_path()], capture_output=True,
                        text=True, check=True).stdout
    exported = set(re.findall(r"\bT (nmp_\w+)$", nm, re.M))
    for name in ENTRIES:
        assert name in decl, f"{name} not declared in the header"
        assert name in _lib.EXPORTED_SYMBOLS and name in exported, name
        assert getattr(engine_lib, name).argtypes is not None, f"{name} not bound in lib.py"


def test_accum_layout_matches_header():
    e = _enum_values(_header())
    assert e["NMP_NACC"] == L.NACC == 17 and e["NMP_NBUDGET"] == L.NBUDGET == 19
    for i, n in enumerate(L.ACC):
        assert e[f"NMP_ACC_{n}"] == i, n
    # rows 0..15 mirror the output fluxes, the precipitation follows
    assert L.ACC[:L.NDIAG_OUT] == L.DIAG_OUT and L.ACC[16] == "PRCP"
    for i, n in enumerate(L.BUDGET):
        assert e[f"NMP_B_{n}"] == i, n
    assert L.BUDGET == [
        "FSA_MEAN", "FSR_MEAN", "FIRA_MEAN", "FSH_MEAN", "SSOIL_MEAN", "FCEV_MEAN", "FGEV_MEAN",
        "FCTR_MEAN", "TRAD_MEAN", "T2M_MEAN", "ALBEDO_MEAN", "ACCPRCP", "ACCECAN", "ACCETRAN",
        "ACCEDIR", "SFCRNOFF", "UGDRNOFF", "DSTOR", "WBRES"]
    assert L.DIAG_OUT_ACC == L.DIAG_OUT + L.BUDGET and len(set(L.DIAG_OUT_ACC)) == 35
    assert re.search(r"#define NMP_ABI_VERSION 8\b", _header())  # additive: the version stays


def test_ldasout_writers_carry_35_fields(tmp_path, ref_params):
    """write_ldasout_grids with the 35 names writes write_ldasout's bytes, and
    the netCDF reader returns every variable under its name."""
    from scipy.io import netcdf_file
    cols = cases.make_columns(32, "mixed", ref_params, seed=8)
    grid = grid_for(cols)
    names = L.DIAG_OUT_ACC
    for dt in (np.float32, np.float64):
        diag = np.random.default_rng(3).normal(size=(len(names), 32)).astype(dt)
        full = np.stack([grid.scatter(diag[i], np.asarray(ncio.FILL, dt)).reshape(-1)
                         for i in range(len(names))]).astype(np.dtype(dt).newbyteorder(">"))
        t = T0 + datetime.timedelta(hours=3)
        a, b = str(tmp_path / "a.nc"), str(tmp_path / "b.nc")
        ncio.write_ldasout(a, grid, diag, t, names=names)
        ncio.write_ldasout_grids(b, grid, full, t, names=names)
        assert open(a, "rb").read() == open(b, "rb").read()
        f = netcdf_file(b, "r", mmap=False)
        try:
            assert list(f.variables) == list(names)
            for i, name in enumerate(names):
                v = np.array(f.variables[name][0])
                assert np.array_equal(bits(grid.columns(v).astype(dt)), bits(diag[i])), name
                assert (v[~grid.mask] == ncio.FILL).all()
        finally:
            f.close()
        assert np.array_equal(bits(ncio.read_ldasout(b, grid, names)), bits(diag))
        # the 16 fluxes alone, read by the default names
        assert np.array_equal(bits(ncio.read_ldasout(b, grid)), bits(diag[:L.NDIAG_OUT]))


def test_ldasout_writers_default_bytes_unchanged(tmp_path, ref_params):
    """names defaults to the 16 output fluxes: both writers produce the file
    they produced before the argument existed (explicit default == implicit,
    and the header's variable list is exactly layout.DIAG_OUT)."""
    cols = cases.make_columns(32, "mixed", ref_params, seed=8)
    grid = grid_for(cols)
    diag = np.random.default_rng(2).normal(size=(L.NDIAG_OUT, 32)).astype(np.float32)
    full = np.stack([grid.scatter(diag[i]).reshape(-1) for i in range(L.NDIAG_OUT)]).astype(">f4")
    a, b, c = (str(tmp_path / f"{k}.nc") for k in "abc")
    ncio.write_ldasout(a, grid, diag, T0)
    ncio.write_ldasout_grids(b, grid, full, T0)
    ncio.write_ldasout_grids(c, grid, full, T0, names=L.DIAG_OUT)
    raw = open(a, "rb").read()
    assert raw == open(b, "rb").read() == open(c, "rb").read()
    hdr = ncio.ldasout_header(grid, "f4", T0)
    assert raw.startswith(hdr) and len(raw) == len(hdr) + full.nbytes
    assert hdr.count(b"_FillValue") == 16 and b"_MEAN" not in hdr and b"WBRES" not in hdr
    pos = [hdr.index(ncio._nc_name(n)) for n in L.DIAG_OUT]
    assert pos == sorted(pos)


def test_state_file_round_trips_accumulation(tmp_path, ref_params):
    cols = cases.make_columns(32, "mixed", ref_params, seed=5)
    grid = grid_for(cols)
    t = datetime.datetime(2000, 3, 1, 6)
    rng = np.random.default_rng(7)
    acc = rng.normal(size=(L.NACC, 32)) * 1e5
    stor = (5800.0 + rng.normal(size=32)).astype(np.float32)
    plain, withacc = str(tmp_path / "plain.nc"), str(tmp_path / "acc.nc")
    ncio.write_state(plain, grid, cols.state, cols.isnow, t, step=17)
    ncio.write_state(withacc, grid, cols.state, cols.isnow, t, step=17, accum=(acc, stor, 4))
    got = ncio.read_accum(withacc, grid)
    assert got is not None and got[2] == 4
    assert got[0].dtype == np.float64 and np.array_equal(bits(got[0]), bits(acc))
    assert np.array_equal(bits(got[1].astype(np.float32)), bits(stor))
    assert ncio.read_accum(plain, grid) is None
    # read_state returns what it returns from a file without the block
    for a, b in zip(ncio.read_state(withacc, grid), ncio.read_state(plain, grid)):
        if isinstance(a, np.ndarray):
            assert a.dtype == b.dtype and np.array_equal(bits(a) if a.dtype.kind == "f" else a,
                                                         bits(b) if b.dtype.kind == "f" else b)
        else:
            assert a == b
    assert np.array_equal(bits(ncio.read_state(withacc, grid)[0]), bits(cols.state))
