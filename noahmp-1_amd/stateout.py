"""State output (nmp_state_output): the groups of soil, snow and canopy fields
an offline run can write beside its fluxes, their LDASOUT variables, and the
kernel's numpy restatement.

The groups (layout.STATE_OUT, NMP_X_* of include/noahmp_engine.h) are selected
by a bit mask; the rows of the selected groups follow each other in group
order.  `state_output_host` restates csrc/stateout.hip operation for operation
in numpy: every operation is one IEEE operation in the header's order, so its
result equals the kernel's bit for bit in fp32 and fp64.
"""
from __future__ import annotations

import numpy as np

from . import layout as L

GROUPS = [n for n, _, _ in L.STATE_OUT]
ALL = (1 << L.NXGROUP) - 1
# the layer dimension of each layered group's LDASOUT variable
LAYER_DIM = {"SOIL_M": "soil_layers_stag", "SOIL_W": "soil_layers_stag",
             "SOIL_T": "soil_layers_stag", "SNOW_T": "snow_layers", "SNOW_Z": "snow_layers"}
LAYER_DIMS = {"soil_layers_stag": L.NSOIL, "snow_layers": L.NSNOW}
_SCALARS = ["SNEQV", "SNOWH", "TG", "TV", "LAI", "SAI", "ZWT", "WA"]


def parse_groups(spec) -> int:
    """The group mask of "all", a comma-separated string of group names or an
    iterable of them (bit g = layout.STATE_OUT[g]).  ValueError for an unknown
    name or an empty selection."""
    if isinstance(spec, str):
        if spec.strip().lower() == "all":
            return ALL
        names = [s.strip() for s in spec.split(",") if s.strip()]
    else:
        names = [str(s) for s in spec]
    if not names:
        raise ValueError("state output: no group selected")
    mask = 0
    for n in names:
        if n not in GROUPS:
            raise ValueError(f"state output: unknown group {n!r} (one of {', '.join(GROUPS)})")
        mask |= 1 << GROUPS.index(n)
    return mask


def check_mask(groups: int) -> int:
    groups = int(groups)
    if groups <= 0 or groups >> L.NXGROUP:
        raise ValueError(f"state output: group mask {groups:#x} is empty or has a bit at or "
                         f"above {L.NXGROUP}")
    return groups


def rows(groups: int) -> list:
    """(variable name, layer index or None) of each row nmp_state_output
    writes for the mask, in row order.  A layered group is one variable with
    layers 0..w-1; CARBON's six rows are six variables."""
    groups = check_mask(groups)
    out = []
    for g, (name, w, _) in enumerate(L.STATE_OUT):
        if not (groups >> g) & 1:
            continue
        if name == "CARBON":
            out += [(p, None) for p in L.CARBON_POOLS]
        elif w == 1:
            out.append((name, None))
        else:
            out += [(name, k) for k in range(w)]
    return out


def nofill_rows(groups: int) -> int:
    """How many of the mask's rows (its leading ones) can never hold the fill value."""
    groups = check_mask(groups)
    return sum(w for g, (_, w, f) in enumerate(L.STATE_OUT) if (groups >> g) & 1 and not f)


def row_names(groups: int) -> list:
    """One flat name per row (the rows of an output block, REGIONS variables):
    a layered group's layer k is NAME_<k+1>."""
    return [n if k is None else f"{n}_{k + 1}" for n, k in rows(groups)]


def variables(names) -> list:
    """(variable, first row, rows, layer dimension or None) of the LDASOUT
    variables a block with the flat row names `names` holds: consecutive
    NAME_1..NAME_w rows of a layered group fold into one variable."""
    out, i, names = [], 0, list(names)
    while i < len(names):
        base = names[i][:-2] if names[i].endswith("_1") else None
        if base in LAYER_DIM:
            w = LAYER_DIMS[LAYER_DIM[base]]
            if names[i:i + w] == [f"{base}_{k + 1}" for k in range(w)]:
                out.append((base, i, w, LAYER_DIM[base]))
                i += w
                continue
        out.append((names[i], i, 1, None))
        i += 1
    return out


def _state_rows(name: str, lo: int = 0, hi: int | None = None) -> set:
    o, w = L.STATE_OFF[name]
    return set(range(o + lo, o + (w if hi is None else hi)))


def algorithmic_bytes(groups: int, itemsize: int) -> int:
    """Bytes per column nmp_state_output has to move for the mask: the distinct
    state rows its groups read, ISNOW and the static integers where a group
    needs them, and the rows written (tools/io_kernels_bench.py)."""
    groups = check_mask(groups)
    sel = lambda *names: any((groups >> GROUPS.index(n)) & 1 for n in names)  # noqa: E731
    rd, ints = set(), 0
    if sel("SOIL_M", "TWS", "SOILSAT", "ROOT_M"):
        rd |= _state_rows("SMC")
    if sel("TWS", "SOILSAT", "ROOT_M"):
        rd |= _state_rows("ZSNSO", 2)
    if sel("SOIL_W"):
        rd |= _state_rows("SH2O")
    if sel("SOIL_T"):
        rd |= _state_rows("STC", 3)
    for n in _SCALARS:
        if sel(n):
            rd |= _state_rows(n)
    if sel("CANWAT", "TWS"):
        rd |= _state_rows("CANLIQ") | _state_rows("CANICE")
    if sel("TWS"):
        rd |= _state_rows("SNEQV") | _state_rows("WA")
    if sel("SNOWLIQ", "SNOWT_AVG"):
        rd |= _state_rows("SNLIQ")
    if sel("SNOWT_AVG"):
        rd |= _state_rows("SNICE")
    if sel("SNOW_T", "SNOWT_AVG"):
        rd |= _state_rows("STC", 0, 3)
    if sel("SNOW_Z"):
        rd |= _state_rows("ZSNSO", 0, 3)
    if sel("CARBON"):
        for p in L.CARBON_POOLS:
            rd |= _state_rows(p)
    if sel("ISNOW", "SNOWLIQ", "TWS", "SOILSAT", "ROOT_M", "SNOW_T", "SNOW_Z", "SNOWT_AVG"):
        ints += 1
    ints += sel("TWS") + sel("SOILSAT") + sel("ROOT_M")   # IST, SOILTYP, VEGTYP
    return (len(rd) + len(rows(groups))) * itemsize + 4 * ints


def _table(params):
    d = params if isinstance(params, dict) else params.as_dict()
    return np.asarray(d["smcmax"], np.float32), np.asarray(d["nroot"], np.int32)


def state_output_host(state, isnow, static_i, params, groups, fill, dtype=None):
    """The rows nmp_state_output writes, (len(rows(groups)), n) of `dtype`
    (default: state's), from state (56, n), isnow (n,), static_i (6, n) and the
    tables `params` (a Params or its as_dict()).  Follows the kernel
    operation for operation; equal to it bit for bit."""
    groups = check_mask(groups)
    T = np.dtype(dtype if dtype is not None else state.dtype).type
    st = np.asarray(state).astype(T, copy=False)
    isn = np.asarray(isnow, np.int32)
    n = isn.shape[0]
    f64 = np.float64
    fillT = T(fill)
    one = lambda name, k=0: st[L.STATE_OFF[name][0] + k]  # noqa: E731
    sel = lambda name: (groups >> GROUPS.index(name)) & 1  # noqa: E731
    smcmax_t, nroot_t = _table(params)
    out = []
    with np.errstate(all="ignore"):
        smc = [one("SMC", i) for i in range(4)]
        dz = L.soil_thickness_host([one("ZSNSO", 2 + i) for i in range(5)], isn)
        active = [k >= isn + 3 for k in range(3)]
        if sel("SOIL_M"):
            out += smc
        if sel("SOIL_W"):
            out += [one("SH2O", i) for i in range(4)]
        if sel("SOIL_T"):
            out += [one("STC", 3 + i) for i in range(4)]
        for name in _SCALARS:
            if sel(name):
                out.append(one(name))
        if sel("CANWAT"):
            out.append(one("CANLIQ") + one("CANICE"))
        if sel("ISNOW"):
            out.append(isn.astype(T))
        if sel("SNOWLIQ"):
            x = np.zeros(n, T)
            for k in range(3):
                x = np.where(active[k], x + one("SNLIQ", k), x)
            out.append(x)
        if sel("TWS"):
            w = L.water_storage_host(one("CANLIQ"), one("CANICE"), one("SNEQV"), one("WA"), smc, dz)
            out.append(np.where(static_i[L.STATIC_I.index("IST")] == 1, w, T(0)))
        if sel("SOILSAT"):
            typ = np.asarray(static_i[L.STATIC_I.index("SOILTYP")], np.int64)
            ok = (typ >= 1) & (typ <= smcmax_t.shape[0])
            smx = smcmax_t[np.where(ok, typ - 1, 0)].astype(f64)
            num, den = np.zeros(n, f64), np.zeros(n, f64)
            for i in range(4):
                num = num + smc[i].astype(f64) * dz[i].astype(f64)
                den = den + smx * dz[i].astype(f64)
            out.append(np.where(ok, (num / den).astype(T), T(np.nan)))
        if sel("ROOT_M"):
            typ = np.asarray(static_i[L.STATIC_I.index("VEGTYP")], np.int64)
            ok = (typ >= 1) & (typ <= nroot_t.shape[0])
            nroot = nroot_t[np.where(ok, typ - 1, 0)]
            num, den = np.zeros(n, f64), np.zeros(n, f64)
            for i in range(4):
                take = i + 1 <= nroot
                num = np.where(take, num + smc[i].astype(f64) * dz[i].astype(f64), num)
                den = np.where(take, den + dz[i].astype(f64), den)
            r = np.where(nroot < 1, T(0), (num / den).astype(T))
            out.append(np.where(ok, r, T(np.nan)))
        if sel("CARBON"):
            out += [one(p) for p in L.CARBON_POOLS]
        if sel("SNOW_T"):
            out += [np.where(active[k], one("STC", k), fillT) for k in range(3)]
        if sel("SNOW_Z"):
            for k in range(3):
                z = one("ZSNSO", k)
                below = one("ZSNSO", max(k - 1, 0)) - z
                out.append(np.where(isn + 3 == k, -z, np.where(active[k], below, fillT)))
        if sel("SNOWT_AVG"):
            num, den = np.zeros(n, f64), np.zeros(n, f64)
            for k in range(3):
                m = (one("SNICE", k) + one("SNLIQ", k)).astype(f64)
                num = np.where(active[k], num + m * one("STC", k).astype(f64), num)
                den = np.where(active[k], den + m, den)
            out.append(np.where((isn == 0) | (den == 0.0), fillT, (num / den).astype(T)))
    res = np.stack([np.asarray(r, T) for r in out])
    assert res.dtype == np.dtype(T) and res.shape == (len(rows(groups)), n)
    return res
