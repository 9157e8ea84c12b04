"""ORACLE TEST INFRASTRUCTURE -- NOT PART OF THE PRODUCT.

ctypes driver for the plain-C restatement (oracle/noahmp_oracle.c), built as
build/liboracle_f32.so and build/liboracle_f64.so by oracle/Makefile.
Same SoA interface as oracle/ref.py.

step_ensemble / run_ensemble drive the perturbed fp64 build
(build/liboracle_f64_perturb.so, noahmp_oracle.c ORACLE_PERTURB): the base and
members whose libm results, powers and Newton-loop divisions are moved within
bounds the caller passes.  The fp64 engine's GPU tests take their per-column
tolerance from it (tests/golden_io.py check_fp64_rule).
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from ref import PARAM_FLOAT_FIELDS, PARAM_INT_FIELDS, PARAM_SHAPES, NPARAM_F, NPARAM_I

HERE = os.path.dirname(os.path.abspath(__file__))
LIBS = {4: os.path.join(HERE, "build", "liboracle_f32.so"),
        8: os.path.join(HERE, "build", "liboracle_f64.so"),
        "cr": os.path.join(HERE, "build", "liboracle_f32cr.so"),
        "4s": os.path.join(HERE, "build", "liboracle_f32_stats.so"),
        "8s": os.path.join(HERE, "build", "liboracle_f64_stats.so"),
        "4d": os.path.join(HERE, "build", "liboracle_f32_divstats.so"),
        "4b": os.path.join(HERE, "build", "liboracle_f32_brstats.so"),
        "8b": os.path.join(HERE, "build", "liboracle_f64_brstats.so"),
        "8p": os.path.join(HERE, "build", "liboracle_f64_perturb.so")}
_F64 = (8, "8s", "8b", "8p")
# the perturbed fp64 build's site kinds, in the order of noahmp_oracle.c's PB_
# enum ("pow" and "tdf" are formed per call from "log" and "exp"): the keys of
# the bounds dict step_ensemble takes, in ulps
PERTURB_SITES = ("exp", "exp2", "log", "log10", "tanh", "atan", "tan", "acos", "cos",
                 "pow", "pow_q", "pow_mq", "div", "tdf", "pow_d")
# ensemble members as (mode, seed): the four fixed sign patterns and 24 seeds
FIXED_MEMBERS = ((1, 0), (2, 0), (3, 0), (4, 0))
ENSEMBLE = FIXED_MEMBERS + tuple((5, s) for s in range(1, 25))
# trip counts recorded by the stats builds, per column (noahmp_oracle.c ITER_STAT)
STAT_LOOPS = ("vege_flux Newton", "stomata bisection", "frh2o", "soilwater sub-steps",
              "bare_flux Newton")
# bit k of the branch-marker builds' per-column mask (noahmp_oracle.c BR(k)): the
# physics branches that columns from cases.make_columns / forcing_random never
# take, pinned by tests/golden/branch_*.npz
BRANCH_SITES = (
    "snowage_sneqv_over_800", "groundalb_soilcolor_9", "sfcdif2_wstar2_zero_first", "stomata_c4",
    "stomata_root_b_nonnegative", "vege_flux_cah2_small", "bare_flux_ehb2_small",
    "frh2o_flerchinger", "phasechange_imelt_reset", "phasechange_below_supercool",
    "combine_negative_snice", "combine_negative_soilice", "combine_middle_layer",
    "combine_middle_layer_upper_neighbour", "snowh2o_nosnow_negative_soilice",
    "snowh2o_thin_negative_soilice", "snowh2o_combine", "snowh2o_epore_small",
    "snowwater_glacier_cap", "groundwater_table_above_layer3", "co2flux_rtmass_negative",
    "sflx_unknown_opt_veg", "combine_negative_ponding", "sfcdif2_wstar2_zero_loop")
NST, NSF, NSI, NFC, NDG = 56, 6, 6, 12, 58
_libs = {}


def available(precision: int = 4) -> bool:
    return os.path.exists(LIBS[precision])


def pack_params(P: dict) -> bytes:
    """dict (ref.dump_params() layout) -> bytes of `struct nmp_params`."""
    fl = []
    for name, w in PARAM_FLOAT_FIELDS:
        a = np.asarray(P[name], np.float32).reshape(-1)
        assert a.size == w, (name, a.size, w)
        fl.append(a)
    il = []
    for name, w in PARAM_INT_FIELDS:
        a = np.asarray(P[name], np.int32).reshape(-1)
        assert a.size == w, (name, a.size, w)
        il.append(a)
    return np.concatenate(fl).tobytes() + np.concatenate(il).tobytes()


def _lib(precision):
    if precision not in _libs:
        if not available(precision):
            raise FileNotFoundError(f"{LIBS[precision]} missing (run make -C oracle port)")
        lib = C.CDLL(LIBS[precision])
        rt = np.float64 if precision in _F64 else np.float32
        rp = np.ctypeslib.ndpointer(rt, flags="C_CONTIGUOUS")
        ip = np.ctypeslib.ndpointer(np.int32, flags="C_CONTIGUOUS")
        creal = C.c_double if precision in _F64 else C.c_float
        lib.oracle_sflx_batch.argtypes = [C.c_int32, creal, C.c_int32, creal, rp, rp, ip, rp, ip,
                                          rp, rp, ip, C.c_char_p, C.c_void_p]
        lib.oracle_sflx_run.argtypes = [C.c_int32, C.c_int32, creal, C.c_int32, creal, rp, rp, ip,
                                        rp, ip, rp, C.c_int32, rp, ip, C.c_char_p, C.c_void_p]
        assert lib.oracle_real_bytes() == (8 if precision in _F64 else 4)
        if precision in ("4s", "8s", "8p"):
            lib.oracle_set_stats.argtypes = [C.c_void_p]
        if precision == "8p":
            lib.oracle_set_perturb.argtypes = [C.c_uint64, C.c_int, C.c_double]
            lib.oracle_set_perturb_bounds.argtypes = [
                np.ctypeslib.ndpointer(np.float64, flags="C_CONTIGUOUS"), C.c_int]
        lib.oracle_set_t2m.argtypes = [C.c_void_p]
        if precision == "4d":
            lib.oracle_div_stats.argtypes = [C.c_void_p, C.c_int]
        if precision in ("4b", "8b"):
            lib.oracle_set_branches.argtypes = [C.c_void_p]
        _libs[precision] = (lib, rt)
    return _libs[precision]


def step(P: dict, options, zsoil, dt, yearlen, julian, state, isnow, static_f, static_i, forcing,
         precision=4):
    """One step of the C restatement.  SoA in, SoA out: (state', isnow', diag(58,n), status).

    precision: 4 (bit-exact to the reference), 8 (fp64), or "cr" (fp32 with
    correctly rounded libm -- what the engine's default math computes)."""
    lib, rt = _lib(precision)
    n = isnow.shape[0]
    st = np.array(np.asarray(state, rt).T, order="C")  # a copy: written in place
    isn = np.ascontiguousarray(isnow, np.int32).copy()
    sf = np.ascontiguousarray(np.asarray(static_f, rt).T)
    si = np.ascontiguousarray(np.asarray(static_i, np.int32).T)
    fc = np.ascontiguousarray(np.asarray(forcing, rt).T)
    dg = np.zeros((n, NDG), rt)
    status = np.zeros(n, np.int32)
    opts = (C.c_int32 * 12)(*[int(x) for x in options])
    lib.oracle_sflx_batch(n, dt, int(yearlen), julian, np.ascontiguousarray(zsoil, rt), st, isn, sf,
                          si, fc, dg, status, pack_params(P), C.addressof(opts))
    return st.T.copy(), isn, dg.T.copy(), status


def step_t2m(P: dict, options, zsoil, dt, yearlen, julian, state, isnow, static_f, static_i,
             forcing, precision=4):
    """step() plus the composite 2-m temperature T2M (func.f90:1256/1270), which
    is not one of the 58 outputs, as an (n,) array (oracle_set_t2m)."""
    lib, rt = _lib(precision)
    t2m = np.zeros(isnow.shape[0], rt)
    lib.oracle_set_t2m(t2m.ctypes.data)
    try:
        out = step(P, options, zsoil, dt, yearlen, julian, state, isnow, static_f, static_i,
                   forcing, precision=precision)
    finally:
        lib.oracle_set_t2m(None)
    return (*out, t2m)


def step_stats(P: dict, options, zsoil, dt, yearlen, julian, state, isnow, static_f, static_i,
               forcing, precision=4):
    """step() through the trip-count build of `precision` (4 or 8): returns
    step()'s tuple plus an (n, 5) int32 array of loop trip counts (STAT_LOOPS)."""
    key = {4: "4s", 8: "8s"}[precision]
    lib, _ = _lib(key)
    n = isnow.shape[0]
    buf = np.zeros((n, 8), np.int32)
    lib.oracle_set_stats(buf.ctypes.data)
    try:
        out = step(P, options, zsoil, dt, yearlen, julian, state, isnow, static_f, static_i,
                   forcing, precision=key)
    finally:
        lib.oracle_set_stats(None)
    return (*out, buf[:, :len(STAT_LOOPS)].copy())


def _member_step(bounds, mode, seed, amplitude, args):
    """One step of the perturbed fp64 build as member (mode, seed): step()'s
    tuple, the (n, 5) trip counts and T2M."""
    lib, _ = _lib("8p")
    b = np.array([float(bounds.get(k, 0.0)) for k in PERTURB_SITES], np.float64)
    lib.oracle_set_perturb_bounds(b, b.size)
    n = args[7].shape[0]
    buf = np.zeros((n, 8), np.int32)
    t2m = np.zeros(n, np.float64)
    lib.oracle_set_perturb(int(seed), int(mode), float(amplitude))
    lib.oracle_set_stats(buf.ctypes.data)
    lib.oracle_set_t2m(t2m.ctypes.data)
    try:
        out = step(*args, precision="8p")
    finally:
        lib.oracle_set_stats(None)
        lib.oracle_set_t2m(None)
        lib.oracle_set_perturb(0, 0, 1.0)
    return (*out, buf[:, :len(STAT_LOOPS)].copy(), t2m)


def _deviation(member, base):
    """Per column, the largest |member - base| / (1e-9 (1 + |base|)) over the
    fields of an (nfield, n) array; fields equal in bits (NaN == NaN, inf ==
    inf) count 0, a finite value against a non-finite one inf."""
    member, base = np.asarray(member, np.float64), np.asarray(base, np.float64)
    same = (member == base) | (np.isnan(member) & np.isnan(base))
    with np.errstate(invalid="ignore", over="ignore"):
        q = np.abs(member - base) / (1e-9 * (1.0 + np.abs(base)))
    q = np.where(same, 0.0, np.where(np.isnan(q), np.inf, q))
    return q.max(axis=0) if q.ndim > 1 else q


def step_ensemble(P: dict, options, zsoil, dt, yearlen, julian, state, isnow, static_f, static_i,
                  forcing, bounds, members=ENSEMBLE, amplitude=1.0):
    """The fp64 restatement (mode 0 of the perturbed build) and an ensemble of
    its perturbed members over one step.

    bounds: {site kind: ulps} for PERTURB_SITES (missing kinds: 0).  Returns
    (base, discrete, q): base = (state', isnow', diag(58, n), status, trips(n, 5),
    T2M(n)); discrete(n,) = a member changed ISNOW, status or a trip count;
    q(n,) = the largest member deviation over the state, the 58 outputs and
    T2M, in units of 1e-9 (1 + |base|)."""
    return run_ensemble(P, options, zsoil, dt, yearlen, [julian], state, isnow, static_f,
                        static_i, [forcing], bounds, members, amplitude)


def run_ensemble(P: dict, options, zsoil, dt, yearlen, julians, state, isnow, static_f, static_i,
                 forcings, bounds, members=ENSEMBLE, amplitude=1.0):
    """step_ensemble over repeated steps (julians[k], forcings[k]): each member
    is perturbed in every step; the trip counts of all steps are compared, the
    values after the last; status is the OR over the steps.  The base carries the
    last step's outputs."""
    def go(mode, seed):
        st, isn, trips, status = state, isnow, [], 0
        for k, (jul, f) in enumerate(zip(julians, forcings)):
            st, isn, dg, stat_k, it, t2m = _member_step(
                bounds, mode, 1000003 * k + seed, amplitude,
                (P, options, zsoil, dt, yearlen, jul, st, isn, static_f, static_i, f))
            trips.append(it)
            status = status | stat_k   # sticky over the steps, like the engine's status word
        return st, isn, dg, status, np.concatenate(trips, axis=1), t2m
    base = go(0, 0)
    n = base[1].shape[0]
    discrete = np.zeros(n, bool)
    q = np.zeros(n)
    for mode, seed in members:
        m = go(mode, seed)
        discrete |= (m[1] != base[1]) | (m[3] != base[3]) | (m[4] != base[4]).any(axis=1)
        q = np.maximum(q, np.maximum(np.maximum(_deviation(m[0], base[0]),
                                                _deviation(m[2], base[2])),
                                     _deviation(m[5], base[5])))
    return base, discrete, q


def step_branches(P: dict, options, zsoil, dt, yearlen, julian, state, isnow, static_f, static_i,
                  forcing, precision=4):
    """step() through the branch-marker build of `precision` (4 or 8): returns
    step()'s tuple plus an (n,) uint32 mask, bit k set where the column
    executed the branch BRANCH_SITES[k]."""
    key = {4: "4b", 8: "8b"}[precision]
    lib, _ = _lib(key)
    mask = np.zeros(isnow.shape[0], np.uint32)
    lib.oracle_set_branches(mask.ctypes.data)
    try:
        out = step(P, options, zsoil, dt, yearlen, julian, state, isnow, static_f, static_i,
                   forcing, precision=key)
    finally:
        lib.oracle_set_branches(None)
    return (*out, mask)


def branch_hits(mask) -> dict:
    """{site name: number of columns} of a step_branches mask."""
    mask = np.asarray(mask, np.uint32)
    return {name: int(((mask >> np.uint32(k)) & 1).sum()) for k, name in enumerate(BRANCH_SITES)}


def div_stats(reset: bool = False) -> np.ndarray:
    """Division operand ranges recorded by the "4d" build since the last reset
    (noahmp_oracle.c ORACLE_DIV_STATS): (40 sites, 8) = min|a|, max|a|, min|b|,
    max|b|, min|q|, max|q| over nonzero finite values, calls, zero numerators."""
    lib, _ = _lib("4d")
    out = np.zeros((40, 8), np.float64)
    lib.oracle_div_stats(out.ctypes.data, int(reset))
    return out


def prepare_run(P: dict, options, zsoil, dt, yearlen, julian0, state, isnow, static_f, static_i,
                forcings, nsteps: int, precision: int = 4):
    """run() split in two: the host transposes happen here, the returned
    callable is only the library's time loop (the CPU baseline times that) and
    returns (state', isnow', diag, status) of the last step."""
    lib, rt = _lib(precision)
    n = isnow.shape[0]
    st = np.array(np.asarray(state, rt).T, order="C")  # a copy: written in place
    isn = np.ascontiguousarray(isnow, np.int32).copy()
    sf = np.ascontiguousarray(np.asarray(static_f, rt).T)
    si = np.ascontiguousarray(np.asarray(static_i, np.int32).T)
    fc = np.ascontiguousarray(np.asarray(forcings, rt).transpose(0, 2, 1))
    dg = np.zeros((n, NDG), rt)
    status = np.zeros(n, np.int32)
    opts = (C.c_int32 * 12)(*[int(x) for x in options])
    zs = np.ascontiguousarray(zsoil, rt)
    packed = pack_params(P)

    def go():
        lib.oracle_sflx_run(n, nsteps, dt, int(yearlen), julian0, zs, st, isn, sf, si, fc,
                            fc.shape[0], dg, status, packed, C.addressof(opts))
        return st.T.copy(), isn, dg.T.copy(), status
    return go


def run(P: dict, options, zsoil, dt, yearlen, julian0, state, isnow, static_f, static_i,
        forcings, nsteps: int, precision: int = 4):
    """nsteps steps over a forcing cycle forcings[(period, 12, n)]."""
    return prepare_run(P, options, zsoil, dt, yearlen, julian0, state, isnow, static_f, static_i,
                       forcings, nsteps, precision)()


# ---- single routines (the code sflx_column calls), fp32 bit-exact build ----
def _rt(name, *argtypes, precision: int = 4):
    lib, _ = _lib(precision)
    f = getattr(lib, name)
    f.argtypes = list(argtypes)
    f.restype = None
    return f


def esat(t):
    f32p = np.ctypeslib.ndpointer(np.float32, flags="C_CONTIGUOUS")
    t = np.ascontiguousarray(t, np.float32)
    out = np.zeros((t.size, 4), np.float32)
    _rt("oracle_esat", C.c_int32, f32p, f32p)(t.size, t, out)
    return out


def tdfcnd(P: dict, sltyp, smc, sh2o):
    f32p = np.ctypeslib.ndpointer(np.float32, flags="C_CONTIGUOUS")
    i32p = np.ctypeslib.ndpointer(np.int32, flags="C_CONTIGUOUS")
    n = len(smc)
    out = np.zeros(n, np.float32)
    _rt("oracle_tdfcnd", C.c_char_p, C.c_int32, i32p, f32p, f32p, f32p)(
        pack_params(P), n, np.ascontiguousarray(sltyp, np.int32),
        np.ascontiguousarray(smc, np.float32), np.ascontiguousarray(sh2o, np.float32), out)
    return out


def frh2o(P: dict, sltyp, tk, smc, sh2o, precision: int = 4):
    rt = np.float32 if precision == 4 else np.float64
    rp = np.ctypeslib.ndpointer(rt, flags="C_CONTIGUOUS")
    i32p = np.ctypeslib.ndpointer(np.int32, flags="C_CONTIGUOUS")
    n = len(tk)
    out = np.zeros(n, rt)
    st = np.zeros(n, np.int32)
    _rt("oracle_frh2o", C.c_char_p, C.c_int32, i32p, rp, rp, rp, rp, i32p, precision=precision)(
        pack_params(P), n, np.ascontiguousarray(sltyp, np.int32), np.ascontiguousarray(tk, rt),
        np.ascontiguousarray(smc, rt), np.ascontiguousarray(sh2o, rt), out, st)
    return out, st


def calhum(sfctmp, sfcprs, precision: int = 4):
    """calhum (func.f90:3958-3984) over arrays: (Q2SAT, DQSDT2)."""
    rt = np.float32 if precision == 4 else np.float64
    rp = np.ctypeslib.ndpointer(rt, flags="C_CONTIGUOUS")
    n = len(sfctmp)
    q, d = np.zeros(n, rt), np.zeros(n, rt)
    _rt("oracle_calhum", C.c_int32, rp, rp, rp, rp, precision=precision)(
        n, np.ascontiguousarray(sfctmp, rt), np.ascontiguousarray(sfcprs, rt), q, d)
    return q, d


def rosr12(kt, a, b, c, d):
    """(n, 7) systems solved on layers kt..6: returns (p, c', delta)."""
    f32p = np.ctypeslib.ndpointer(np.float32, flags="C_CONTIGUOUS")
    i32p = np.ctypeslib.ndpointer(np.int32, flags="C_CONTIGUOUS")
    n = len(kt)
    c = np.array(c, np.float32, order="C")
    p = np.zeros((n, 7), np.float32)
    dl = np.zeros((n, 7), np.float32)
    _rt("oracle_rosr12", C.c_int32, i32p, f32p, f32p, f32p, f32p, f32p, f32p)(
        n, np.ascontiguousarray(kt, np.int32), np.ascontiguousarray(a, np.float32),
        np.ascontiguousarray(b, np.float32), c, np.ascontiguousarray(d, np.float32), p, dl)
    return p, c, dl
