/*
 * noahmp_engine.h -- C ABI of the MI355X Noah-MP column engine.
 *
 * Drop-in for the reference engine slot `module noahmp_engine`
 * (/root/reference/core/module_noahmp_engine.f90:5-10: empty `noahmp_init`,
 * `noahmp_run`) and for the per-column physics entry it was meant to drive,
 * `noahmp_sflx` (core/module_noahmp_func.f90:66-91, 131 by-reference args).
 *
 * Entry point                 replaces (reference file:line)
 * --------------------------  ------------------------------------------------
 * nmp_read_tables             noahmp_gen_param_readptable   core/module_noahmp_gen_param.f90:51-89
 *                             noahmp_soil_param_readptable  core/module_noahmp_soil_param.f90:31-72
 *                             noahmp_veg_param_readptable   core/module_noahmp_veg_param.f90:77-161
 *                             (block/tag finder             core/module_noahmp_utils.f90:200-237)
 * nmp_init                    noahmp_init                   core/module_noahmp_engine.f90:5-6
 *                             noahmp_set_options            core/module_noahmp_global.f90:77-112
 * nmp_step                    noahmp_run                    core/module_noahmp_engine.f90:8-10
 *                             = noahmp_sflx over every column core/module_noahmp_func.f90:66-476
 * nmp_run, nmp_run_out        the offline time loop around noahmp_run (run/main.py:12-14
 *                             stops after the namelist): many steps, one launch
 * nmp_sflx_columns,           noahmp_sflx itself, argument for argument, on n host records
 *   nmp_sflx_column                                         core/module_noahmp_func.f90:66-476
 * nmp_forcing_from_ldasin,    the forcing arguments of noahmp_sflx (:72-74) from the LDASIN
 *   nmp_forcing_from_ldasin_geo, variables the namelist's input files carry (run/case.nml:6-7)
 *   nmp_ldasin_ingest,
 *   nmp_ldasout_grid         (and the LDASOUT file's grids from the step's diagnostics)
 * nmp_accumulate,             interval totals / means of the output fluxes and the water
 *   nmp_water_storage,        budget's closure: BEG_WB / END_WB / ERRWAT, which the reference
 *   nmp_accum_finish          forms and drops             core/module_noahmp_func.f90:339-344, 723-731
 * nmp_region_reduce           no counterpart: weighted sums / means of an output block's fields
 *                             over the columns of each region (basin means), on the device
 * nmp_ldasin_regrid,          no counterpart: an LDASIN file on its own (coarse) grid onto the
 *   nmp_ldasin_downscale      columns, and its elevation (lapse-rate) correction, on the device
 * nmp_ldasin_cosz,            no counterpart: the forcing of a step between two input times
 *   nmp_forcing_from_ldasin_interp  from the two resident blocks at the interval's ends
 * nmp_state_output            no counterpart: the soil, snow and canopy state of an output step as
 *                             output rows (the NMP_X_* groups), formed on the device
 * nmp_state_drift,            no counterpart: a spin-up's convergence test -- the state's drift
 *   nmp_drift_reduce          between two passes over the forcing period (the NMP_G_* groups)
 *                             and its max / argmax / count / weighted sum, on the device
 * nmp_static_monthly          no counterpart: the vegetation fraction SHDFAC of a date from the
 *                             12-month GREENFRAC climatology (fveg = SHDFAC with opt_veg = 1,
 *                             core/module_noahmp_func.f90:366-368), on the device
 * nmp_extremes_update,        no counterpart: an output interval's running maximum and minimum
 *   nmp_extremes_output       of per-column series (fluxes, forcing, state rows) and the time
 *                             each occurred, on the device
 * nmp_frh2o, nmp_frh2o_host   frh2o (public routine)       core/module_noahmp_func.f90:4494-4598
 * nmp_calhum, nmp_calhum_host calhum (public by default)     core/module_noahmp_func.f90:3958-3984
 * nmp_state_from_aos          layout bridge from noahmp_state_t records
 *                                                           core/module_noahmp_type.f90:10-42
 * nmp_finalize, nmp_strerror  (error path of utils `assert`/`stop`, core/module_noahmp_utils.f90:21-53)
 * nmp_set_launch_variant, nmp_type_size, nmp_option_set, nmp_set_math,
 *   nmp_set_cols_per_wave     engine tuning / host layout checks (no reference counterpart)
 *
 * Conventions
 *  - Plain pointers and sizes only.  All per-column arrays are structure of
 *    arrays, field-major: field f of column c lives at base[f*ld + c]
 *    (ld >= ncol), so one wavefront of 64 lanes reads 64 consecutive columns
 *    of one field per load.  ld < 2^29 (536,870,912 columns per call;
 *    NMP_E_ARG otherwise): the kernel forms a column's byte offset in 32 bits.
 *  - "real" arrays are float when the engine was created with precision 4 and
 *    double with precision 8.  Table values (nmp_params) are always float, as
 *    in the reference (real(r4) module arrays).
 *  - Pointers passed to nmp_step are DEVICE pointers on the engine's device;
 *    `stream` is a hipStream_t (NULL = default stream).  nmp_step only
 *    enqueues work; it never synchronises and never allocates.
 *  - Return codes: 0 ok, negative = NMP_E_*.  Per-column physics failures
 *    that abort the reference (wrf_error_fatal) are reported as NMP_ST_* bits
 *    in col_status instead; the column continues, as the reference code does
 *    after the external returns.
 *  - Threading: one engine per device; calls on one engine are serialised by
 *    the caller.  Engines on different devices/ranks are independent.  The
 *    synchronous host entries (nmp_sflx_columns, nmp_frh2o_host,
 *    nmp_calhum_host) share one device scratch block and stream per engine
 *    and take an engine lock, so concurrent calls of them are safe (they run
 *    one after another).
 */
#ifndef NOAHMP_ENGINE_H
#define NOAHMP_ENGINE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NMP_ABI_VERSION 8

/* ---- dimensions (core/module_noahmp_global.f90:9-13) -------------------- */
#define NMP_NSOIL 4
#define NMP_NSNOW 3
#define NMP_NLAYER 7 /* -NSNOW+1 .. NSOIL ; C index k <-> Fortran index k-2 */
#define NMP_NBAND 2

/* ---- physics options, order = noahmp_set_options (global.f90:77-80) ----- */
typedef struct nmp_options {
  int32_t opt_veg, opt_crs, opt_btr, opt_run, opt_sfc, opt_frz;
  int32_t opt_inf, opt_rad, opt_alb, opt_snf, opt_tbot, opt_stc;
} nmp_options;

/* ---- lookup tables: the reference module arrays, in memory ------------- *
 * Field order == the reference module declarations; 2-D Fortran arrays
 * (band,type) / (month,type) map to C [type][band] / [type][month].
 * Indices are 1-based in the reference: entry i of the C arrays is type i+1. */
#define NMP_MSLOPETYP 30 /* gen_param.f90:8   */
#define NMP_MSLTYP 30    /* soil_param.f90:7  */
#define NMP_MSLCOL 20    /* soil_param.f90:8  */
#define NMP_MLUTYP 27    /* veg_param.f90:8   */

typedef struct nmp_params {
  /* GENPARMMP.TBL  (gen_param.f90:12-48) */
  float slope[NMP_MSLOPETYP];
  float csoil, zbot, czil, dkref, kdtref, frzk, timean, fsatmax;
  float mltfct, z0sno, ssi, swemax;
  float albice[2], alblake[2], omegas[2];
  float betads, betais, emssoil, emslake;
  /* SOILPARMMP.TBL  (soil_param.f90:13-28) */
  float bexp[NMP_MSLTYP], smcmax[NMP_MSLTYP], smcref[NMP_MSLTYP], smcwlt[NMP_MSLTYP];
  float psisat[NMP_MSLTYP], dksat[NMP_MSLTYP], dwsat[NMP_MSLTYP], quartz[NMP_MSLTYP];
  float kdt[NMP_MSLTYP], frzx[NMP_MSLTYP];
  float albsat[NMP_MSLCOL][2], albdry[NMP_MSLCOL][2];
  /* VEGPARMMP.TBL  (veg_param.f90:19-74) */
  float xl[NMP_MLUTYP];
  float rhol[NMP_MLUTYP][2], rhos[NMP_MLUTYP][2], taul[NMP_MLUTYP][2], taus[NMP_MLUTYP][2];
  float canwmxp[NMP_MLUTYP], dleaf[NMP_MLUTYP], z0mvt[NMP_MLUTYP], hvt[NMP_MLUTYP];
  float hvb[NMP_MLUTYP], den[NMP_MLUTYP], rcrown[NMP_MLUTYP], cwpvt[NMP_MLUTYP];
  float sai12m[NMP_MLUTYP][12], lai12m[NMP_MLUTYP][12];
  float sla[NMP_MLUTYP], dilefc[NMP_MLUTYP], dilefw[NMP_MLUTYP], fragr[NMP_MLUTYP];
  float ltovrc[NMP_MLUTYP], wrrat[NMP_MLUTYP], wdpool[NMP_MLUTYP], tdlef[NMP_MLUTYP];
  float rgl[NMP_MLUTYP], hs[NMP_MLUTYP], rsmax[NMP_MLUTYP], rsmin[NMP_MLUTYP], topt[NMP_MLUTYP];
  float kc25[NMP_MLUTYP], akc[NMP_MLUTYP], ko25[NMP_MLUTYP], ako[NMP_MLUTYP];
  float vcmx25[NMP_MLUTYP], avcmx[NMP_MLUTYP], bp[NMP_MLUTYP], mp[NMP_MLUTYP];
  float qe25[NMP_MLUTYP], aqe[NMP_MLUTYP], folnmx[NMP_MLUTYP], tmin[NMP_MLUTYP];
  float rmf25[NMP_MLUTYP], rms25[NMP_MLUTYP], rmr25[NMP_MLUTYP], arm[NMP_MLUTYP], mrp[NMP_MLUTYP];
  float slarea[NMP_MLUTYP], eps[NMP_MLUTYP][5];
  /* integers */
  int32_t nslptyp, nsltyp, nsoilcol, nlutyp;
  int32_t isurban, iswater, isbarren, isice, isegblf; /* veg_param.f90:13-17 */
  int32_t nroot[NMP_MLUTYP], c3c4[NMP_MLUTYP];
} nmp_params;

/* ---- per-column SoA layouts ---------------------------------------------
 * Prognostic fp state (read + written every step).  The first block keeps
 * the snow/soil arrays; index k of a 7-layer field is Fortran layer k-2. */
enum {
  NMP_S_STC = 0,     /* [7] snow/soil temperature (K)              */
  NMP_S_ZSNSO = 7,   /* [7] layer-bottom depth from snow surface (m, <0) */
  NMP_S_SNICE = 14,  /* [3] snow layer ice (mm)                    */
  NMP_S_SNLIQ = 17,  /* [3] snow layer liquid (mm)                 */
  NMP_S_SH2O = 20,   /* [4] soil liquid water (m3/m3) ("soilwat")  */
  NMP_S_SMC = 24,    /* [4] soil total water (m3/m3)               */
  NMP_S_TV = 28, NMP_S_TG, NMP_S_TAH, NMP_S_EAH, NMP_S_FWET, NMP_S_CANLIQ,
  NMP_S_CANICE, NMP_S_QSFC, NMP_S_SNOWH, NMP_S_SNEQV, NMP_S_SNEQVO, NMP_S_ALBOLD,
  NMP_S_TAUSS, NMP_S_QSNOW, NMP_S_ZWT, NMP_S_WA, NMP_S_WT, NMP_S_WSLAKE,
  NMP_S_LAI, NMP_S_SAI, NMP_S_LFMASS, NMP_S_RTMASS, NMP_S_STMASS, NMP_S_WOOD,
  NMP_S_STBLCP, NMP_S_FASTCP, NMP_S_CM, NMP_S_CH,
  NMP_NSTATE = 56 /* + int32 ISNOW in its own array */
};

/* Static fp / int per column (read every step). */
enum { NMP_F_LAT = 0, NMP_F_ZLVL, NMP_F_SHDFAC, NMP_F_SHDMAX, NMP_F_TBOT, NMP_F_FOLN, NMP_NSTATIC_F };
enum { NMP_I_VEGTYP = 0, NMP_I_SOILTYP, NMP_I_SLOPETYP, NMP_I_SOILCOLOR, NMP_I_IST, NMP_I_ICE,
       NMP_NSTATIC_I };

/* Forcing per step (noahmp_sflx :72-74). */
enum { NMP_A_SFCTMP = 0, NMP_A_SFCPRS, NMP_A_PSFC, NMP_A_UU, NMP_A_VV, NMP_A_Q2, NMP_A_SOLDN,
       NMP_A_LWDN, NMP_A_PRCP, NMP_A_COSZ, NMP_A_CO2AIR, NMP_A_O2AIR, NMP_NFORCING };

/* LDASIN forcing block (nmp_forcing_from_ldasin): the 8 variables of an
 * HRLDAS LDASIN file (noahmp-1_amd/ncio.py) plus the step's cosine of the
 * solar zenith angle, always fp32, field-major like every SoA array. */
enum { NMP_L_T2D = 0, NMP_L_Q2D, NMP_L_U2D, NMP_L_V2D, NMP_L_PSFC, NMP_L_RAINRATE, NMP_L_SWDOWN,
       NMP_L_LWDOWN, NMP_L_COSZ, NMP_NLDASIN };

/* Per-column climate record of the synthetic forcing generator
 * (nmp_forcing_synth): latitude / longitude (radians), mean air temperature
 * (K), diurnal amplitude (K), relative humidity (0-1), surface pressure (Pa),
 * mean wind u / v (m/s), precipitation probability per step. */
enum { NMP_CLIM_LAT = 0, NMP_CLIM_LON, NMP_CLIM_T0, NMP_CLIM_AMP, NMP_CLIM_RH, NMP_CLIM_PRES,
       NMP_CLIM_WIND_U, NMP_CLIM_WIND_V, NMP_CLIM_WET, NMP_NCLIM };

/* Full diagnostics = the 58 intent(out) args of noahmp_sflx in dummy order (:82-91). */
enum {
  NMP_D_FSA = 0, NMP_D_FSR, NMP_D_FIRA, NMP_D_FSH, NMP_D_SSOIL, NMP_D_FCEV,
  NMP_D_FGEV, NMP_D_FCTR, NMP_D_ECAN, NMP_D_ETRAN, NMP_D_EDIR, NMP_D_TRAD,
  NMP_D_TGB, NMP_D_TGV, NMP_D_T2MV, NMP_D_T2MB, NMP_D_Q2V, NMP_D_Q2B,
  NMP_D_RUNSRF, NMP_D_RUNSUB, NMP_D_APAR, NMP_D_PSN, NMP_D_SAV, NMP_D_SAG,
  NMP_D_FSNO, NMP_D_NEE, NMP_D_GPP, NMP_D_NPP, NMP_D_FVEG, NMP_D_ALBEDO,
  NMP_D_QSNBOT, NMP_D_PONDING, NMP_D_PONDING1, NMP_D_PONDING2, NMP_D_RSSUN, NMP_D_RSSHA,
  NMP_D_BGAP, NMP_D_WGAP, NMP_D_CHV, NMP_D_CHB, NMP_D_EMISSI,
  NMP_D_SHG, NMP_D_SHC, NMP_D_SHB, NMP_D_EVG, NMP_D_EVB, NMP_D_GHV,
  NMP_D_GHB, NMP_D_IRG, NMP_D_IRC, NMP_D_IRB, NMP_D_TR, NMP_D_EVC,
  NMP_D_CHLEAF, NMP_D_CHUC, NMP_D_CHV2, NMP_D_CHB2, NMP_D_FPICE,
  NMP_NDIAG_FULL = 58
};

/* Output-step surface fluxes, gathered across ranks at output steps. */
enum {
  NMP_O_FSA = 0, NMP_O_FSR, NMP_O_FIRA, NMP_O_FSH, NMP_O_SSOIL, NMP_O_FCEV, NMP_O_FGEV,
  NMP_O_FCTR, NMP_O_ECAN, NMP_O_ETRAN, NMP_O_EDIR, NMP_O_TRAD, NMP_O_RUNSRF, NMP_O_RUNSUB,
  NMP_O_T2M, NMP_O_ALBEDO, NMP_NDIAG_OUT = 16
};

/* Accumulators of an output interval (nmp_accumulate), always double: rows
 * 0..15 mirror NMP_O_* (flux x seconds), row 16 is the precipitation. */
enum {
  NMP_ACC_FSA = 0, NMP_ACC_FSR, NMP_ACC_FIRA, NMP_ACC_FSH, NMP_ACC_SSOIL, NMP_ACC_FCEV,
  NMP_ACC_FGEV, NMP_ACC_FCTR, NMP_ACC_ECAN, NMP_ACC_ETRAN, NMP_ACC_EDIR, NMP_ACC_TRAD,
  NMP_ACC_RUNSRF, NMP_ACC_RUNSUB, NMP_ACC_T2M, NMP_ACC_ALBEDO, NMP_ACC_PRCP, NMP_NACC = 17
};

/* An interval's accumulated output (nmp_accum_finish), engine precision: 11
 * time means (LDASOUT <F>_MEAN), 6 totals in mm (the HRLDAS ACC* fields), the
 * change of the column's water storage (mm) and the water budget's residual
 * (mm): DSTOR - (ACCPRCP - ACCECAN - ACCETRAN - ACCEDIR - SFCRNOFF - UGDRNOFF). */
enum {
  NMP_B_FSA_MEAN = 0, NMP_B_FSR_MEAN, NMP_B_FIRA_MEAN, NMP_B_FSH_MEAN, NMP_B_SSOIL_MEAN,
  NMP_B_FCEV_MEAN, NMP_B_FGEV_MEAN, NMP_B_FCTR_MEAN, NMP_B_TRAD_MEAN, NMP_B_T2M_MEAN,
  NMP_B_ALBEDO_MEAN, NMP_B_ACCPRCP, NMP_B_ACCECAN, NMP_B_ACCETRAN, NMP_B_ACCEDIR,
  NMP_B_SFCRNOFF, NMP_B_UGDRNOFF, NMP_B_DSTOR, NMP_B_WBRES, NMP_NBUDGET = 19
};

/* diag_level for nmp_step */
enum { NMP_DIAG_NONE = 0, NMP_DIAG_OUT = 1, NMP_DIAG_FULL = 2 };

/* Per-column status bits (replace wrf_error_fatal / wrf_message). */
enum {
  NMP_ST_ERRSW = 1,   /* |SWDOWN-(FSA+FSR)| > 0.01     func.f90:688-710 */
  NMP_ST_ERRENG = 2,  /* |energy residual| > 0.01 W/m2 func.f90:712-721 */
  NMP_ST_FIRE = 4,    /* emitted longwave <= 0         func.f90:1284-1292 */
  NMP_ST_HCAN = 8,    /* HCAN <= ZPD                   func.f90:2726-2738 */
  NMP_ST_ZLVL = 16,   /* ZLVL <= ZPD                   func.f90:3412-3415 */
  NMP_ST_FLERCH = 32, /* Flerchinger fallback (info)   func.f90:4588-4590 */
  NMP_ST_OPTVEG = 64, /* unknown opt_veg               func.f90:375-377 */
  NMP_ST_STOP = 128   /* FIRE|ZLVL as the reference oracle reports them (one message) */
};

/* ---- one column, the reference calling sequence ---------------------------
 * All 131 noahmp_sflx dummy arguments (core/module_noahmp_func.f90:66-91), in
 * dummy-argument order.  Every member is 4 bytes and there is no padding, so a
 * Fortran `type, bind(C)` with the same components in the same order maps onto
 * it 1:1.  Arrays follow the reference bounds in C order:
 * stc/zsnso[k] = Fortran (k-2), ficeold/snice/snliq[j] = (j-2),
 * zsoil/soilwat/smc[k] = (k+1). */
typedef struct nmp_sflx_args {
  /* IN: time/space (:67) */
  int32_t iloc, jloc;
  float lat;
  int32_t yearlen;
  float julian, cosz;
  /* IN: model configuration (:68) */
  float dt, dx, dz8w;
  int32_t nsoil;
  float zsoil[NMP_NSOIL];
  int32_t nsnow;
  /* IN: vegetation / soil characteristics (:69-70) and the unused IZ0TLND (:71) */
  float shdfac, shdmax;
  int32_t slptyp, sltyp, lutyp, ice, ist, isc, iz0tlnd;
  /* IN: forcing (:72-74) */
  float sfctmp, sfcprs, psfc, uu, vv, q2, qc, soldn, lwdn, prcp, tbot, co2air, o2air, foln;
  float ficeold[NMP_NSNOW];
  float pblh, zlvl;
  /* IN/OUT (:75-80) */
  float albold, sneqvo;
  float stc[NMP_NLAYER], soilwat[NMP_NSOIL], smc[NMP_NSOIL];
  float tah, eah, fwet, canliq, canice, tv, tg, qsfc, qsnow;
  int32_t isnow;
  float zsnso[NMP_NLAYER], snowh, sneqv, snice[NMP_NSNOW], snliq[NMP_NSNOW];
  float zwt, wa, wt, wslake, lfmass, rtmass, stmass, wood, stblcp, fastcp, lai, sai;
  float cm, ch, tauss;
  /* OUT (:82-91): the 58 intent(out) arguments, indexed by NMP_D_* */
  float out[NMP_NDIAG_FULL];
  /* OUT: NMP_ST_* bits of this call (what wrf_error_fatal / wrf_message reported) */
  int32_t status;
} nmp_sflx_args;

/* ---- errors -------------------------------------------------------------- */
enum {
  NMP_OK = 0,
  NMP_E_ARG = -1,      /* bad argument / null pointer / ld < ncol          */
  NMP_E_TABLE = -2,    /* table file missing, block not found, parse error */
  NMP_E_OPTION = -3,   /* option value outside the reference's range      */
  NMP_E_DEVICE = -4,   /* HIP error (no device, launch failure)           */
  NMP_E_PRECISION = -5, /* precision not 4 or 8                           */
  NMP_E_CALENDAR = -6   /* julian outside [0, yearlen] (split a run at the
                           year boundary; see nmp_step)                     */
};

typedef struct nmp_engine nmp_engine;

/* Parse GENPARMMP.TBL / SOILPARMMP.TBL / VEGPARMMP.TBL from tbl_dir with the
 * reference's block/tag rules ("&NAME" or "&NAME#TAG").  soil_tag is e.g.
 * "STAS" or "STAS-RUC", veg_tag "USGS" or "MODIFIED_IGBP_MODIS_NOAH".  Every
 * field not present in the tables is NaN, as in the reference (nan4 init). */
int nmp_read_tables(const char* tbl_dir, const char* soil_tag, const char* veg_tag,
                    nmp_params* out);

/* Create an engine on HIP device `device` computing in `precision` (4|8)
 * bytes.  Copies the tables to the device once. */
int nmp_init(const nmp_params* params, const nmp_options* opts, int device, int precision,
             nmp_engine** out);

/* One noahmp_sflx time step for ncol columns (all pointers device, SoA with
 * leading dimension ld).  zsoil[4] (<0, m) and dt are domain-wide; julian /
 * yearlen are the step's calendar position (noahmp_sflx :67), 0 <= julian <=
 * yearlen, else NMP_E_CALENDAR (far enough outside it the reference's
 * phenology reads its monthly LAI/SAI tables out of bounds).  FICEOLD is
 * derived on device from SNICE/SNLIQ at step start, as an offline driver does.
 * diag may be NULL when diag_level == NMP_DIAG_NONE; col_status is OR-ed
 * (caller zeroes it when it wants a fresh mask). */
int nmp_step(nmp_engine* eng, int64_t ncol, int64_t ld, const float zsoil[4], float dt,
             float julian, int32_t yearlen, void* state, int32_t* isnow, const void* static_f,
             const int32_t* static_i, const void* forcing, void* diag, int diag_level,
             int32_t* col_status, void* stream);

/* Column re-binning (no reference counterpart: a scheduling aid for the wave's
 * slowest-lane cost).  nmp_step_binned is nmp_step where lane i
 * steps column order[i] (order: a permutation of 0..ncol-1, device int32, or
 * NULL for the identity) and, when cost is non-NULL, each column's loop-cost
 * key (its vege_flux Newton trip count this step, 0 without a canopy; one byte
 * per column, indexed by column) is written.  Every column reads and writes
 * only its own index in every array, so results are bit-identical for any
 * order.  nmp_rebin builds an order from such keys: within each tile of `tile`
 * consecutive columns (a multiple of 64), the columns sorted by key, so that
 * the waves of the next step hold columns of similar cost.
 * PRECONDITION (not checked by the library): order must be a permutation of
 * 0..ncol-1.  A duplicate entry makes two lanes step the same column at once
 * (a data race on its state) and an entry outside [0, ncol) reads and writes
 * outside the arrays; neither is reported.  Orders built by nmp_rebin satisfy
 * it; the Python Engine.step checks a caller-supplied order when
 * NMP_CHECK_ORDER=1. */
int nmp_step_binned(nmp_engine* eng, int64_t ncol, int64_t ld, const float zsoil[4], float dt,
                    float julian, int32_t yearlen, void* state, int32_t* isnow,
                    const void* static_f, const int32_t* static_i, const void* forcing, void* diag,
                    int diag_level, int32_t* col_status, const int32_t* order, uint8_t* cost,
                    void* stream);
int nmp_rebin(nmp_engine* eng, int64_t ncol, const uint8_t* cost, int32_t* order, int32_t tile,
              void* stream);

/* Same step, many times: nsteps steps (one launch each, enqueued on stream)
 * whose forcing slices are forcing + (s % forcing_period)*forcing_stride
 * (elements, real type; forcing_period 0 = nsteps distinct slices), julian
 * advancing by dt/86400 per step (julian0 + (float)s*dt/86400.0f, every one
 * within [0, yearlen], else NMP_E_CALENDAR: split a run at the year
 * boundary, the next year with its own yearlen, as the reference's driver
 * recomputes the day of year every step);
 * bitwise the same as nsteps nmp_step calls.  diag (if non-NULL) receives the last step only. */
/* Synthetic forcing for one step, generated on the device (no reference
 * counterpart: the reference reads LDASIN files, run/case.nml:6-7, and ships
 * none).  Writes the 12 NMP_A_* fields of ncol columns
 * (SoA, leading dimension ld, engine precision) from their NMP_CLIM_* climate
 * records: a diurnal temperature cycle at local solar time, solar geometry,
 * cloud, humidity, wind and precipitation, with every random draw a
 * counter-based hash of (seed, step, first_col + column, draw).  Stateless:
 * any step of any column can be generated on its own, on any rank. */
int nmp_forcing_synth(nmp_engine* eng, int64_t ncol, int64_t ld, const void* climate,
                      double julian, int32_t yearlen, uint64_t seed, int64_t step,
                      int64_t first_col, void* forcing, void* stream);

/* The 12 NMP_A_* forcing fields of one step (SoA, leading dimension ld,
 * engine precision) from an LDASIN block (fp32, NMP_NLDASIN x ld): the
 * fields noahmp_sflx takes (core/module_noahmp_func.f90:72-74) that the
 * files do not carry are formed on the device -- SFCPRS = PSFC, CO2AIR =
 * 395e-6 PSFC, O2AIR = 0.209 PSFC (one double product rounded to fp32, as the
 * offline driver's host reader forms them) -- so a host uploads 36 B per
 * column per step instead of 48 (fp32) or 96 (fp64).  Device pointers,
 * enqueued on `stream`.  Hosts that supply all 12 fields write the forcing
 * array themselves and skip this call. */
int nmp_forcing_from_ldasin(nmp_engine* eng, int64_t ncol, int64_t ld, const float* ldasin,
                            void* forcing, void* stream);

/* As nmp_forcing_from_ldasin, with COSZ formed on the device instead of read
 * from the block (its NMP_L_COSZ row is not read): geo is (3, ld) double per
 * column -- sin(lat), cos(lat), lon (radians) -- and the step's solar terms
 * come from the host (sin_decl, cos_decl of the declination; ha0 = 2 pi x the
 * UTC fraction of the day).  COSZ = sin_lat sin_decl + (cos_lat cos_decl)
 * cos((ha0 + lon) - pi) in double, rounded once to fp32: the offline driver's
 * host expression (noahmp-1_amd/timeman.py cosz) in its operation order, with
 * the device's double cosine.  A host then uploads an LDASIN file's 8
 * variables once per input interval and nothing on the steps in between. */
int nmp_forcing_from_ldasin_geo(nmp_engine* eng, int64_t ncol, int64_t ld, const float* ldasin,
                                const double* geo, double sin_decl, double cos_decl, double ha0,
                                void* forcing, void* stream);

/* Rows NMP_L_T2D..NMP_L_LWDOWN of an LDASIN block (fp32, leading dimension
 * ld, ncol columns) from the file's own bytes: grid_be holds the 8 variables
 * in NMP_L_* order, each npts grid points of big-endian fp32 as a netCDF-3
 * file stores them, and column c of the block takes grid point point[c]
 * (the land-point selection and the host's column order in one index; a
 * column whose point lies outside [0, npts) gets NaN rows).  The NMP_L_COSZ
 * row is not written.  A host then
 * copies each file's bytes and uploads them; byte order and gather happen
 * here.  Device pointers, enqueued on `stream`. */
int nmp_ldasin_ingest(nmp_engine* eng, int64_t ncol, int64_t ld, int64_t npts,
                      const void* grid_be, const int32_t* point, float* ldasin, void* stream);

/* Forcing on its own grid (no counterpart in the reference, which has no
 * forcing reader): rows NMP_L_T2D..NMP_L_LWDOWN of an LDASIN block (fp32,
 * leading dimension ld, ncol columns, possibly offset by a range's first
 * column like nmp_ldasin_ingest's) from a file stored on another, coarser
 * grid.  grid_be holds the 8 variables in NMP_L_* order, each npts source
 * points of big-endian fp32 as a netCDF-3 file stores them.  Column c has four
 * source entries k = 0..3: source point corner[k*ld + c] (int32) with weight
 * weight[k*ld + c] (double) -- for a bilinear plan the cell's corners
 * (j0,i0), (j0,i0+1), (j0+1,i0), (j0+1,i0+1).  The operation order below is
 * part of this interface: the result's bits depend on the plan and the values
 * alone, and a host can restate them (noahmp-1_amd/regrid.py apply_host).
 * All arithmetic is IEEE double, each operation rounded once (no fused
 * multiply-add).  Per column and per variable v:
 *  - bilinear: x = +0.0; for k = 0, 1, 2, 3 in this order, if corner[k] >= 0:
 *    x = x + (double)value_k * weight_k (one rounded product, then one add),
 *    value_k the byte-swapped fp32 word grid_be[v*npts + corner[k]]; the row
 *    gets (float)x.
 *  - an entry with corner[k] < 0 is a masked source point: skipped, its value
 *    never loaded nor multiplied, so no NaN*0 arises from it.
 *  - nearest (bit v of nearest_mask set, e.g. 1u << NMP_L_RAINRATE): among the
 *    entries with corner[k] >= 0 the one of largest weight, ties to the lowest
 *    k; that word's (byte-swapped) bits go to the row unchanged.
 *  - a column with no valid entry, or with any corner[k] >= npts, gets
 *    quiet-NaN rows (0x7fc00000) and no out-of-bounds load, as
 *    nmp_ldasin_ingest gives a column outside the grid.
 * The NMP_L_COSZ row is not written.  Device pointers, one kernel enqueued on
 * `stream`.  NMP_E_ARG for ld < ncol, npts < 1 or npts >= 2^29, or a NULL
 * pointer; ncol == 0 is NMP_OK with nothing enqueued.
 *
 * nmp_ldasin_downscale corrects such a block in place for the elevation
 * difference dz[c] (fp32, metres: model terrain minus the source grid's
 * elevation interpolated to the column) with the lapse rate `lapse` (K/m,
 * e.g. 0.0065).  Rows T2D, Q2D, PSFC and LWDOWN, in double from the fp32
 * values t0, q0, p0, lw0, with G = 9.80616 and RD = 287.04 (the reference's
 * GRAV and RAIR, core/module_noahmp_const.f90:17,32), every operation one IEEE
 * operation in this order:
 *   d   = (double)dz[c]
 *   t1  = t0 - lapse*d
 *   tm  = 0.5*(t0 + t1)
 *   p1  = p0 * exp(-(G*d) / (RD*tm))                  hypsometric
 *   a(t) = (17.67*(t - 273.15)) / (t - 29.65)
 *   q1  = (q0 * exp(a(t1) - a(t0))) * (p0/p1)         relative humidity kept (Magnus)
 *   r   = t1/t0
 *   lw1 = lw0 * ((r*r)*(r*r))
 * each result rounded once to fp32 (t1 enters the later lines unrounded).  Wind,
 * SWDOWN, RAINRATE and COSZ are untouched; with dz == 0 every row comes back
 * bit-identical.  exp is the device's double exponential (within 1 ulp of a
 * correctly rounded one), so PSFC and Q2D may differ from a host's by one fp32
 * ulp; T2D and LWDOWN do not. */
int nmp_ldasin_regrid(nmp_engine* eng, int64_t ncol, int64_t ld, int64_t npts,
                      const void* grid_be, const int32_t* corner, const double* weight,
                      uint32_t nearest_mask, float* ldasin, void* stream);
int nmp_ldasin_downscale(nmp_engine* eng, int64_t ncol, int64_t ld, const float* dz, double lapse,
                         float* ldasin, void* stream);

/* Forcing between input times (no counterpart in the reference, which has no
 * forcing reader): the 12 NMP_A_* fields of the step that starts at t,
 * t0 <= t < t1, from the two resident LDASIN blocks of the input times t0
 * (ldasin0) and t1 (ldasin1), both fp32 with leading dimension ld like
 * nmp_forcing_from_ldasin_geo's, possibly offset by a range's first column.
 * The operation order below is part of this interface: the result's bits
 * depend on the two blocks, the weight and the step's COSZ alone, and a host
 * can restate them (noahmp-1_amd/tinterp.py interp_host).  All arithmetic is
 * IEEE double, each operation rounded once (no fused multiply-add); each
 * result is rounded once to fp32 and that fp32 value is widened to the engine
 * precision, as nmp_forcing_from_ldasin does.
 *  - weights: w1 = (t - t0) / (t1 - t0), formed by the caller in double,
 *    0 <= w1 < 1; w0 = 1.0 - w1 is formed once on the host side of the call
 *    and is what the kernel uses.
 *  - w1 == 0.0: the result is nmp_forcing_from_ldasin_geo(ldasin0, ...) bit
 *    for bit in all 12 fields, SWDOWN included; ldasin1 is not read and may be
 *    NULL (NaNs in it cannot leak).
 *  - COSZ (NMP_A_COSZ) = (float)(sin_lat*sin_decl + (cos_lat*cos_decl) *
 *    cos((ha0 + lon) - pi)): nmp_forcing_from_ldasin_geo's expression, operation
 *    order, geo layout and solar terms, at the step's own time t.
 *  - a plain variable v (T2D, Q2D, U2D, V2D, PSFC, LWDOWN, and RAINRATE and
 *    SWDOWN when not treated otherwise below), a and b its fp32 values in
 *    blocks 0 and 1: x = (double)a*w0 + (double)b*w1 -- two rounded products,
 *    then one add, in that order; the row gets (float)x.
 *  - a held variable (bit v of hold_mask, v < NMP_L_COSZ; e.g. 1u <<
 *    NMP_L_RAINRATE, an interval rate): block 0's bits, unchanged; block 1's
 *    row of it is never loaded.
 *  - SWDOWN with sw_zenith != 0 and its bit not in hold_mask: with czt =
 *    (double)COSZ, the fp32 value above widened, cz0 and cz1 the two blocks'
 *    NMP_L_COSZ rows widened to double (nmp_ldasin_cosz writes them), sw0 and
 *    sw1 the blocks' SWDOWN and floor = cosz_floor:
 *      m0 = cz0 > floor ? cz0 : floor        m1 = cz1 > floor ? cz1 : floor
 *      k0 = (double)sw0 / m0                 k1 = (double)sw1 / m1
 *      k  = k0*w0 + k1*w1                    (two products, then one add)
 *      sw = czt > 0 ? czt*k : 0.0            rounded once to fp32
 *    A NaN czt, cz0 or cz1 fails its comparison: a NaN czt gives 0.0, a NaN
 *    cz0 or cz1 takes the floor.  Working from the fp32-rounded COSZ values is
 *    deliberate: the device's double cosine is not correctly rounded, and a
 *    host that is given the three COSZ rows still reproduces every bit.
 *    cosz_floor (in (0, 1]; the offline driver's default is 0.05) bounds the
 *    clearness ratio sw/cz at sunrise and sunset; it is a setting, not a
 *    measurement.  Where both end points are darker than the floor and the
 *    files' SWDOWN is 0 the result is 0.  With sw_zenith == 0 SWDOWN is a plain
 *    variable and the blocks' NMP_L_COSZ rows are not read.
 *  - SFCPRS = PSFC = the interpolated fp32 PSFC; CO2AIR = (float)(395e-6 *
 *    (double)PSFC) and O2AIR = (float)(0.209 * (double)PSFC) from that fp32
 *    value, as nmp_forcing_from_ldasin derives them from the file's.
 * Device pointers, one kernel enqueued on `stream` (one double cosine per
 * column).  NMP_E_ARG, with nothing enqueued and the outputs untouched, for
 * ld < ncol, w1 outside [0, 1) or NaN, a hold_mask bit at or above NMP_L_COSZ,
 * sw_zenith with cosz_floor outside (0, 1] or NaN, a NULL ldasin0, geo or
 * forcing, or a NULL ldasin1 with w1 != 0; ncol == 0 is NMP_OK with nothing
 * enqueued.
 *
 * nmp_ldasin_cosz writes row NMP_L_COSZ of a resident block: COSZ at the
 * block's own input time, by the expression above from the same geo and that
 * time's solar terms -- one cosine per column per input interval.  The other
 * rows and the columns ncol..ld-1 are untouched.  NMP_E_ARG for ld < ncol or a
 * NULL geo or ldasin; ncol == 0 is NMP_OK. */
int nmp_ldasin_cosz(nmp_engine* eng, int64_t ncol, int64_t ld, const double* geo, double sin_decl,
                    double cos_decl, double ha0, float* ldasin, void* stream);
int nmp_forcing_from_ldasin_interp(nmp_engine* eng, int64_t ncol, int64_t ld,
                                   const float* ldasin0, const float* ldasin1, double w1,
                                   uint32_t hold_mask, int sw_zenith, double cosz_floor,
                                   const double* geo, double sin_decl, double cos_decl, double ha0,
                                   void* forcing, void* stream);

/* The output side's mirror: nfield diagnostics of ncol columns (engine
 * precision, field-major, leading dimension ld -- e.g. the NMP_O_* fluxes of
 * nmp_step's diag at level 1) onto the LDASOUT file's grids as a netCDF-3
 * file stores them: grid_be = nfield grids of npts points of big-endian
 * engine-precision reals, `fill` (rounded to the engine precision) where no
 * column lands; column c goes to grid point point[c] (a point outside
 * [0, npts) is skipped).  A host then writes the bytes as they are.  Device
 * pointers, enqueued on `stream`. */
int nmp_ldasout_grid(nmp_engine* eng, int64_t ncol, int64_t ld, int64_t npts, int nfield,
                     const void* diag, const int32_t* point, double fill, void* grid_be,
                     void* stream);

/* Accumulated output over an output interval (no reference counterpart: the
 * reference forms the column water storage and the step's residual ERRWAT,
 * core/module_noahmp_func.f90:339-344 and :723-731, and drops them).  Device
 * pointers, SoA with leading dimension ld, possibly offset by a range's first
 * column like nmp_step's; each call only enqueues one kernel on `stream`.
 *  - nmp_accumulate: after a step at NMP_DIAG_OUT, acc[f] = acc[f] +
 *    (double)v * (double)dt for the 16 NMP_O_* rows of `diag` (engine
 *    precision) and row NMP_A_PRCP of the step's `forcing` block; acc is
 *    NMP_NACC x ld double for both precisions (NMP_ACC_*), zeroed by the
 *    caller before the first interval.
 *  - nmp_water_storage: storage[c] (engine precision) = the reference's
 *    BEG_WB / END_WB of the column's state, in its operation order:
 *    ((CANLIQ + CANICE) + SNEQV) + WA, then + (SMC(IZ) * DZSNSO(IZ)) * 1000
 *    for soil layers 1..4 (DZSNSO from ZSNSO and ISNOW, func.f90:322-328);
 *    0 where IST != 1 (static_i row NMP_I_IST).
 *  - nmp_accum_finish: the interval's NMP_B_* block `out` (NMP_NBUDGET x ld,
 *    engine precision T): means (T)(acc / span_s), totals (T)acc,
 *    DSTOR = (T)d with d = (double)stor_end - (double)stor_beg, and
 *    WBRES = (T)(d - (((((P - ECAN) - ETRAN) - EDIR) - RUNSRF) - RUNSUB)) from
 *    the double totals.  Then every acc entry of the column is set to +0.0 and
 *    stor_end is copied to stor_beg: the next interval starts with no further
 *    call.  span_s (seconds accumulated) <= 0 is NMP_E_ARG. */
int nmp_accumulate(nmp_engine* eng, int64_t ncol, int64_t ld, float dt, const void* diag,
                   const void* forcing, double* acc, void* stream);
int nmp_water_storage(nmp_engine* eng, int64_t ncol, int64_t ld, const void* state,
                      const int32_t* isnow, const int32_t* static_i, void* storage, void* stream);
int nmp_accum_finish(nmp_engine* eng, int64_t ncol, int64_t ld, double span_s, double* acc,
                     const void* stor_end, void* stor_beg, void* out, void* stream);

/* Region-aggregated output (no counterpart in the reference): for each of
 * nfield fields of the field-major block `fields` (engine precision T,
 * fields[f*ld + c], ncol columns; e.g. nmp_step's diag or an output step's
 * 35-field block) the weighted sum, and optionally the weighted mean, over the
 * columns of each of nreg regions.  The summation tree is fixed by the plan
 * below and is part of this interface: the result's bits do not depend on the
 * launch shape, the stream, the world size or anything but the plan and the
 * values, and a host can restate them.  All arithmetic is IEEE double, each
 * operation rounded once (no fused multiply-add), no atomics.
 *
 * Plan (built once by the caller; device arrays):
 *  - The columns of a region are listed in ascending column order, region
 *    after region; each region's list is padded to a multiple of
 *    NMP_REGION_CHUNK = 256 entries.  entry_col[e] (int32) is entry e's column,
 *    -1 for a pad; entry_w[e] (double) its weight, 0 for a pad.  A *chunk* is
 *    256 consecutive entries; there are nchunk of them (nchunk*256 entries).
 *  - region_chunk0[nreg+1] (int64): region r owns chunks region_chunk0[r] ..
 *    region_chunk0[r+1]-1.  A region without columns owns no chunk.
 *  - wsum[nreg] (double): the divisor of the means -- by convention the same
 *    tree applied to a field of ones, i.e. to the weights.
 * Pass 1, per chunk k and field f, as 64 lanes: lane l starts at x = +0.0 and
 * for j = 0, 1, 2, 3 in this order takes entry e = 256 k + 64 j + l; if
 * entry_col[e] >= 0: x = x + (double)fields[f*ld + entry_col[e]] * entry_w[e]
 * (one rounded product, then one add).  A pad entry is skipped: its value is
 * never loaded nor multiplied, so no NaN*0 arises from it (an entry_col >= ncol
 * is skipped likewise).  Then, for s = 32, 16, 8, 4, 2, 1:
 * x[l] = x[l] + x[l xor s] for every lane; partial[f*nchunk + k] = x[0].
 * With a the 64 lane values, that is numpy's
 *   for s in (32, 16, 8, 4, 2, 1): a = a[:s] + a[s:2*s]
 * Pass 2, per region r and field f: sum = +0.0; for k = region_chunk0[r] ..
 * region_chunk0[r+1]-1 in this order: sum = sum + partial[f*nchunk + k];
 * sums[f*nreg + r] = sum and, where means is not NULL,
 * means[f*nreg + r] = sum / wsum[r] (one division).  A region without chunks
 * gives sum +0.0 and, with wsum 0, mean NaN (0/0).
 * Values reduce as they are: a NaN column makes its region's sum NaN (and no
 * other's), and the night-time ALBEDO = -999.9 (hazard H8) enters a mean as
 * that number; nothing is masked.
 * partial is caller scratch of nfield*nchunk doubles; sums and means are
 * nfield*nreg doubles.  Device pointers; both passes are enqueued on `stream`
 * in that order and the call neither synchronises nor allocates.  NMP_E_ARG
 * for nfield < 1, ld < ncol, a negative count or a NULL pointer other than
 * means; nchunk == 0 or nreg == 0 is NMP_OK with nothing enqueued. */
enum { NMP_REGION_CHUNK = 256 };
int nmp_region_reduce(nmp_engine* eng, int64_t ncol, int64_t ld, int nfield, const void* fields,
                      int64_t nchunk, const int32_t* entry_col, const double* entry_w,
                      int64_t nreg, const int64_t* region_chunk0, const double* wsum,
                      double* partial, double* sums, double* means /* may be NULL */,
                      void* stream);

/* State output (no counterpart in the reference, which writes no output): the
 * land state of an output step as output rows, formed from the state block
 * (NMP_S_* rows, engine precision T, leading dimension ld), ISNOW and the
 * static integers, next to the output step's fluxes.  The rows come in groups
 * (NMP_X_*, group g is bit g of `groups`); the rows of the selected groups are
 * written compactly in group order: row k of them goes to out[k*ld_out + c]
 * (T, ld_out >= ncol).  The groups' widths are NMP_X_WIDTHS; the first
 * NMP_NXROWS_NOFILL rows of the full block (groups NMP_X_SOIL_M ..
 * NMP_X_CARBON) never hold `fill`, the last three groups can.  `groups` is
 * uniform over the launch: an unselected group costs neither a load nor a
 * store.  One lane per column; pointers may be offset by a range's first
 * column, as for nmp_water_storage; one kernel enqueued on `stream`.
 *
 * The operation order below is part of this interface: every operation is one
 * IEEE operation, rounded once (no fused multiply-add), in the order stated, so
 * a host given the same arrays reproduces every bit
 * (noahmp-1_amd/stateout.py state_output_host).
 *
 * Layers.  Soil layer i = 1..4 is C index i + 2 of the 7-layer STC / ZSNSO and
 * index i - 1 of SMC / SH2O.  Its thickness dz_i is formed in T as
 * nmp_water_storage forms it: zb = ZSNSO[i+2]; dz_i = -zb where
 * i == isnow + 1, else ZSNSO[i+1] - zb.  Snow layer k is C index 0..2; it is
 * active when k >= isnow + 3.
 *
 * Groups that never hold `fill`, in this order:
 *   SOIL_M  (4)  SMC as stored
 *   SOIL_W  (4)  SH2O as stored
 *   SOIL_T  (4)  STC[3..6] as stored
 *   SNEQV, SNOWH, TG, TV, LAI, SAI, ZWT, WA  (1 each)  the state value
 *   CANWAT  (1)  CANLIQ + CANICE, one add in T
 *   ISNOW   (1)  (T)isnow
 *   SNOWLIQ (1)  from +0: + SNLIQ[k] over the active layers, top to bottom, in T
 *   TWS     (1)  the expression of nmp_water_storage, bit for bit:
 *                ((CANLIQ + CANICE) + SNEQV) + WA, then for i = 1..4
 *                + (SMC_i * dz_i) * 1000, in T; 0 where IST != 1
 *   SOILSAT (1)  in double, starting from +0.0, over i = 1..4:
 *                num += (double)SMC_i*(double)dz_i and
 *                den += (double)smcmax*(double)dz_i; the result is (T)(num/den).
 *                smcmax is the table value of the column's soil type
 *                (soil[SOILTYP-1].smcmax, fp32)
 *   ROOT_M  (1)  the same sums, but over i <= nroot, with den += (double)dz_i;
 *                the result is (T)(num/den).  nroot < 1 gives +0.0.  nroot is
 *                the table value of the column's vegetation type
 *                (veg[VEGTYP-1].nroot)
 *   CARBON  (6)  LFMASS RTMASS STMASS WOOD STBLCP FASTCP as stored (NaN stays
 *                NaN, hazard H13)
 * Groups that can hold `fill`, the block's last rows:
 *   SNOW_T  (3)  STC[0..2]; fill on an inactive layer
 *   SNOW_Z  (3)  thickness of a snow layer: the top active one -ZSNSO[k], the
 *                others ZSNSO[k-1] - ZSNSO[k], in T; fill where inactive
 *   SNOWT_AVG (1)  in double, starting from +0.0, over the active layers top to
 *                bottom: m_k = (double)(SNICE[k] + SNLIQ[k]), where the add is
 *                done in T; num += m_k*(double)STC[k] and den += m_k; the result
 *                is (T)(num/den).  It is fill where isnow == 0 or den == 0
 * `fill` is rounded once to T.
 * A SOILTYP outside 1..NMP_MSLTYP or a VEGTYP outside 1..NMP_MLUTYP (outside
 * its table) gives quiet NaN for SOILSAT or ROOT_M respectively and causes no
 * out-of-bounds load, as nmp_ldasin_regrid treats a bad corner.
 * NMP_E_ARG, with nothing enqueued, for groups == 0, a bit at or above
 * NMP_NXGROUP, ld < ncol, ld_out < ncol or a NULL pointer; ncol == 0 (with a
 * valid mask) is NMP_OK with nothing enqueued. */
enum {
  NMP_X_SOIL_M = 0, NMP_X_SOIL_W, NMP_X_SOIL_T, NMP_X_SNEQV, NMP_X_SNOWH, NMP_X_TG, NMP_X_TV,
  NMP_X_LAI, NMP_X_SAI, NMP_X_ZWT, NMP_X_WA, NMP_X_CANWAT, NMP_X_ISNOW, NMP_X_SNOWLIQ,
  NMP_X_TWS, NMP_X_SOILSAT, NMP_X_ROOT_M, NMP_X_CARBON, NMP_X_SNOW_T, NMP_X_SNOW_Z,
  NMP_X_SNOWT_AVG, NMP_NXGROUP = 21
};
/* rows of each group, in group order; the groups from NMP_X_SNOW_T on can hold `fill` */
#define NMP_X_WIDTHS {4, 4, 4, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 6, 3, 3, 1}
#define NMP_NXROWS_NOFILL 32 /* rows of groups NMP_X_SOIL_M .. NMP_X_CARBON */
#define NMP_NXROWS 39        /* rows of all groups */
int nmp_state_output(nmp_engine* eng, int64_t ncol, int64_t ld, const void* state,
                     const int32_t* isnow, const int32_t* static_i, uint32_t groups,
                     double fill, void* out, int64_t ld_out, void* stream);

/* Spin-up drift (no counterpart in the reference): a spin-up runs the forcing
 * period over and over from the state the last pass left until the state at
 * the end of a pass stops changing.  nmp_state_drift measures that change per
 * column next to the state, nmp_drift_reduce reduces it to a few dozen
 * numbers, so a loop's convergence test costs no copy of the state.
 *
 * Tracked values (NMP_K_*, NMP_NTRACKED = 13 rows, engine precision T), formed
 * from the state block (NMP_S_* rows, leading dimension ld), ISNOW and the
 * static integers.  Every operation is one IEEE operation, rounded once (no
 * fused multiply-add), in the order stated, so a host given the same arrays
 * reproduces every bit (noahmp-1_amd/spinup.py tracked_host, drift_host):
 *   rows 0..3   SMC[i], i = 0..3, as stored
 *   rows 4..7   STC[NMP_NSNOW + i], i = 0..3, as stored
 *   row  8      SNEQV      row 9   WA      row 10   ZWT, as stored
 *   row  11     TWS: the expression of nmp_water_storage, bit for bit:
 *               ((CANLIQ + CANICE) + SNEQV) + WA, then for i = 1..4
 *               + (SMC_i * dz_i) * 1000 in T, with zb = ZSNSO[i+2] and
 *               dz_i = -zb where i == isnow + 1, else ZSNSO[i+1] - zb;
 *               0 where IST != 1
 *   row  12     CTOT = ((((LFMASS + RTMASS) + STMASS) + WOOD) + STBLCP) + FASTCP
 * The kernel reads those state rows and no others: SMC, STC[3..6], SNEQV, WA,
 * ZWT, ZSNSO[2..6], CANLIQ, CANICE and the six pools, plus ISNOW and IST.
 *
 * Drift groups (NMP_G_*, NMP_NDRIFT = 7 rows, T) against the snapshot `snap`
 * of the tracked values an earlier call stored:
 *   SNEQV, WA, ZWT, TWS, CARBON   fabs(now - snap) of rows 8, 9, 10, 11, 12:
 *                                 one subtraction in T
 *   SOIL_M (rows 0..3), SOIL_T (rows 4..7)   x_i = fabs(now_i - snap_i) of the
 *                                 four layers; m = x_0, then for i = 1, 2, 3:
 *                                 m = (x_i > m || x_i != x_i) ? x_i : m.  A NaN
 *                                 sticks: once m is NaN no layer replaces it.
 *
 * nmp_state_drift, one lane per column: where drift is not NULL it writes the
 * 7 drift rows (drift[g*ld_drift + c]) of the state against snap; then it
 * stores the new tracked values into snap (snap[k*ld_snap + c]), so one call
 * measures a loop and arms the next.  With drift NULL it only takes the
 * snapshot (snap is not read).  Columns >= ncol and rows beyond those named
 * are never touched.  Pointers may be offset by a range's first column, as for
 * nmp_water_storage; one kernel enqueued on `stream`.  NMP_E_ARG, with nothing
 * enqueued, for ld < ncol, ld_snap < ncol, ld_drift < ncol (with a drift), or a
 * NULL state, isnow, static_i or snap; ncol == 0 is NMP_OK with nothing
 * enqueued.
 *
 * nmp_drift_reduce reduces the 7 drift rows (T, drift[g*ld_drift + c]) of ncol
 * columns -- one call for the rank's whole block.  weight (double[ncol], or
 * NULL = 1 for every column) is the caller's mask and the mean's weight; tol
 * is double[7].  Results, per group g:
 *  - Skipped columns.  A column whose weight is exactly 0 is skipped in
 *    everything below: it is not loaded.
 *  - out_max[g]: the largest drift of the unskipped columns, converted exactly
 *    to double; the quiet NaN 0x7ff8000000000000 if any unskipped column's
 *    drift is NaN; +0.0 when no column is unskipped.
 *  - out_arg[g] (int64): the lowest column index that holds a NaN if there is
 *    one, otherwise the lowest index whose drift equals out_max[g]; -1 when no
 *    column is unskipped.
 *  - out_count[g] (int64): the number of unskipped columns with
 *    !((double)d <= tol[g]); a NaN drift counts as not converged.
 *  - out_wsum[g]: the weighted sum by a fixed tree.  One wavefront handles each
 *    chunk of NMP_DRIFT_CHUNK = 256 columns, chunk k = columns
 *    [256 k, 256 k + 256).  Lane l starts at x = +0.0 and for j = 0, 1, 2, 3 in
 *    this order takes column c = 256 k + l + 64 j; unless c >= ncol or the
 *    column is skipped: x = x + (double)d * w (one rounded product, then one
 *    add; such a column is neither loaded nor multiplied).  Then, for s = 32,
 *    16, 8, 4, 2, 1: x[l] = x[l] + x[l xor s] for every lane -- numpy's
 *      for s in (32, 16, 8, 4, 2, 1): a = a[:s] + a[s:2*s]
 *    and the chunk's partial is x[0].  Pass 2 adds the chunk partials in chunk
 *    order from +0.0.
 *  - *out_wtot: the weights summed by the same tree (x = x + w per column).
 *    The weighted mean is out_wsum[g] / *out_wtot, formed by the caller.
 * max, arg and count do not depend on the order of combination; the sum's tree
 * depends on ncol alone, never on the launch shape, the stream or T's width.
 * All arithmetic is IEEE double, each operation rounded once; no atomics.
 * partial is caller scratch of NMP_DRIFT_SCRATCH * ceil(ncol / 256) 8-byte
 * words.  Device pointers; two kernels enqueued on `stream` in order; the call
 * neither synchronises nor allocates.  NMP_E_ARG for ld_drift < ncol or a NULL
 * pointer other than weight; ncol == 0 is NMP_OK and writes the empty result
 * (max, wsum, wtot +0.0, arg -1, count 0). */
enum {
  NMP_K_SMC = 0, NMP_K_STC = 4, NMP_K_SNEQV = 8, NMP_K_WA, NMP_K_ZWT, NMP_K_TWS, NMP_K_CTOT,
  NMP_NTRACKED = 13
};
enum {
  NMP_G_SOIL_M = 0, NMP_G_SOIL_T, NMP_G_SNEQV, NMP_G_WA, NMP_G_ZWT, NMP_G_TWS, NMP_G_CARBON,
  NMP_NDRIFT = 7
};
enum { NMP_DRIFT_CHUNK = 256, NMP_DRIFT_SCRATCH = 29 };
int nmp_state_drift(nmp_engine* eng, int64_t ncol, int64_t ld, const void* state,
                    const int32_t* isnow, const int32_t* static_i, void* snap, int64_t ld_snap,
                    void* drift /* may be NULL */, int64_t ld_drift, void* stream);
int nmp_drift_reduce(nmp_engine* eng, int64_t ncol, int64_t ld_drift, const void* drift,
                     const double* weight /* may be NULL */, const double* tol, void* partial,
                     double* out_max, int64_t* out_arg, double* out_wsum, int64_t* out_count,
                     double* out_wtot, void* stream);

/* Vegetation fraction through the year (no counterpart in the reference, whose
 * caller passes SHDFAC): row NMP_F_SHDFAC of static_f for a date from the
 * static file's 12 monthly GREENFRAC rows, resident on the device, so a long
 * run's canopy follows the calendar without a host copy of the row.  table12
 * is 12 fp32 rows with leading dimension ld_tab (month m of column c at
 * table12[m*ld_tab + c]; fp32 for both precisions, as the file stores f4),
 * possibly offset by a range's first column; out_row is ncol elements of the
 * engine precision T, e.g. static_f + NMP_F_SHDFAC*ld (+ the range's first
 * column).  m0, m1 and w are the caller's: the two months whose mid-month values
 * bracket the date and the weight of the later one (noahmp-1_amd/vegclim.py
 * month_weights: t = 12*julian/yearlen - 0.5 in double, f = floor(t),
 * m0 = f mod 12, m1 = (m0 + 1) mod 12, w = t - f).
 * The operation order is part of this interface: per column c, in IEEE double,
 * each operation rounded once (no fused multiply-add),
 *   a = (double)table12[m0*ld_tab + c]      b = (double)table12[m1*ld_tab + c]
 *   u = 1.0 - w        (formed once on the host side of the call)
 *   r = (float)(u*a + w*b)                  (two rounded products, then one add)
 *   out_row[c] = (T)r
 * so the result is rounded once to fp32 and that fp32 value is widened to T:
 * an fp64 engine sees the value a host that interpolates in fp32 storage and
 * then converts gives it.  There are no special cases: w == 0, NaN, -0 and
 * subnormals go through the formula (vegclim.py shdfac_host restates it in
 * numpy, bit for bit).  One lane per column, one kernel enqueued on `stream`;
 * the call neither synchronises nor allocates; elements ncol.. of out_row and
 * every other row are untouched.  NMP_E_ARG, with nothing enqueued and the row
 * untouched, for a NULL engine, ncol < 0, ld_tab < ncol, ld_tab >= 2^29 (so
 * ncol above the limit too), m0 or m1 outside 0..11, w outside [0, 1) or NaN,
 * or a NULL table12 or out_row with ncol > 0; ncol == 0 is NMP_OK with nothing
 * enqueued. */
int nmp_static_monthly(nmp_engine* eng, int64_t ncol, int64_t ld_tab, const float* table12,
                       int m0, int m1, double w, void* out_row, void* stream);

/* Interval extremes (no counterpart in the reference, which writes no output):
 * the running maximum and minimum of per-column series over an output
 * interval, and the step of the interval that set each of them -- the day's
 * highest and lowest 2-m temperature, the peak runoff rate and when it fell.
 *
 * Series.  A series is one value per column per step, named by a pair
 * (kind, row): NMP_EXT_SRC_DIAG = row NMP_O_* of the step's NMP_NDIAG_OUT-row
 * flux block `diag` (a step at NMP_DIAG_OUT), NMP_EXT_SRC_FORCING = row NMP_A_*
 * of the step's NMP_NFORCING-row `forcing` block, NMP_EXT_SRC_STATE = row
 * NMP_S_* (0..55) of the `state` the step left.  `series` is a HOST array of
 * nseries pairs, series[2*s] = kind and series[2*s + 1] = row, 1 <= nseries <=
 * NMP_EXT_MAXSERIES; the three blocks share the leading dimension ld.
 *
 * Resident state, leading dimension ld_ext: `val`, 2*nseries x ld_ext of the
 * engine precision T, row 2*s the running maximum of series s and row 2*s + 1
 * its running minimum; `when`, int32 of the same shape, the 1-based number
 * within the interval of the step that set each of them.
 *
 * nmp_extremes_update: one kernel.  k >= 1 is the number of this step within
 * its interval.  Per column and series, with v the series' value, the rule is
 * part of this interface:
 *   k == 1:  max = min = v, both when = 1.  A value of any kind is taken, NaN
 *            included: no reset launch exists or is needed.
 *   k > 1:   the max takes v, and its when = k, iff (v > max) || (max != max && v == v);
 *            the min takes v, and its when = k, iff (v < min) || (min != min && v == v).
 * So the first occurrence wins a tie; -0 and +0 tie, and whichever came first
 * stays with its sign bit; NaN survives only while every value so far was NaN,
 * and its when is then 1.  Values are stored as loaded: no arithmetic, no
 * rounding.  diag may be NULL when no series has kind DIAG; the same holds for
 * forcing and for state.
 *
 * nmp_extremes_output: one kernel.  `stats` is a HOST array of nseries bit
 * masks of NMP_EXT_MAX, NMP_EXT_MIN, NMP_EXT_TMAX, NMP_EXT_TMIN.  It writes the
 * rows of `out` (leading dimension ld_out, engine precision) in series order
 * and within a series in bit order MAX, MIN, TMAX, TMIN, for the bits that are
 * set: a value row is val as stored; a time row is (T)((double)when * dt), one
 * rounded product and one conversion -- the seconds from the interval's start
 * to the end of the step that produced the extreme (dt: the step in seconds).
 * It changes neither val nor when.
 *
 * Both: device pointers, possibly offset by a range's first column; one lane
 * per column, enqueued on `stream`; the calls neither synchronise nor
 * allocate; elements ncol.. of every row, and rows not named, are untouched
 * (noahmp-1_amd/extremes.py update_host / output_host restate both in numpy,
 * bit for bit).  NMP_E_ARG, with nothing enqueued, for a NULL engine,
 * ncol < 0, ld, ld_ext or ld_out below ncol or at or above 2^29, nseries
 * outside 1..NMP_EXT_MAXSERIES, a kind outside the three, a row outside its
 * block, a stats mask of 0 or with a bit above NMP_EXT_TMIN, k < 1, dt not
 * finite or <= 0, a NULL series or stats, or -- with ncol > 0 -- a NULL val,
 * when or out or a NULL block that a named series needs; ncol == 0 with
 * otherwise valid arguments is NMP_OK with nothing enqueued. */
#define NMP_EXT_MAXSERIES 32
enum { NMP_EXT_SRC_DIAG = 0, NMP_EXT_SRC_FORCING = 1, NMP_EXT_SRC_STATE = 2 };
enum { NMP_EXT_MAX = 1, NMP_EXT_MIN = 2, NMP_EXT_TMAX = 4, NMP_EXT_TMIN = 8 };
int nmp_extremes_update(nmp_engine* eng, int64_t ncol, int64_t ld, int nseries,
                        const int32_t* series, const void* diag /* may be NULL */,
                        const void* forcing /* may be NULL */, const void* state /* may be NULL */,
                        int32_t k, void* val, int32_t* when, int64_t ld_ext, void* stream);
int nmp_extremes_output(nmp_engine* eng, int64_t ncol, int nseries, const int32_t* stats,
                        double dt, const void* val, const int32_t* when, int64_t ld_ext,
                        void* out, int64_t ld_out, void* stream);

/* Interval statistics (no counterpart in the reference, which writes no
 * output): over an output interval, the mean of a per-column series, or -- for
 * a series with a condition -- how long the condition held, the longest
 * unbroken spell of it and the value-seconds beyond its threshold: a day's
 * mean soil moisture, its frost hours, its longest wet spell, its growing
 * degree-days.
 *
 * Items.  An item is a series with either nothing or a condition attached.
 * The series is a (kind, row) pair as in "Interval extremes" (NMP_EXT_SRC_DIAG,
 * NMP_EXT_SRC_FORCING, NMP_EXT_SRC_STATE; the three blocks share the leading
 * dimension ld).  The condition is an operator NMP_IST_GT, _GE, _LT or _LE and
 * a threshold c; NMP_IST_NONE makes a mean item.  `items` is a HOST array of
 * four words per item: items[4*i] = kind, [4*i + 1] = row, [4*i + 2] = operator,
 * [4*i + 3] = the mask of the item's output rows, NMP_IST_MEAN for a mean item
 * and any of NMP_IST_DUR, NMP_IST_DEG, NMP_IST_SPELL for a conditioned one;
 * 1 <= nitems <= NMP_IST_MAXITEMS.  `thresholds` is a HOST array of nitems
 * doubles (a mean item's is not read).
 *
 * Resident state, leading dimension ld_st: `acc`, nitems x ld_st doubles in
 * both engine precisions, row i the running sum of item i; `cnt`, 3*nitems x
 * ld_st int32, row 3*i the steps the condition held (count), row 3*i + 1 the
 * current run, row 3*i + 2 the longest run.  A mean item never touches its
 * cnt rows.
 *
 * nmp_intstats_update: one kernel.  k >= 1 is the number of this step within
 * its interval.  Per column and item, with v the series' value as loaded (the
 * engine precision T) and cT the threshold rounded to T, the rule is part of
 * this interface:
 *   k == 1:  the old acc and cnt are not read: they count as +0.0 and 0.  No
 *            reset launch exists or is needed; stale or NaN contents are
 *            harmless.
 *   mean item:         acc = acc + (double)v, one double add per step.
 *   conditioned item:  h = v OP cT, compared in T: a NaN never holds, -0 and
 *            +0 compare equal.  If h: acc = acc + d with d = (double)v -
 *            (double)cT for GT and GE, d = (double)cT - (double)v for LT and
 *            LE; count += 1; run += 1; longest = max(longest, run).  Otherwise
 *            run = 0 and nothing else changes.
 * A store that would write the value already there may be skipped; at k == 1
 * every row of the item is written.  A NaN the sum forms itself (inf + -inf
 * in a mean) is the adder's default quiet NaN, sign bit set, on the device as
 * on an x86 host; a NaN operand travels quieted with its payload.  diag may be NULL when no item has kind
 * DIAG; the same holds for forcing and for state.
 *
 * nmp_intstats_output: one kernel.  k is the interval's step count, dt the
 * step in seconds.  It takes the same `items` and writes the rows of `out`
 * (leading dimension ld_out, engine precision) in item order and within an
 * item in bit order MEAN, DUR, DEG, SPELL, for the bits that are set:
 *   MEAN   (T)(acc / (double)k)       one IEEE double division, one conversion
 *   DUR    (T)((double)count * dt)    seconds the condition held
 *   DEG    (T)(acc * dt)              value-seconds beyond the threshold
 *   SPELL  (T)((double)longest * dt)  seconds of the longest unbroken spell
 * It changes neither acc nor cnt.  Only the operations listed are performed,
 * in the stated order, and nothing in them can be contracted.
 *
 * Both: device pointers, possibly offset by a range's first column; one lane
 * per column, enqueued on `stream`; the calls neither synchronise nor
 * allocate; elements ncol.. of every row, and rows not named, are untouched
 * (noahmp-1_amd/intstats.py update_host / output_host restate both in numpy,
 * bit for bit).  NMP_E_ARG, with nothing enqueued, first for a NULL engine,
 * ncol < 0, ld, ld_st or ld_out below ncol or at or above 2^29; then for
 * nitems outside 1..NMP_IST_MAXITEMS, a NULL items or thresholds, a kind
 * outside the three, a row outside its block, an operator outside the five, a
 * mask of 0 or with a bit above NMP_IST_SPELL, a mean item with another bit
 * than MEAN or a conditioned one with MEAN, a conditioned item's threshold
 * that is not finite, k < 1, dt not finite or <= 0; then ncol == 0 is NMP_OK
 * with nothing enqueued; then -- with ncol > 0 -- for a NULL acc or out, a
 * NULL cnt with a conditioned item, or a NULL block that a named item needs. */
#define NMP_IST_MAXITEMS 32
enum { NMP_IST_NONE = 0, NMP_IST_GT = 1, NMP_IST_GE = 2, NMP_IST_LT = 3, NMP_IST_LE = 4 };
enum { NMP_IST_MEAN = 1, NMP_IST_DUR = 2, NMP_IST_DEG = 4, NMP_IST_SPELL = 8 };
int nmp_intstats_update(nmp_engine* eng, int64_t ncol, int64_t ld, int nitems,
                        const int32_t* items, const double* thresholds,
                        const void* diag /* may be NULL */, const void* forcing /* may be NULL */,
                        const void* state /* may be NULL */, int32_t k, double* acc, int32_t* cnt,
                        int64_t ld_st, void* stream);
int nmp_intstats_output(nmp_engine* eng, int64_t ncol, int nitems, const int32_t* items,
                        int32_t k, double dt, const double* acc, const int32_t* cnt,
                        int64_t ld_st, void* out, int64_t ld_out, void* stream);

int nmp_run(nmp_engine* eng, int64_t ncol, int64_t ld, const float zsoil[4], float dt,
            float julian0, int32_t yearlen, int32_t nsteps, void* state, int32_t* isnow,
            const void* static_f, const int32_t* static_i, const void* forcing,
            int64_t forcing_stride, int32_t forcing_period, void* diag, int diag_level,
            int32_t* col_status, void* stream);

/* nmp_run with periodic output: every step s with (s+1) % out_every == 0
 * writes its diagnostics (diag_level) to slot ((s+1)/out_every - 1) % diag_slots
 * of the ring diag + slot*diag_stride (elements; >= the diag block size
 * x ld when more than one slot is written).  nmp_run is out_every = nsteps,
 * diag_slots = 1. */
int nmp_run_out(nmp_engine* eng, int64_t ncol, int64_t ld, const float zsoil[4], float dt,
                float julian0, int32_t yearlen, int32_t nsteps, void* state, int32_t* isnow,
                const void* static_f, const int32_t* static_i, const void* forcing,
                int64_t forcing_stride, int32_t forcing_period, void* diag, int diag_level,
                int32_t out_every, int32_t diag_slots, int64_t diag_stride, int32_t* col_status,
                void* stream);

/* Host-side converter: n byte-identical `noahmp_state_t` sequence records
 * (168 B each, core/module_noahmp_type.f90:10-42) -> host SoA float state
 * (ld >= n) + isnow, applying the unit/sign mapping of SURVEY.md 8b.
 * Fields the record lacks are left untouched.
 * PARITY-UNPINNED: no reference code reads or writes noahmp_state_t, so the
 * record's conventions are taken from its field comments alone
 * (core/module_noahmp_type.f90:18,33,41): snowwat is read as mm (kg m-2)
 * although the comment says kg m-3, zsnow as layer tops above ground, zwt as
 * height (+up).  Only the byte layout is tested (tests/test_abi_host.py). */
int nmp_state_from_aos(const void* records, int64_t n, int64_t ld, float* state, int32_t* isnow,
                       int32_t* static_i);

/* noahmp_sflx with the reference calling sequence (func.f90:66-91), for n
 * HOST records: the records are packed into the SoA layout, stepped on the
 * engine's GPU by the same kernel as nmp_step (all 58 outputs), and unpacked
 * in place; synchronous.  Replaces a loop of `call noahmp_sflx(...)` over n
 * columns (the per-column entry SURVEY 8b names nmp_sflx_column).
 *  - nsoil must be 4 and nsnow 3; dt, julian, yearlen and zsoil must be the
 *    same in every record of one call (they are launch-wide), else NMP_E_ARG;
 *    julian outside [0, yearlen] is NMP_E_CALENDAR.
 *  - FICEOLD is taken as the record carries it, like noahmp_sflx's
 *    intent(in) argument (the SoA nmp_step path derives it from SNICE/SNLIQ
 *    at step start instead, as the offline and WRF drivers compute it).
 *  - iloc, jloc, dx, dz8w, qc, pblh and iz0tlnd never enter the arithmetic
 *    (SURVEY H9); zlvl is intent(inout) but never modified, as in the reference.
 *  - status receives the column's NMP_ST_* bits (0 = the reference would not
 *    have called wrf_error_fatal / wrf_message). */
int nmp_sflx_columns(nmp_engine* eng, nmp_sflx_args* cols, int64_t n);
int nmp_sflx_column(nmp_engine* eng, nmp_sflx_args* col);

/* The reference's other public physics routines, batched: element i is one
 * `call frh2o(sltyp(i), FREE(i), TKELV(i), SMC(i), soilwat(i))`
 * (core/module_noahmp_func.f90:4494-4598; public at :6-8) or one
 * `call calhum(SFCTMP(i), SFCPRS(i), Q2SAT(i), DQSDT2(i))` (:3958-3984; a
 * module procedure, public by default).  Reals are the engine's precision;
 * frh2o reads LK_BEXP / LK_PSISAT / LK_SMCMAX of the soil type from the
 * engine's tables, as the reference reads its module arrays.  The device code
 * is the one noahmp_sflx inlines, so in the fp32 "ref" math policy the values
 * are the reference's bit for bit.
 *  - nmp_frh2o / nmp_calhum: device pointers, enqueued on `stream`.
 *  - nmp_frh2o_host / nmp_calhum_host: host arrays, synchronous (copy in,
 *    launch, copy out) -- the drop-in for the scalar Fortran calls (n = 1).
 *  - frh2o: col_status (may be NULL) is OR-ed with NMP_ST_FLERCH where the
 *    reference would call wrf_message (Flerchinger fallback, :4586-4590), and
 *    with NMP_ST_STOP for a soil type outside 1..NMP_MSLTYP (FREE = NaN).
 *  - calhum: q2sat or dqsdt2 may be NULL (not computed). */
int nmp_frh2o(nmp_engine* eng, int64_t n, const int32_t* sltyp, const void* tkelv,
              const void* smc, const void* soilwat, void* free_water, int32_t* col_status,
              void* stream);
int nmp_frh2o_host(nmp_engine* eng, int64_t n, const int32_t* sltyp, const void* tkelv,
                   const void* smc, const void* soilwat, void* free_water, int32_t* col_status);
int nmp_calhum(nmp_engine* eng, int64_t n, const void* sfctmp, const void* sfcprs, void* q2sat,
               void* dqsdt2, void* stream);
int nmp_calhum_host(nmp_engine* eng, int64_t n, const void* sfctmp, const void* sfcprs,
                    void* q2sat, void* dqsdt2);

/* Transcendental policy for fp32 engines: 0 = "ref", a bit-exact restatement of
 * the glibc float libm the reference is linked against (csrc/glibc_math.h;
 * default), 1 = ocml fp32 functions (faster, within a few ulp).  fp64 engines
 * always use ocml double.  Default can also be set with NMP_MATH=fast. */
int nmp_set_math(nmp_engine* eng, int mode);

/* Columns stepped per 64-lane wave: 8..64 (multiple of 8); 0 = 64 (default).
 * Fewer columns per wave spread a small column set over more, partly filled
 * waves; measured slower on config #2, kept as a tuning knob.
 * Results do not depend on it. */
int nmp_set_cols_per_wave(nmp_engine* eng, int cpw);

/* Kernel specialisation for the engine's physics options.  The kernel is
 * compiled for fixed option sets (case.nml's, and case.nml with opt_veg 2);
 * nmp_init picks the one equal to the engine's options, any other combination
 * runs the run-time-options kernel (set 0).  request: -1 = query only,
 * 0 = force the run-time-options kernel, 1 = pick the matching compiled set
 * (the default; env NMP_GENERIC_OPTIONS=1 makes nmp_init start at 0).
 * Returns the set in use (>= 0) or a negative NMP_E_* code.  Results do not
 * depend on it (DESIGN.md "Compile-time option sets"). */
int nmp_option_set(nmp_engine* eng, int request);

/* Occupancy instantiation of the step kernel.  The kernel is compiled twice
 * per option set: at full occupancy (4 waves/SIMD fp32, 2 fp64; spills) and
 * at half occupancy (2 fp32, 1 fp64; fewer or no spills).  NMP_LAUNCH_AUTO
 * (the default) picks the half-occupancy kernel for launches whose waves fit
 * in its slots (csrc/engine.hip small_launch), the full one otherwise;
 * NMP_LAUNCH_SMALL / NMP_LAUNCH_FULL force one for every launch, so a small
 * column set can be pushed through the kernel production sizes run (parity
 * tests of both instantiations).  Env NMP_LAUNCH_VARIANT=auto|small|full sets
 * the default at nmp_init.  Returns the variant in use, or NMP_E_ARG;
 * request -1 only queries.  Results do not depend on it.  The fp32 "fast"
 * math kernel has one instantiation (full) and ignores the setting. */
#define NMP_LAUNCH_AUTO 0
#define NMP_LAUNCH_SMALL 1
#define NMP_LAUNCH_FULL 2
int nmp_set_launch_variant(nmp_engine* eng, int variant);

int nmp_engine_info(const nmp_engine* eng, int* device, int* precision, nmp_options* opts);

/* sizeof of the ABI's records, for hosts that lay them out themselves (a
 * Fortran bind(C) type, a ctypes Structure) and check the layout at start-up:
 * which = NMP_TYPE_PARAMS | NMP_TYPE_OPTIONS | NMP_TYPE_SFLX_ARGS; -1 otherwise. */
#define NMP_TYPE_PARAMS 0
#define NMP_TYPE_OPTIONS 1
#define NMP_TYPE_SFLX_ARGS 2
int64_t nmp_type_size(int which);
void nmp_finalize(nmp_engine* eng);
const char* nmp_strerror(int code);
int nmp_abi_version(void);
/* Hash of the sources and flags this library was compiled from
 * (noahmp-1_amd/build.py source_hash()); the Python loader refuses a library
 * whose hash differs from the sources beside it, so a stale .so never runs. */
const char* nmp_build_hash(void);

#ifdef __cplusplus
}
#endif
#endif /* NOAHMP_ENGINE_H */
