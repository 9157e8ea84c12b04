// Accumulated output (nmp_accumulate / nmp_water_storage / nmp_accum_finish):
// the interval totals and means an offline run writes beside the output
// step's own fluxes, and the water budget's closure over the interval.
//
// The reference forms the column's water storage before and after a step and
// the step's residual ERRWAT and then drops them
// (core/module_noahmp_func.f90:339-344, :723-731); it has no accumulators (its
// driver stops after the namelist).  These kernels carry both
// across steps.  They are bandwidth-bound kernels of their own, enqueued on
// the step's stream right after it; the step kernel is not touched.
//
// One lane per column, field-major SoA with leading dimension ld like every
// other array.  The accumulators are double for both engine precisions and
// every operation is a fixed sequence of IEEE operations (the build has
// -ffp-contract=off), so a host reproduces every bit
// (tests/test_gpu_accum.py restates them in numpy).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "col_math.h"
#include "engine_impl.h"

namespace nmp {

// acc[f] = acc[f] + (double)v * (double)dt for the 16 NMP_O_* rows of the
// step's diagnostics and the step's precipitation rate.  In fp32 the product
// of two floats is exact in double; in fp64 it is one rounded product.  diag
// and forcing are read once: nontemporal loads keep them out of the way of
// the accumulators, which the next step's call reads again.
template <class T>
__global__ __launch_bounds__(256) void accumulate_kernel(int64_t ncol, int64_t ld, double dt,
                                                         const T* __restrict__ diag,
                                                         const T* __restrict__ forcing,
                                                         double* __restrict__ acc) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= ncol) return;
  T v[NMP_NACC];
#pragma unroll
  for (int f = 0; f < NMP_NDIAG_OUT; ++f) v[f] = __builtin_nontemporal_load(diag + f * ld + c);
  v[NMP_ACC_PRCP] = __builtin_nontemporal_load(forcing + NMP_A_PRCP * ld + c);
#pragma unroll
  for (int f = 0; f < NMP_NACC; ++f) {
    double* a = acc + f * ld + c;
    *a = *a + (double)v[f] * dt;
  }
}

// The reference's BEG_WB / END_WB in engine precision (col_math.h
// water_storage): canopy water and ice, snow water equivalent, aquifer water,
// then the four soil layers' total water over their thicknesses.  Columns
// that are not soil (IST != 1) get 0, as the reference sets ERRWAT = 0 for
// them (func.f90:729-730).
template <class T>
__global__ __launch_bounds__(256) void water_storage_kernel(int64_t ncol, int64_t ld,
                                                            const T* __restrict__ state,
                                                            const int32_t* __restrict__ isnow,
                                                            const int32_t* __restrict__ static_i,
                                                            T* __restrict__ storage) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= ncol) return;
  if (static_i[NMP_I_IST * ld + c] != 1) {
    storage[c] = (T)0;
    return;
  }
  const T* s = state + c;
  const int isn = isnow[c];
  const T canliq = s[NMP_S_CANLIQ * ld], canice = s[NMP_S_CANICE * ld];
  const T sneqv = s[NMP_S_SNEQV * ld], wa = s[NMP_S_WA * ld];
  T z[NMP_NSOIL + 1], smc[NMP_NSOIL], dz[NMP_NSOIL];
  // ZSNSO's soil rows are C index 2..6; the first, the snow pack's bottom, is
  // used (and loaded) only under snow
  z[0] = isn == 0 ? (T)0 : s[(NMP_S_ZSNSO + 2) * ld];
#pragma unroll
  for (int i = 0; i < NMP_NSOIL; ++i) {
    z[i + 1] = s[(NMP_S_ZSNSO + 3 + i) * ld];
    smc[i] = s[(NMP_S_SMC + i) * ld];
  }
  soil_thickness(z, isn, dz);
  storage[c] = water_storage(canliq, canice, sneqv, wa, smc, dz);
}

// The interval's NMP_B_* block from the accumulators: time means of the
// energy fluxes and the surface temperatures / albedo, totals (mm) of the
// water fluxes, the storage change and the budget's residual -- the
// reference's ERRWAT expression (func.f90:728) summed over the interval, in
// double.  The column's accumulators are then zeroed and the interval's end
// storage becomes the next one's beginning, so no second launch starts the
// next interval.
template <class T>
__global__ __launch_bounds__(256) void accum_finish_kernel(int64_t ncol, int64_t ld, double span_s,
                                                           double* __restrict__ acc,
                                                           const T* __restrict__ stor_end,
                                                           T* __restrict__ stor_beg,
                                                           T* __restrict__ out) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= ncol) return;
  constexpr int kMean[11] = {NMP_ACC_FSA,   NMP_ACC_FSR,  NMP_ACC_FIRA, NMP_ACC_FSH,
                             NMP_ACC_SSOIL, NMP_ACC_FCEV, NMP_ACC_FGEV, NMP_ACC_FCTR,
                             NMP_ACC_TRAD,  NMP_ACC_T2M,  NMP_ACC_ALBEDO};
  double a[NMP_NACC];
#pragma unroll
  for (int f = 0; f < NMP_NACC; ++f) a[f] = acc[f * ld + c];
  T* o = out + c;
#pragma unroll
  for (int i = 0; i < 11; ++i) o[(NMP_B_FSA_MEAN + i) * ld] = (T)(a[kMean[i]] / span_s);
  const double p = a[NMP_ACC_PRCP], ecan = a[NMP_ACC_ECAN], etran = a[NMP_ACC_ETRAN];
  const double edir = a[NMP_ACC_EDIR], runsrf = a[NMP_ACC_RUNSRF], runsub = a[NMP_ACC_RUNSUB];
  o[NMP_B_ACCPRCP * ld] = (T)p;
  o[NMP_B_ACCECAN * ld] = (T)ecan;
  o[NMP_B_ACCETRAN * ld] = (T)etran;
  o[NMP_B_ACCEDIR * ld] = (T)edir;
  o[NMP_B_SFCRNOFF * ld] = (T)runsrf;
  o[NMP_B_UGDRNOFF * ld] = (T)runsub;
  const T end = stor_end[c];
  const double d = (double)end - (double)stor_beg[c];
  o[NMP_B_DSTOR * ld] = (T)d;
  o[NMP_B_WBRES * ld] = (T)(d - (((((p - ecan) - etran) - edir) - runsrf) - runsub));
#pragma unroll
  for (int f = 0; f < NMP_NACC; ++f) acc[f * ld + c] = 0.0;
  stor_beg[c] = end;
}

}  // namespace nmp

extern "C" {

int nmp_accumulate(nmp_engine* eng, int64_t ncol, int64_t ld, float dt, const void* diag,
                   const void* forcing, double* acc, void* stream) {
  if (!eng || ncol < 0 || nmp::bad_ld(ld, ncol)) return NMP_E_ARG;
  if (ncol == 0) return NMP_OK;
  if (!diag || !forcing || !acc) return NMP_E_ARG;
  if (int rc = nmp::ensure_device(eng->device)) return rc;
  return nmp::launch_cols(eng->precision, ncol, stream, nmp::accumulate_kernel<float>,
                          nmp::accumulate_kernel<double>, ncol, ld, dt, diag, forcing, acc);
}

int nmp_water_storage(nmp_engine* eng, int64_t ncol, int64_t ld, const void* state,
                      const int32_t* isnow, const int32_t* static_i, void* storage, void* stream) {
  if (!eng || ncol < 0 || nmp::bad_ld(ld, ncol)) return NMP_E_ARG;
  if (ncol == 0) return NMP_OK;
  if (!state || !isnow || !static_i || !storage) return NMP_E_ARG;
  if (int rc = nmp::ensure_device(eng->device)) return rc;
  return nmp::launch_cols(eng->precision, ncol, stream, nmp::water_storage_kernel<float>,
                          nmp::water_storage_kernel<double>, ncol, ld, state, isnow, static_i,
                          storage);
}

int nmp_accum_finish(nmp_engine* eng, int64_t ncol, int64_t ld, double span_s, double* acc,
                     const void* stor_end, void* stor_beg, void* out, void* stream) {
  // !(span_s > 0) also refuses NaN
  if (!eng || ncol < 0 || nmp::bad_ld(ld, ncol) || !(span_s > 0.0)) return NMP_E_ARG;
  if (ncol == 0) return NMP_OK;
  if (!acc || !stor_end || !stor_beg || !out) return NMP_E_ARG;
  if (int rc = nmp::ensure_device(eng->device)) return rc;
  return nmp::launch_cols(eng->precision, ncol, stream, nmp::accum_finish_kernel<float>,
                          nmp::accum_finish_kernel<double>, ncol, ld, span_s, acc, stor_end,
                          stor_beg, out);
}

}  // extern "C"
