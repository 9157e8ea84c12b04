// The arithmetic that several column kernels share and whose every bit is
// promised to a host restatement (the build keeps -ffp-contract=off: each
// operation below is one IEEE operation).  Every function takes values the
// caller has loaded -- its own load flavour and order -- and the operation
// order is stated here once; include/noahmp_engine.h states it for callers.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "noahmp_engine.h"

namespace nmp {

// ---- the column's water storage ---------------------------------------------
// The soil layers' thickness DZSNSO (func.f90:322-328).  z: ZSNSO's five soil
// rows, C index 2..6 (Fortran layer 0..4, the layer bottoms below the snow
// surface).  Soil layer iz = 1..4 has thickness z[iz - 1] - z[iz], but -z[iz]
// where it is the column's top layer (iz == ISNOW + 1).
template <class T>
__device__ __forceinline__ void soil_thickness(const T (&z)[NMP_NSOIL + 1], int isnow,
                                               T (&dz)[NMP_NSOIL]) {
#pragma unroll
  for (int iz = 1; iz <= NMP_NSOIL; ++iz) dz[iz - 1] = iz == isnow + 1 ? -z[iz] : z[iz - 1] - z[iz];
}

// The reference's BEG_WB / END_WB (func.f90:339-344, :723-727) in its
// operation order: ((CANLIQ + CANICE) + SNEQV) + WA, then, layer by layer from
// the top, + (SMC dz) 1000.  (Columns that are not soil, IST != 1, hold 0: the
// caller's test.)
template <class T>
__device__ __forceinline__ T water_storage(T canliq, T canice, T sneqv, T wa,
                                           const T (&smc)[NMP_NSOIL], const T (&dz)[NMP_NSOIL]) {
  T w = ((canliq + canice) + sneqv) + wa;
#pragma unroll
  for (int i = 0; i < NMP_NSOIL; ++i) w = w + (smc[i] * dz[i]) * (T)1000;
  return w;
}

// ---- forcing ------------------------------------------------------------------
constexpr double kPi = 3.141592653589793;

// COSZ of a column from its geometry (sin lat, cos lat, lon) and a time's solar
// terms, timeman.cosz's expression and operation order in double, rounded once
// to fp32: sin_lat sin_decl + (cos_lat cos_decl) cos((ha0 + lon) - pi).
__device__ __forceinline__ float cosz_geo(double sin_lat, double cos_lat, double lon,
                                          double sin_decl, double cos_decl, double ha0) {
  const double ha = (ha0 + lon) - kPi;
  return (float)(sin_lat * sin_decl + (cos_lat * cos_decl) * cos(ha));
}

// The 12 noahmp_sflx forcing fields of column o[0] (rows ld apart) from the 8
// LDASIN file variables r (NMP_L_* order, fp32) and COSZ, as the host reader
// forms them (ncio.py LdasinForcing): SFCPRS = PSFC = the file's PSFC,
// CO2AIR = 395e-6 PSFC and O2AIR = 0.209 PSFC as one IEEE double product of
// the fp32 pressure rounded once to fp32, every field then widened to T.
template <class T>
__device__ __forceinline__ void store_forcing(T* __restrict__ o, int64_t ld,
                                              const float (&r)[NMP_L_COSZ], float cosz) {
  const float psfc = r[NMP_L_PSFC];
  o[NMP_A_SFCTMP * ld] = (T)r[NMP_L_T2D];
  o[NMP_A_SFCPRS * ld] = (T)psfc;
  o[NMP_A_PSFC * ld] = (T)psfc;
  o[NMP_A_UU * ld] = (T)r[NMP_L_U2D];
  o[NMP_A_VV * ld] = (T)r[NMP_L_V2D];
  o[NMP_A_Q2 * ld] = (T)r[NMP_L_Q2D];
  o[NMP_A_SOLDN * ld] = (T)r[NMP_L_SWDOWN];
  o[NMP_A_LWDN * ld] = (T)r[NMP_L_LWDOWN];
  o[NMP_A_PRCP * ld] = (T)r[NMP_L_RAINRATE];
  o[NMP_A_COSZ * ld] = (T)cosz;
  o[NMP_A_CO2AIR * ld] = (T)(float)(395.0e-6 * (double)psfc);
  o[NMP_A_O2AIR * ld] = (T)(float)(0.209 * (double)psfc);
}

// ---- the fixed summation tree of the two-pass reductions ------------------------
// Pass 1: one wavefront per chunk of kWave x kPerLane = 256 entries, lane l
// adding its entries l, l + 64, l + 128, l + 192 from +0.0 in that order (the
// caller's loop: it knows which entries are left out), then wave_sum; pass 2:
// wave_ordered_sum over the chunk partials.
constexpr int kWave = 64;
constexpr int kPerLane = 4;
constexpr int kWavesPerBlock = 4;

// Wave-uniform: no lane of the chunk leaves an entry out, so the chunk takes
// the instantiation whose loads and adds carry no predicate -- the same
// operations in the same order; with predicates the compiler branches around
// every load and waits for each (measured 2.3x the time in fp32).
__device__ __forceinline__ bool chunk_full(const bool (&ok)[kPerLane]) {
  return __all(ok[0] && ok[1] && ok[2] && ok[3]);
}

// The xor butterfly over a full wave: x = x + shfl_xor(x, s) for s = 32, 16,
// 8, 4, 2, 1; every lane ends with the same sum.
__device__ __forceinline__ double wave_sum(double x) {
#pragma unroll
  for (int s = kWave / 2; s >= 1; s >>= 1) x = x + __shfl_xor(x, s, kWave);
  return x;
}

__device__ __forceinline__ int64_t shfl_xor_i64(int64_t x, int s) {
  return (int64_t)__shfl_xor((long long)x, s, kWave);
}

// From +0.0, p[k0], p[k0 + 1], ... p[k1 - 1] added in that order, by one
// wavefront: the lanes load 64 consecutive partials at once, the next 64 while
// these are added, and every lane adds them in order from the lanes' registers
// -- a sequential sum, bit for bit, without a memory latency per batch (a full
// batch is unrolled, the last one loops).  Every lane returns the sum.
__device__ __forceinline__ double wave_ordered_sum(const double* __restrict__ p, int64_t k0,
                                                   int64_t k1, int lane) {
  double sum = 0.0;
  double v = k0 + lane < k1 ? p[k0 + lane] : 0.0;
  for (int64_t k = k0; k < k1; k += kWave) {
    const double next = k + kWave + lane < k1 ? p[k + kWave + lane] : 0.0;
    // lane i's partial to every lane (i is uniform: two v_readlane_b32)
    const int lo = __double2loint(v), hi = __double2hiint(v);
    if (k1 - k >= kWave) {
#pragma unroll
      for (int i = 0; i < kWave; ++i)
        sum = sum + __hiloint2double(__builtin_amdgcn_readlane(hi, i),
                                     __builtin_amdgcn_readlane(lo, i));
    } else {
      const int m = (int)(k1 - k);
      for (int i = 0; i < m; ++i)
        sum = sum + __hiloint2double(__builtin_amdgcn_readlane(hi, i),
                                     __builtin_amdgcn_readlane(lo, i));
    }
    v = next;
  }
  return sum;
}

}  // namespace nmp
