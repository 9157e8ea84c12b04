// Forcing on its own grid: an LDASIN file stored on a coarse rectilinear
// source grid is interpolated to the engine's columns here
// (nmp_ldasin_regrid), and optionally corrected for the elevation difference
// between the source grid and the model terrain (nmp_ldasin_downscale), so the
// host uploads the coarse file's bytes as stored and nothing per column.
//
// Both kernels take one lane per column and write the fp32 LDASIN block
// (NMP_L_* rows, leading dimension ld) that nmp_forcing_from_ldasin[_geo]
// reads.  Every operation is one IEEE operation in the order the header
// documents (no contraction: the build keeps -ffp-contract=off), which the
// numpy restatement in noahmp-1_amd/regrid.py follows operation for operation.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "engine_impl.h"

namespace nmp {

// Column c has four source entries k = 0..3: source point corner[k*ld + c]
// (< 0: a masked source point, skipped and never loaded) with weight
// weight[k*ld + c].  The corner and weight loads are coalesced; the 8 x 4
// gathered words are loaded before any is used, so they are in flight
// together (the source grid is small: it stays in L2 / the Infinity Cache).
__global__ __launch_bounds__(256) void ldasin_regrid_kernel(int64_t ncol, int64_t ld, int64_t npts,
                                                            const uint32_t* __restrict__ grid_be,
                                                            const int32_t* __restrict__ corner,
                                                            const double* __restrict__ weight,
                                                            uint32_t nearest_mask,
                                                            float* __restrict__ block) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= ncol) return;
  int32_t p[4];
  double w[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    p[k] = corner[k * ld + c];
    w[k] = weight[k * ld + c];
  }
  bool outside = false;
  // the nearest entry's source point: the valid entry of largest weight, ties
  // to the lowest k (-1: the column has no valid entry)
  int32_t pn = -1;
  double wbest = 0.0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    outside = outside || (int64_t)p[k] >= npts;
    if (p[k] >= 0 && (pn < 0 || w[k] > wbest)) {
      pn = p[k];
      wbest = w[k];
    }
  }
  if (pn < 0 || outside) {  // no source point, or one outside the grid: NaN, never an out-of-bounds load
#pragma unroll
    for (int v = 0; v < NMP_L_COSZ; ++v) block[v * ld + c] = __int_as_float(0x7fc00000);
    return;
  }
  // every gathered word first (a nearest variable needs one, the others
  // their valid entries'), then the arithmetic
  uint32_t word[NMP_L_COSZ][4];
#pragma unroll
  for (int v = 0; v < NMP_L_COSZ; ++v) {
    const uint32_t* gv = grid_be + (int64_t)v * npts;
    if ((nearest_mask >> v) & 1u) {
      word[v][0] = __builtin_bswap32(gv[pn]);
      word[v][1] = word[v][2] = word[v][3] = 0u;
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) word[v][k] = p[k] >= 0 ? __builtin_bswap32(gv[p[k]]) : 0u;
    }
  }
#pragma unroll
  for (int v = 0; v < NMP_L_COSZ; ++v) {
    if ((nearest_mask >> v) & 1u) {
      block[v * ld + c] = __uint_as_float(word[v][0]);  // the word's bits, unchanged
    } else {
      double x = 0.0;
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (p[k] >= 0) x = x + (double)__uint_as_float(word[v][k]) * w[k];
      block[v * ld + c] = (float)x;
    }
  }
}

// Elevation (lapse-rate) downscaling of a block in place: temperature by the
// lapse rate, pressure hypsometrically at the layer's mean temperature,
// specific humidity at constant relative humidity (Magnus form) and longwave
// by the fourth power of the temperature ratio.  G and RD are the reference's
// GRAV and RAIR (core/module_noahmp_const.f90).
__device__ __forceinline__ double magnus_arg(double t) {
  return (17.67 * (t - 273.15)) / (t - 29.65);
}

__global__ __launch_bounds__(256) void ldasin_downscale_kernel(int64_t ncol, int64_t ld,
                                                               const float* __restrict__ dz,
                                                               double lapse,
                                                               float* __restrict__ block) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= ncol) return;
  const double G = 9.80616, RD = 287.04;
  float* b = block + c;
  const double d = (double)dz[c];
  const double t0 = (double)b[NMP_L_T2D * ld];
  const double q0 = (double)b[NMP_L_Q2D * ld];
  const double p0 = (double)b[NMP_L_PSFC * ld];
  const double lw0 = (double)b[NMP_L_LWDOWN * ld];
  const double t1 = t0 - lapse * d;
  const double tm = 0.5 * (t0 + t1);
  const double p1 = p0 * exp(-(G * d) / (RD * tm));
  const double q1 = (q0 * exp(magnus_arg(t1) - magnus_arg(t0))) * (p0 / p1);
  const double r = t1 / t0;
  const double lw1 = lw0 * ((r * r) * (r * r));
  b[NMP_L_T2D * ld] = (float)t1;
  b[NMP_L_Q2D * ld] = (float)q1;
  b[NMP_L_PSFC * ld] = (float)p1;
  b[NMP_L_LWDOWN * ld] = (float)lw1;
}

}  // namespace nmp

extern "C" {

int nmp_ldasin_regrid(nmp_engine* eng, int64_t ncol, int64_t ld, int64_t npts,
                      const void* grid_be, const int32_t* corner, const double* weight,
                      uint32_t nearest_mask, float* ldasin, void* stream) {
  if (!eng || ncol < 0 || nmp::bad_ld(ld, ncol) || npts < 1 || npts >= nmp::kMaxColumns)
    return NMP_E_ARG;
  if (ncol == 0) return NMP_OK;
  if (!grid_be || !corner || !weight || !ldasin) return NMP_E_ARG;
  if (int rc = nmp::ensure_device(eng->device)) return rc;
  return nmp::launch_cols(ncol, stream, nmp::ldasin_regrid_kernel, ncol, ld, npts, grid_be, corner,
                          weight, nearest_mask, ldasin);
}

int nmp_ldasin_downscale(nmp_engine* eng, int64_t ncol, int64_t ld, const float* dz, double lapse,
                         float* ldasin, void* stream) {
  if (!eng || ncol < 0 || nmp::bad_ld(ld, ncol)) return NMP_E_ARG;
  if (ncol == 0) return NMP_OK;
  if (!dz || !ldasin) return NMP_E_ARG;
  if (int rc = nmp::ensure_device(eng->device)) return rc;
  return nmp::launch_cols(ncol, stream, nmp::ldasin_downscale_kernel, ncol, ld, dz, lapse, ldasin);
}

}  // extern "C"
