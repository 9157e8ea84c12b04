// State output (nmp_state_output): the land state of an output step as output
// rows -- soil moisture and temperature, the snow pack, canopy water, LAI, the
// water table, the column's water storage, soil saturation and root-zone
// moisture, the carbon pools -- formed from the state block next to the output
// step's fluxes.  The reference writes no output at all; the groups and their
// arithmetic are this engine's (include/noahmp_engine.h "State output").
//
// One lane per column, field-major SoA like every other array.  `groups` is a
// kernel argument, so every `groups & bit` test is a scalar branch: an
// unselected group costs neither a load nor a store, and the row counter k is
// uniform.  Every operation is one IEEE operation in the order the header
// documents (the build keeps -ffp-contract=off), which the numpy restatement
// in noahmp-1_amd/stateout.py follows operation for operation.
//
// The two per-type table values (soil[].smcmax, veg[].nroot) are staged into
// LDS once per workgroup, 57 words, and each lane reads its own type's entry
// from there; a launch that selects neither SOILSAT nor ROOT_M skips the
// staging and its barrier.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "col_math.h"
#include "engine_impl.h"

namespace nmp {

namespace {
constexpr uint32_t xbit(int g) { return 1u << g; }
// groups that read ZSNSO's soil rows and ISNOW for the soil layers' thickness
constexpr uint32_t kNeedDz = xbit(NMP_X_TWS) | xbit(NMP_X_SOILSAT) | xbit(NMP_X_ROOT_M);
constexpr uint32_t kNeedSmc = xbit(NMP_X_SOIL_M) | kNeedDz;
constexpr uint32_t kNeedIsnow = kNeedDz | xbit(NMP_X_ISNOW) | xbit(NMP_X_SNOWLIQ) |
                                xbit(NMP_X_SNOW_T) | xbit(NMP_X_SNOW_Z) | xbit(NMP_X_SNOWT_AVG);
constexpr uint32_t kNeedTable = xbit(NMP_X_SOILSAT) | xbit(NMP_X_ROOT_M);
}  // namespace

template <class T>
__global__ __launch_bounds__(256) void state_output_kernel(int64_t ncol, int64_t ld,
                                                           const T* __restrict__ state,
                                                           const int32_t* __restrict__ isnow,
                                                           const int32_t* __restrict__ static_i,
                                                           const DevParams* __restrict__ p,
                                                           uint32_t groups, T fill,
                                                           T* __restrict__ out, int64_t ld_out) {
  __shared__ float s_smcmax[NMP_MSLTYP];
  __shared__ int32_t s_nroot[NMP_MLUTYP];
  if (groups & kNeedTable) {  // uniform: every lane of the workgroup reaches the barrier
    const int t = threadIdx.x;
    if (t < NMP_MSLTYP) s_smcmax[t] = p->soil[t].smcmax;
    if (t >= 64 && t < 64 + NMP_MLUTYP) s_nroot[t - 64] = p->veg[t - 64].nroot;
    __syncthreads();
  }
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= ncol) return;
  const T* s = state + c;
  T* o = out + c;
  int k = 0;  // next output row (uniform)
  const T qnan = sizeof(T) == 4 ? (T)__int_as_float(0x7fc00000)
                                : (T)__longlong_as_double(0x7ff8000000000000LL);

  const int isn = (groups & kNeedIsnow) ? isnow[c] : 0;
  T smc[NMP_NSOIL], dz[NMP_NSOIL];
  if (groups & kNeedSmc) {
#pragma unroll
    for (int i = 0; i < NMP_NSOIL; ++i) smc[i] = s[(NMP_S_SMC + i) * ld];
  }
  if (groups & kNeedDz) {
    // ZSNSO's soil rows are C index 2..6; the first, the snow pack's bottom,
    // is used (and loaded) only under snow
    T z[NMP_NSOIL + 1];
    z[0] = isn == 0 ? (T)0 : s[(NMP_S_ZSNSO + 2) * ld];
#pragma unroll
    for (int i = 1; i <= NMP_NSOIL; ++i) z[i] = s[(NMP_S_ZSNSO + 2 + i) * ld];
    soil_thickness(z, isn, dz);
  }

  if (groups & xbit(NMP_X_SOIL_M)) {
#pragma unroll
    for (int i = 0; i < NMP_NSOIL; ++i) o[(k + i) * ld_out] = smc[i];
    k += NMP_NSOIL;
  }
  if (groups & xbit(NMP_X_SOIL_W)) {
#pragma unroll
    for (int i = 0; i < NMP_NSOIL; ++i) o[(k + i) * ld_out] = s[(NMP_S_SH2O + i) * ld];
    k += NMP_NSOIL;
  }
  if (groups & xbit(NMP_X_SOIL_T)) {
#pragma unroll
    for (int i = 0; i < NMP_NSOIL; ++i) o[(k + i) * ld_out] = s[(NMP_S_STC + NMP_NSNOW + i) * ld];
    k += NMP_NSOIL;
  }
  constexpr int kScalar[8] = {NMP_S_SNEQV, NMP_S_SNOWH, NMP_S_TG,  NMP_S_TV,
                              NMP_S_LAI,   NMP_S_SAI,   NMP_S_ZWT, NMP_S_WA};
#pragma unroll
  for (int g = 0; g < 8; ++g)
    if (groups & xbit(NMP_X_SNEQV + g)) {
      o[k * ld_out] = s[kScalar[g] * ld];
      k += 1;
    }
  if (groups & xbit(NMP_X_CANWAT)) {
    o[k * ld_out] = s[NMP_S_CANLIQ * ld] + s[NMP_S_CANICE * ld];
    k += 1;
  }
  if (groups & xbit(NMP_X_ISNOW)) {
    o[k * ld_out] = (T)isn;
    k += 1;
  }
  if (groups & xbit(NMP_X_SNOWLIQ)) {
    T x = (T)0;
#pragma unroll
    for (int j = 0; j < NMP_NSNOW; ++j) {
      const T v = s[(NMP_S_SNLIQ + j) * ld];
      if (j >= isn + NMP_NSNOW) x = x + v;
    }
    o[k * ld_out] = x;
    k += 1;
  }
  if (groups & xbit(NMP_X_TWS)) {
    T w = (T)0;
    if (static_i[NMP_I_IST * ld + c] == 1)
      w = water_storage(s[NMP_S_CANLIQ * ld], s[NMP_S_CANICE * ld], s[NMP_S_SNEQV * ld],
                        s[NMP_S_WA * ld], smc, dz);
    o[k * ld_out] = w;
    k += 1;
  }
  if (groups & xbit(NMP_X_SOILSAT)) {
    const int st = static_i[NMP_I_SOILTYP * ld + c];
    T r = qnan;
    if (st >= 1 && st <= NMP_MSLTYP) {  // a type outside the table: NaN, never an out-of-bounds load
      const double smcmax = (double)s_smcmax[st - 1];
      double num = 0.0, den = 0.0;
#pragma unroll
      for (int i = 0; i < NMP_NSOIL; ++i) {
        num = num + (double)smc[i] * (double)dz[i];
        den = den + smcmax * (double)dz[i];
      }
      r = (T)(num / den);
    }
    o[k * ld_out] = r;
    k += 1;
  }
  if (groups & xbit(NMP_X_ROOT_M)) {
    const int vt = static_i[NMP_I_VEGTYP * ld + c];
    T r = qnan;
    if (vt >= 1 && vt <= NMP_MLUTYP) {
      const int nroot = s_nroot[vt - 1];
      double num = 0.0, den = 0.0;
#pragma unroll
      for (int i = 0; i < NMP_NSOIL; ++i)
        if (i + 1 <= nroot) {
          num = num + (double)smc[i] * (double)dz[i];
          den = den + (double)dz[i];
        }
      r = nroot < 1 ? (T)0 : (T)(num / den);
    }
    o[k * ld_out] = r;
    k += 1;
  }
  if (groups & xbit(NMP_X_CARBON)) {
#pragma unroll
    for (int i = 0; i < 6; ++i) o[(k + i) * ld_out] = s[(NMP_S_LFMASS + i) * ld];
    k += 6;
  }
  if (groups & xbit(NMP_X_SNOW_T)) {
#pragma unroll
    for (int j = 0; j < NMP_NSNOW; ++j) {
      const T v = s[(NMP_S_STC + j) * ld];
      o[(k + j) * ld_out] = j >= isn + NMP_NSNOW ? v : fill;
    }
    k += NMP_NSNOW;
  }
  if (groups & xbit(NMP_X_SNOW_Z)) {
    T z[NMP_NSNOW];
#pragma unroll
    for (int j = 0; j < NMP_NSNOW; ++j) z[j] = s[(NMP_S_ZSNSO + j) * ld];
#pragma unroll
    for (int j = 0; j < NMP_NSNOW; ++j) {
      T v = fill;
      if (j == isn + NMP_NSNOW)
        v = -z[j];
      else if (j > isn + NMP_NSNOW)
        v = z[j > 0 ? j - 1 : 0] - z[j];
      o[(k + j) * ld_out] = v;
    }
    k += NMP_NSNOW;
  }
  if (groups & xbit(NMP_X_SNOWT_AVG)) {
    double num = 0.0, den = 0.0;
#pragma unroll
    for (int j = 0; j < NMP_NSNOW; ++j) {
      const T ice = s[(NMP_S_SNICE + j) * ld], liq = s[(NMP_S_SNLIQ + j) * ld];
      const T tk = s[(NMP_S_STC + j) * ld];
      if (j >= isn + NMP_NSNOW) {
        const double m = (double)(ice + liq);
        num = num + m * (double)tk;
        den = den + m;
      }
    }
    o[k * ld_out] = (isn == 0 || den == 0.0) ? fill : (T)(num / den);
    k += 1;
  }
}

}  // namespace nmp

extern "C" {

int nmp_state_output(nmp_engine* eng, int64_t ncol, int64_t ld, const void* state,
                     const int32_t* isnow, const int32_t* static_i, uint32_t groups,
                     double fill, void* out, int64_t ld_out, void* stream) {
  if (!eng || ncol < 0 || nmp::bad_ld(ld, ncol) || nmp::bad_ld(ld_out, ncol) || groups == 0 ||
      (groups >> NMP_NXGROUP) != 0)
    return NMP_E_ARG;
  if (ncol == 0) return NMP_OK;
  if (!state || !isnow || !static_i || !out) return NMP_E_ARG;
  if (int rc = nmp::ensure_device(eng->device)) return rc;
  return nmp::launch_cols(eng->precision, ncol, stream, nmp::state_output_kernel<float>,
                          nmp::state_output_kernel<double>, ncol, ld, state, isnow, static_i,
                          eng->dparams, groups, fill, out, ld_out);
}

}  // extern "C"
