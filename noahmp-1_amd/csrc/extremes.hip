// Interval extremes (nmp_extremes_update / nmp_extremes_output): the running
// maximum and minimum of up to NMP_EXT_MAXSERIES per-column series over an
// output interval, and the step of the interval that set each of them.  The
// reference writes no output at all; the series, the rule and the rows are this
// engine's (include/noahmp_engine.h "Interval extremes").
//
// Two bandwidth-bound kernels of their own, enqueued on the step's stream right
// after it; the step kernel is not touched.  One lane per column, field-major
// SoA like every other array.  The series table (and the output's stat masks)
// is a kernel argument passed by value, so a series' kind, its row and every
// row base are wave-uniform: the loop over the series is a scalar loop around
// coalesced row accesses.  diag and forcing rows are read once (nontemporal
// loads keep them out of the way of val / when, which the next step's call
// reads again); state rows, val and when take plain accesses.
//
// No arithmetic touches a value: it is compared and stored as loaded, so a host
// restates every bit (noahmp-1_amd/extremes.py).  The only arithmetic is the
// time rows' one rounded double product and one conversion.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "engine_impl.h"

namespace nmp {

namespace {

// by-value kernel argument: word s is kind << 8 | row of series s (update) or
// the stat mask of series s (output)
struct ExtTable {
  int32_t w[NMP_EXT_MAXSERIES];
};

}  // namespace

template <class T>
__global__ __launch_bounds__(256) void extremes_update_kernel(
    int64_t ncol, int64_t ld, int nseries, ExtTable tab, const T* __restrict__ diag,
    const T* __restrict__ forcing, const T* __restrict__ state, int32_t k, T* __restrict__ val,
    int32_t* __restrict__ when, int64_t ld_ext) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= ncol) return;
  for (int s = 0; s < nseries; ++s) {  // uniform trip count, uniform table words
    const int32_t kind = tab.w[s] >> 8;
    const int64_t row = tab.w[s] & 0xff;
    T* vmax = val + (int64_t)(2 * s) * ld_ext + c;
    T* vmin = vmax + ld_ext;
    int32_t* wmax = when + (int64_t)(2 * s) * ld_ext + c;
    int32_t* wmin = wmax + ld_ext;
    // the running extremes first, so that their loads and the value's are in
    // flight together (k is uniform; the interval's first step reads neither)
    T mx = (T)0, mn = (T)0;
    if (k != 1) {
      mx = *vmax;
      mn = *vmin;
    }
    T v;
    if (kind == NMP_EXT_SRC_STATE) {
      v = state[row * ld + c];
    } else {
      const T* block = kind == NMP_EXT_SRC_DIAG ? diag : forcing;
      v = __builtin_nontemporal_load(block + row * ld + c);
      // (keeps this arm's load apart from the state arm's: merged, the two
      // become one plain load and the hint is lost)
      asm volatile("" : "+v"(v));
    }
    if (k == 1) {  // the interval's first step takes any value: no reset launch
      *vmax = v;
      *vmin = v;
      *wmax = 1;
      *wmin = 1;
      continue;
    }
    if ((v > mx) || (mx != mx && v == v)) {
      *vmax = v;
      *wmax = k;
    }
    if ((v < mn) || (mn != mn && v == v)) {
      *vmin = v;
      *wmin = k;
    }
  }
}

template <class T>
__global__ __launch_bounds__(256) void extremes_output_kernel(int64_t ncol, int nseries,
                                                              ExtTable tab, double dt,
                                                              const T* __restrict__ val,
                                                              const int32_t* __restrict__ when,
                                                              int64_t ld_ext, T* __restrict__ out,
                                                              int64_t ld_out) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= ncol) return;
  T* o = out + c;  // the next output row (uniform)
  for (int s = 0; s < nseries; ++s) {
    const int32_t m = tab.w[s];
    const T* v = val + (int64_t)(2 * s) * ld_ext + c;
    const int32_t* w = when + (int64_t)(2 * s) * ld_ext + c;
    if (m & NMP_EXT_MAX) {
      *o = v[0];
      o += ld_out;
    }
    if (m & NMP_EXT_MIN) {
      *o = v[ld_ext];
      o += ld_out;
    }
    if (m & NMP_EXT_TMAX) {
      *o = (T)((double)w[0] * dt);
      o += ld_out;
    }
    if (m & NMP_EXT_TMIN) {
      *o = (T)((double)w[ld_ext] * dt);
      o += ld_out;
    }
  }
}

}  // namespace nmp

extern "C" {

int nmp_extremes_update(nmp_engine* eng, int64_t ncol, int64_t ld, int nseries,
                        const int32_t* series, const void* diag, const void* forcing,
                        const void* state, int32_t k, void* val, int32_t* when, int64_t ld_ext,
                        void* stream) {
  if (!eng || ncol < 0 || nmp::bad_ld(ld, ncol) || nmp::bad_ld(ld_ext, ncol)) return NMP_E_ARG;
  if (nseries < 1 || nseries > NMP_EXT_MAXSERIES || !series || k < 1) return NMP_E_ARG;
  nmp::ExtTable tab = {};
  bool need[3] = {false, false, false};
  for (int s = 0; s < nseries; ++s) {
    const int32_t kind = series[2 * s], row = series[2 * s + 1];
    if (kind != NMP_EXT_SRC_DIAG && kind != NMP_EXT_SRC_FORCING && kind != NMP_EXT_SRC_STATE)
      return NMP_E_ARG;
    const int32_t nrow = kind == NMP_EXT_SRC_DIAG      ? NMP_NDIAG_OUT
                         : kind == NMP_EXT_SRC_FORCING ? NMP_NFORCING
                                                       : NMP_NSTATE;
    if (row < 0 || row >= nrow) return NMP_E_ARG;
    need[kind] = true;
    tab.w[s] = kind << 8 | row;
  }
  if (ncol == 0) return NMP_OK;
  if (!val || !when || (need[NMP_EXT_SRC_DIAG] && !diag) ||
      (need[NMP_EXT_SRC_FORCING] && !forcing) || (need[NMP_EXT_SRC_STATE] && !state))
    return NMP_E_ARG;
  if (int rc = nmp::ensure_device(eng->device)) return rc;
  return nmp::launch_cols(eng->precision, ncol, stream, nmp::extremes_update_kernel<float>,
                          nmp::extremes_update_kernel<double>, ncol, ld, nseries, tab, diag,
                          forcing, state, k, val, when, ld_ext);
}

int nmp_extremes_output(nmp_engine* eng, int64_t ncol, int nseries, const int32_t* stats,
                        double dt, const void* val, const int32_t* when, int64_t ld_ext,
                        void* out, int64_t ld_out, void* stream) {
  if (!eng || ncol < 0 || nmp::bad_ld(ld_ext, ncol) || nmp::bad_ld(ld_out, ncol))
    return NMP_E_ARG;
  if (nseries < 1 || nseries > NMP_EXT_MAXSERIES || !stats) return NMP_E_ARG;
  // the negated form also refuses NaN
  if (!(dt > 0.0) || !std::isfinite(dt)) return NMP_E_ARG;
  nmp::ExtTable tab = {};
  const int32_t all = NMP_EXT_MAX | NMP_EXT_MIN | NMP_EXT_TMAX | NMP_EXT_TMIN;
  for (int s = 0; s < nseries; ++s) {
    if (stats[s] == 0 || (stats[s] & ~all)) return NMP_E_ARG;
    tab.w[s] = stats[s];
  }
  if (ncol == 0) return NMP_OK;
  if (!val || !when || !out) return NMP_E_ARG;
  if (int rc = nmp::ensure_device(eng->device)) return rc;
  return nmp::launch_cols(eng->precision, ncol, stream, nmp::extremes_output_kernel<float>,
                          nmp::extremes_output_kernel<double>, ncol, nseries, tab, dt, val, when,
                          ld_ext, out, ld_out);
}

}  // extern "C"
