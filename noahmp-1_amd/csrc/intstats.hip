// Interval statistics (nmp_intstats_update / nmp_intstats_output): over an
// output interval, the mean of up to NMP_IST_MAXITEMS per-column series, or --
// for a series with a condition v OP c -- the time the condition held, its
// longest unbroken spell and the value-seconds beyond the threshold.  The
// reference writes no output at all; the items, the rule and the rows are this
// engine's (include/noahmp_engine.h "Interval statistics").
//
// Two bandwidth-bound kernels of their own, enqueued on the step's stream right
// after it, built like the extremes kernels (extremes.hip): one lane per
// column, field-major SoA, the item table a kernel argument passed by value, so
// an item's kind, row, operator and threshold and every row base are
// wave-uniform: the loop over the items is a scalar loop around coalesced row
// accesses.  diag and forcing rows are read once (nontemporal loads keep them
// out of the way of acc / cnt, which the next step's call reads again); state
// rows, acc and cnt take plain accesses.
//
// The arithmetic is one double add per step and item (of the value, or of its
// distance from the threshold), and at output one division or one product and
// one conversion: nothing a compiler could contract, so a host restates every
// bit (noahmp-1_amd/intstats.py).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "engine_impl.h"

namespace nmp {

namespace {

// by-value kernel arguments: word i is kind << 16 | row << 8 | op << 4 | stat
// mask of item i; c[i] its threshold
struct IstWords {
  int32_t w[NMP_IST_MAXITEMS];
};
struct IstTable {
  IstWords t;
  double c[NMP_IST_MAXITEMS];
};

}  // namespace

template <class T>
__global__ __launch_bounds__(256) void intstats_update_kernel(
    int64_t ncol, int64_t ld, int nitems, IstTable tab, const T* __restrict__ diag,
    const T* __restrict__ forcing, const T* __restrict__ state, int32_t k,
    double* __restrict__ acc, int32_t* __restrict__ cnt, int64_t ld_st) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= ncol) return;
  const bool first = k == 1;  // uniform
  for (int i = 0; i < nitems; ++i) {  // uniform trip count, uniform table words
    const int32_t w = tab.t.w[i];
    const int32_t kind = w >> 16, op = (w >> 4) & 0xf;
    const int64_t row = (w >> 8) & 0xff;
    double* pa = acc + (int64_t)i * ld_st + c;
    int32_t* pn = cnt + (int64_t)(3 * i) * ld_st + c;
    int32_t* prun = pn + ld_st;
    int32_t* plong = prun + ld_st;
    // the resident state first, so that its loads and the value's are in
    // flight together (the interval's first step reads none of it)
    double a = 0.0;
    int32_t n = 0, run = 0, lng = 0;
    if (!first) {
      a = *pa;
      if (op != NMP_IST_NONE) {
        n = *pn;
        run = *prun;
        lng = *plong;
      }
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
    if (op == NMP_IST_NONE) {
      *pa = a + (double)v;
      continue;
    }
    const T ct = (T)tab.c[i];
    const bool above = op == NMP_IST_GT || op == NMP_IST_GE;
    const bool h = op == NMP_IST_GT   ? v > ct
                   : op == NMP_IST_GE ? v >= ct
                   : op == NMP_IST_LT ? v < ct
                                      : v <= ct;
    int32_t run2 = 0, lng2 = lng;
    if (h) {
      const double d = above ? (double)v - (double)ct : (double)ct - (double)v;
      a = a + d;
      n += 1;
      run2 = run + 1;
      lng2 = lng > run2 ? lng : run2;
    }
    if (first || h) {
      *pa = a;
      *pn = n;
    }
    if (first || run2 != run) *prun = run2;
    if (first || lng2 != lng) *plong = lng2;
  }
}

template <class T>
__global__ __launch_bounds__(256) void intstats_output_kernel(
    int64_t ncol, int nitems, IstWords tab, int32_t k, double dt, const double* __restrict__ acc,
    const int32_t* __restrict__ cnt, int64_t ld_st, T* __restrict__ out, int64_t ld_out) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= ncol) return;
  T* o = out + c;  // the next output row (uniform)
  for (int i = 0; i < nitems; ++i) {
    const int32_t m = tab.w[i] & 0xf;
    const double* a = acc + (int64_t)i * ld_st + c;
    const int32_t* n = cnt + (int64_t)(3 * i) * ld_st + c;
    if (m & NMP_IST_MEAN) {
      *o = (T)(a[0] / (double)k);
      o += ld_out;
    }
    if (m & NMP_IST_DUR) {
      *o = (T)((double)n[0] * dt);
      o += ld_out;
    }
    if (m & NMP_IST_DEG) {
      *o = (T)(a[0] * dt);
      o += ld_out;
    }
    if (m & NMP_IST_SPELL) {
      *o = (T)((double)n[2 * ld_st] * dt);
      o += ld_out;
    }
  }
}

namespace {

// The items' table words from the host array, and which blocks they name
// (need[kind]; need[3]: a conditioned item, which has cnt rows).  False for a
// bad item.  thresholds == nullptr: not checked (the output entry).
bool ist_table(int nitems, const int32_t* items, const double* thresholds, IstTable* tab,
               bool need[4]) {
  for (int i = 0; i < nitems; ++i) {
    const int32_t kind = items[4 * i], row = items[4 * i + 1], op = items[4 * i + 2],
                  m = items[4 * i + 3];
    if (kind != NMP_EXT_SRC_DIAG && kind != NMP_EXT_SRC_FORCING && kind != NMP_EXT_SRC_STATE)
      return false;
    const int32_t nrow = kind == NMP_EXT_SRC_DIAG      ? NMP_NDIAG_OUT
                         : kind == NMP_EXT_SRC_FORCING ? NMP_NFORCING
                                                       : NMP_NSTATE;
    if (row < 0 || row >= nrow) return false;
    if (op < NMP_IST_NONE || op > NMP_IST_LE) return false;
    const int32_t cond = NMP_IST_DUR | NMP_IST_DEG | NMP_IST_SPELL;
    if (m == 0 || (m & ~(op == NMP_IST_NONE ? NMP_IST_MEAN : cond))) return false;
    if (op != NMP_IST_NONE && thresholds && !std::isfinite(thresholds[i])) return false;
    need[kind] = true;
    if (op != NMP_IST_NONE) need[3] = true;
    tab->t.w[i] = kind << 16 | row << 8 | op << 4 | m;
    tab->c[i] = thresholds && op != NMP_IST_NONE ? thresholds[i] : 0.0;
  }
  return true;
}

}  // namespace

}  // namespace nmp

extern "C" {

int nmp_intstats_update(nmp_engine* eng, int64_t ncol, int64_t ld, int nitems,
                        const int32_t* items, const double* thresholds, const void* diag,
                        const void* forcing, const void* state, int32_t k, double* acc,
                        int32_t* cnt, int64_t ld_st, void* stream) {
  if (!eng || ncol < 0 || nmp::bad_ld(ld, ncol) || nmp::bad_ld(ld_st, ncol)) return NMP_E_ARG;
  if (nitems < 1 || nitems > NMP_IST_MAXITEMS || !items || !thresholds || k < 1)
    return NMP_E_ARG;
  nmp::IstTable tab = {};
  bool need[4] = {false, false, false, false};
  if (!nmp::ist_table(nitems, items, thresholds, &tab, need)) return NMP_E_ARG;
  if (ncol == 0) return NMP_OK;
  if (!acc || (need[3] && !cnt) || (need[NMP_EXT_SRC_DIAG] && !diag) ||
      (need[NMP_EXT_SRC_FORCING] && !forcing) || (need[NMP_EXT_SRC_STATE] && !state))
    return NMP_E_ARG;
  if (int rc = nmp::ensure_device(eng->device)) return rc;
  return nmp::launch_cols(eng->precision, ncol, stream, nmp::intstats_update_kernel<float>,
                          nmp::intstats_update_kernel<double>, ncol, ld, nitems, tab, diag,
                          forcing, state, k, acc, cnt, ld_st);
}

int nmp_intstats_output(nmp_engine* eng, int64_t ncol, int nitems, const int32_t* items,
                        int32_t k, double dt, const double* acc, const int32_t* cnt,
                        int64_t ld_st, void* out, int64_t ld_out, void* stream) {
  if (!eng || ncol < 0 || nmp::bad_ld(ld_st, ncol) || nmp::bad_ld(ld_out, ncol))
    return NMP_E_ARG;
  if (nitems < 1 || nitems > NMP_IST_MAXITEMS || !items || k < 1) return NMP_E_ARG;
  // the negated form also refuses NaN
  if (!(dt > 0.0) || !std::isfinite(dt)) return NMP_E_ARG;
  nmp::IstTable tab = {};
  bool need[4] = {false, false, false, false};
  if (!nmp::ist_table(nitems, items, nullptr, &tab, need)) return NMP_E_ARG;
  if (ncol == 0) return NMP_OK;
  if (!acc || !out || (need[3] && !cnt)) return NMP_E_ARG;
  if (int rc = nmp::ensure_device(eng->device)) return rc;
  return nmp::launch_cols(eng->precision, ncol, stream, nmp::intstats_output_kernel<float>,
                          nmp::intstats_output_kernel<double>, ncol, nitems, tab.t, k, dt, acc,
                          cnt, ld_st, out, ld_out);
}

}  // extern "C"
