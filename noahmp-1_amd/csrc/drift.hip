// Spin-up drift (nmp_state_drift / nmp_drift_reduce): how far the land state
// at the end of a pass over the forcing period lies from where the pass before
// left it, measured next to the state, and its reduction to a few dozen
// numbers -- what lets a spin-up decide on the device's side of the bus that
// it has converged.  No reference counterpart (HRLDAS loops its forcing by a
// namelist entry and tests nothing).
//
// nmp_state_drift: one lane per column, field-major SoA like every other
// array.  It forms the column's 13 tracked values (NMP_K_*) from the state
// block, writes -- where asked -- the 7 drift groups (NMP_G_*) against the
// snapshot of the pass before, and then stores the new tracked values into
// the snapshot: one launch measures a loop and arms the next, the way
// accum_finish_kernel rolls stor_beg.  Every operation is one IEEE operation
// in the order the header documents (the build keeps -ffp-contract=off),
// which spinup.py restates in numpy operation for operation.  The state rows
// are read once: nontemporal loads, as in accum.hip.
//
// nmp_drift_reduce: per group the largest drift and where, the count of
// columns over the tolerance and the weighted sum, over the rank's whole
// block.  The sum's tree is fixed by the interface (include/noahmp_engine.h
// "Spin-up drift"; its pieces are col_math.h's), there are no atomics and no
// completion flags, and every operation is one IEEE double operation, so a
// host reproduces every bit.  The terms of pass 1 are the rounded products
// (double)d * w of columns 256 k + l + 64 j, j = 0..3 (a column >= ncol or of
// weight 0 is left out: not loaded, not multiplied).
//
// max, arg and count do not depend on the order they are combined in; the
// lanes and chunks combine them by the same butterfly and a strided loop.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <mutex>

#include "col_math.h"
#include "engine_impl.h"

namespace nmp {

template <class T>
__global__ __launch_bounds__(256) void state_drift_kernel(int64_t ncol, int64_t ld,
                                                          const T* __restrict__ state,
                                                          const int32_t* __restrict__ isnow,
                                                          const int32_t* __restrict__ static_i,
                                                          T* __restrict__ snap, int64_t ld_snap,
                                                          T* __restrict__ drift,
                                                          int64_t ld_drift) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= ncol) return;
  const T* s = state + c;
  auto ld1 = [&](int row) { return __builtin_nontemporal_load(s + row * ld); };
  T v[NMP_NTRACKED], smc[NMP_NSOIL];
#pragma unroll
  for (int i = 0; i < NMP_NSOIL; ++i) v[NMP_K_SMC + i] = smc[i] = ld1(NMP_S_SMC + i);
#pragma unroll
  for (int i = 0; i < NMP_NSOIL; ++i) v[NMP_K_STC + i] = ld1(NMP_S_STC + NMP_NSNOW + i);
  v[NMP_K_SNEQV] = ld1(NMP_S_SNEQV);
  v[NMP_K_WA] = ld1(NMP_S_WA);
  v[NMP_K_ZWT] = ld1(NMP_S_ZWT);
  // TWS: ZSNSO's soil rows are C index 2..6
  T z[NMP_NSOIL + 1], dz[NMP_NSOIL];
#pragma unroll
  for (int i = 0; i <= NMP_NSOIL; ++i) z[i] = ld1(NMP_S_ZSNSO + 2 + i);
  const T canliq = ld1(NMP_S_CANLIQ), canice = ld1(NMP_S_CANICE);
  const int isn = __builtin_nontemporal_load(isnow + c);
  const int ist = __builtin_nontemporal_load(static_i + NMP_I_IST * ld + c);
  T pool[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) pool[i] = ld1(NMP_S_LFMASS + i);

  soil_thickness(z, isn, dz);
  const T w = water_storage(canliq, canice, v[NMP_K_SNEQV], v[NMP_K_WA], smc, dz);
  v[NMP_K_TWS] = ist == 1 ? w : (T)0;
  v[NMP_K_CTOT] = ((((pool[0] + pool[1]) + pool[2]) + pool[3]) + pool[4]) + pool[5];

  T* sn = snap + c;
  if (drift) {  // uniform over the launch
    T d[NMP_NTRACKED];
#pragma unroll
    for (int k = 0; k < NMP_NTRACKED; ++k) d[k] = fabs(v[k] - sn[k * ld_snap]);
    T* o = drift + c;
    // the layered groups: the layers' largest drift, a NaN sticks
    constexpr int kLayered[2][2] = {{NMP_G_SOIL_M, NMP_K_SMC}, {NMP_G_SOIL_T, NMP_K_STC}};
#pragma unroll
    for (int g = 0; g < 2; ++g) {
      T m = d[kLayered[g][1]];
#pragma unroll
      for (int i = 1; i < NMP_NSOIL; ++i) {
        const T x = d[kLayered[g][1] + i];
        m = (x > m || x != x) ? x : m;
      }
      o[kLayered[g][0] * ld_drift] = m;
    }
    o[NMP_G_SNEQV * ld_drift] = d[NMP_K_SNEQV];
    o[NMP_G_WA * ld_drift] = d[NMP_K_WA];
    o[NMP_G_ZWT * ld_drift] = d[NMP_K_ZWT];
    o[NMP_G_TWS * ld_drift] = d[NMP_K_TWS];
    o[NMP_G_CARBON * ld_drift] = d[NMP_K_CTOT];
  }
#pragma unroll
  for (int k = 0; k < NMP_NTRACKED; ++k) sn[k * ld_snap] = v[k];
}

namespace {

static_assert(NMP_DRIFT_CHUNK == kWave * kPerLane, "one wavefront per chunk");
constexpr int kNG = NMP_NDRIFT;

// rows of the pass-1 scratch, each nchunk 8-byte words: the 7 weighted sums
// and the weights' sum (double), the chunk's max (double), its arg and its
// count of columns over the tolerance (int64): NMP_DRIFT_SCRATCH = 29 rows
constexpr int kRowSum = 0, kRowMax = kNG + 1, kRowArg = 2 * kNG + 1, kRowCount = 3 * kNG + 1;
static_assert(kRowCount + kNG == NMP_DRIFT_SCRATCH, "scratch rows");

// (m, a): a candidate for a group's max and its column; a < 0 = none yet.  A
// NaN beats every number, a larger number a smaller one, and among equals (or
// among NaNs) the lower column wins: commutative and associative, so lanes
// and chunks may be combined in any order.
__device__ __forceinline__ void better(double& m, int64_t& a, double m2, int64_t a2) {
  if (a2 < 0) return;
  const bool n1 = m != m, n2 = m2 != m2;
  const bool take = a < 0 || (n2 && !n1) || (n1 == n2 && (n1 || m2 == m) && a2 < a) ||
                    (!n1 && !n2 && m2 > m);
  if (take) {
    m = m2;
    a = a2;
  }
}

// FULL: no column of the chunk is left out (col_math.h chunk_full)
template <class T, bool FULL>
__device__ __forceinline__ void reduce_chunk(const T* __restrict__ drift, int64_t ld_drift,
                                             const int64_t (&col)[kPerLane],
                                             const bool (&ok)[kPerLane],
                                             const double (&w)[kPerLane],
                                             const double* __restrict__ tol, int lane,
                                             double* __restrict__ part, int64_t nchunk) {
  T v[kNG][kPerLane];
#pragma unroll
  for (int j = 0; j < kPerLane; ++j) {
    // one predicate around the 7 loads of column j, not one around each
    if (FULL || ok[j]) {
#pragma unroll
      for (int g = 0; g < kNG; ++g)
        v[g][j] = __builtin_nontemporal_load(drift + (int64_t)g * ld_drift + col[j]);
    } else {
#pragma unroll
      for (int g = 0; g < kNG; ++g) v[g][j] = (T)0;
    }
  }
  int64_t* parti = reinterpret_cast<int64_t*>(part);
#pragma unroll
  for (int g = 0; g < kNG; ++g) {
    const double t = tol[g];
    double x = 0.0, m = 0.0;
    int64_t a = -1, n = 0;
#pragma unroll
    for (int j = 0; j < kPerLane; ++j)
      if (FULL || ok[j]) {
        const double d = (double)v[g][j];
        x = x + d * w[j];
        better(m, a, d, col[j]);
        n += !(d <= t);
      }
    x = wave_sum(x);
#pragma unroll
    for (int s = kWave / 2; s >= 1; s >>= 1) {
      better(m, a, __shfl_xor(m, s, kWave), shfl_xor_i64(a, s));
      n += shfl_xor_i64(n, s);
    }
    if (lane == 0) {
      part[(kRowSum + g) * nchunk] = x;
      part[(kRowMax + g) * nchunk] = m;
      parti[(kRowArg + g) * nchunk] = a;
      parti[(kRowCount + g) * nchunk] = n;
    }
  }
  double x = 0.0;
#pragma unroll
  for (int j = 0; j < kPerLane; ++j)
    if (FULL || ok[j]) x = x + w[j];
  x = wave_sum(x);
  if (lane == 0) part[(kRowSum + kNG) * nchunk] = x;
}

template <class T>
__global__ __launch_bounds__(kWave* kWavesPerBlock) void drift_pass1_kernel(
    int64_t ncol, int64_t ld_drift, const T* __restrict__ drift,
    const double* __restrict__ weight, const double* __restrict__ tol, int64_t nchunk,
    double* __restrict__ partial) {
  const int lane = threadIdx.x % kWave;
  const int64_t k = (int64_t)blockIdx.x * kWavesPerBlock + threadIdx.x / kWave;
  if (k >= nchunk) return;  // whole waves leave: the butterfly is over full waves
  int64_t col[kPerLane];
  bool ok[kPerLane];
  double w[kPerLane];
#pragma unroll
  for (int j = 0; j < kPerLane; ++j) {
    col[j] = k * NMP_DRIFT_CHUNK + j * kWave + lane;
    ok[j] = col[j] < ncol;
    w[j] = 1.0;
    if (weight && ok[j]) {
      w[j] = __builtin_nontemporal_load(weight + col[j]);
      ok[j] = w[j] != 0.0;  // the caller's mask
    }
  }
  double* part = partial + k;
  if (chunk_full(ok))
    reduce_chunk<T, true>(drift, ld_drift, col, ok, w, tol, lane, part, nchunk);
  else
    reduce_chunk<T, false>(drift, ld_drift, col, ok, w, tol, lane, part, nchunk);
}

// One wavefront per output.  Waves 0..7: the sum of row t of the partials
// (the 7 weighted sums, then the weights'), from +0.0 in chunk order.  Waves
// 8..14: group t - 8's max, arg and count, the lanes striding over the chunks.
__global__ __launch_bounds__(kWave* kWavesPerBlock) void drift_pass2_kernel(
    int64_t nchunk, const double* __restrict__ partial, double* __restrict__ out_max,
    int64_t* __restrict__ out_arg, double* __restrict__ out_wsum, int64_t* __restrict__ out_count,
    double* __restrict__ out_wtot) {
  const int lane = threadIdx.x % kWave;
  const int t = blockIdx.x * kWavesPerBlock + threadIdx.x / kWave;
  if (t > 2 * kNG) return;
  if (t <= kNG) {
    const double sum =
        wave_ordered_sum(partial + (int64_t)(kRowSum + t) * nchunk, 0, nchunk, lane);
    if (lane == 0) {
      if (t < kNG)
        out_wsum[t] = sum;
      else
        *out_wtot = sum;
    }
    return;
  }
  const int g = t - kNG - 1;
  const double* pm = partial + (int64_t)(kRowMax + g) * nchunk;
  const int64_t* pi = reinterpret_cast<const int64_t*>(partial);
  const int64_t* pa = pi + (int64_t)(kRowArg + g) * nchunk;
  const int64_t* pc = pi + (int64_t)(kRowCount + g) * nchunk;
  double m = 0.0;
  int64_t a = -1, n = 0;
  for (int64_t k = lane; k < nchunk; k += kWave) {
    better(m, a, pm[k], pa[k]);
    n += pc[k];
  }
#pragma unroll
  for (int s = kWave / 2; s >= 1; s >>= 1) {
    better(m, a, __shfl_xor(m, s, kWave), shfl_xor_i64(a, s));
    n += shfl_xor_i64(n, s);
  }
  if (lane == 0) {
    out_max[g] = m != m ? __longlong_as_double(0x7ff8000000000000LL) : m;
    out_arg[g] = a;
    out_count[g] = n;
  }
}

}  // namespace

}  // namespace nmp

extern "C" {

int nmp_state_drift(nmp_engine* eng, int64_t ncol, int64_t ld, const void* state,
                    const int32_t* isnow, const int32_t* static_i, void* snap, int64_t ld_snap,
                    void* drift, int64_t ld_drift, void* stream) {
  if (!eng || ncol < 0 || nmp::bad_ld(ld, ncol) || nmp::bad_ld(ld_snap, ncol) ||
      (drift && nmp::bad_ld(ld_drift, ncol)))
    return NMP_E_ARG;
  if (ncol == 0) return NMP_OK;
  if (!state || !isnow || !static_i || !snap) return NMP_E_ARG;
  if (int rc = nmp::ensure_device(eng->device)) return rc;
  std::lock_guard<std::mutex> lk(eng->host_mu);
  return nmp::launch_cols(eng->precision, ncol, stream, nmp::state_drift_kernel<float>,
                          nmp::state_drift_kernel<double>, ncol, ld, state, isnow, static_i, snap,
                          ld_snap, drift, ld_drift);
}

int nmp_drift_reduce(nmp_engine* eng, int64_t ncol, int64_t ld_drift, const void* drift,
                     const double* weight, const double* tol, void* partial, double* out_max,
                     int64_t* out_arg, double* out_wsum, int64_t* out_count, double* out_wtot,
                     void* stream) {
  using namespace nmp;
  if (!eng || ncol < 0 || bad_ld(ld_drift, ncol)) return NMP_E_ARG;
  if (!drift || !tol || !partial || !out_max || !out_arg || !out_wsum || !out_count || !out_wtot)
    return NMP_E_ARG;
  if (int rc = ensure_device(eng->device)) return rc;
  // the two passes of one call are enqueued back to back
  std::lock_guard<std::mutex> lk(eng->host_mu);
  const hipStream_t st = static_cast<hipStream_t>(stream);
  const int64_t nchunk = (ncol + NMP_DRIFT_CHUNK - 1) / NMP_DRIFT_CHUNK;
  double* part = static_cast<double*>(partial);
  const dim3 block(kWave * kWavesPerBlock);
  if (nchunk > 0) {
    const dim3 grid1((unsigned)((nchunk + kWavesPerBlock - 1) / kWavesPerBlock));
    if (eng->precision == 4)
      hipLaunchKernelGGL(drift_pass1_kernel<float>, grid1, block, 0, st, ncol, ld_drift,
                         static_cast<const float*>(drift), weight, tol, nchunk, part);
    else
      hipLaunchKernelGGL(drift_pass1_kernel<double>, grid1, block, 0, st, ncol, ld_drift,
                         static_cast<const double*>(drift), weight, tol, nchunk, part);
    if (int rc = rc_of(hipGetLastError())) return rc;
  }
  // without a column pass 2 alone writes the empty result
  const int grid2 = (2 * kNG + 1 + kWavesPerBlock - 1) / kWavesPerBlock;
  hipLaunchKernelGGL(drift_pass2_kernel, dim3(grid2), block, 0, st, nchunk, part, out_max, out_arg,
                     out_wsum, out_count, out_wtot);
  return rc_of(hipGetLastError());
}

}  // extern "C"
