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
// "Spin-up drift"), there are no atomics and no completion flags, and every
// operation is one IEEE double operation, so a host reproduces every bit:
//
//   pass 1  one wavefront per chunk of NMP_DRIFT_CHUNK = 256 columns; lane l
//           adds, from +0.0 and in this order, the rounded products
//           (double)d * w of columns 256 k + l + 64 j, j = 0..3 (a column
//           >= ncol or of weight 0 is left out: not loaded, not multiplied);
//           then the xor butterfly x = x + shfl_xor(x, s), s = 32 .. 1.
//   pass 2  from +0.0, the chunk partials added in chunk order.
//
// max, arg and count do not depend on the order they are combined in; the
// lanes and chunks combine them by the same butterfly and a strided loop.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "noahmp_engine.h"
#include "sflx_kargs.h"

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
  T v[NMP_NTRACKED];
#pragma unroll
  for (int i = 0; i < NMP_NSOIL; ++i) v[NMP_K_SMC + i] = ld1(NMP_S_SMC + i);
#pragma unroll
  for (int i = 0; i < NMP_NSOIL; ++i) v[NMP_K_STC + i] = ld1(NMP_S_STC + NMP_NSNOW + i);
  v[NMP_K_SNEQV] = ld1(NMP_S_SNEQV);
  v[NMP_K_WA] = ld1(NMP_S_WA);
  v[NMP_K_ZWT] = ld1(NMP_S_ZWT);
  // TWS: water_storage_kernel's expression; ZSNSO's soil rows are C index 2..6
  T z[NMP_NSOIL + 1];
#pragma unroll
  for (int i = 0; i <= NMP_NSOIL; ++i) z[i] = ld1(NMP_S_ZSNSO + 2 + i);
  const T canliq = ld1(NMP_S_CANLIQ), canice = ld1(NMP_S_CANICE);
  const int isn = __builtin_nontemporal_load(isnow + c);
  const int ist = __builtin_nontemporal_load(static_i + NMP_I_IST * ld + c);
  T pool[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) pool[i] = ld1(NMP_S_LFMASS + i);

  T w = ((canliq + canice) + v[NMP_K_SNEQV]) + v[NMP_K_WA];
#pragma unroll
  for (int iz = 1; iz <= NMP_NSOIL; ++iz) {
    const T zb = z[iz];
    const T dz = iz == isn + 1 ? -zb : z[iz - 1] - zb;
    w = w + (v[NMP_K_SMC + iz - 1] * dz) * (T)1000;
  }
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

hipError_t launch_state_drift(int precision, int64_t ncol, int64_t ld, const void* state,
                              const int32_t* isnow, const int32_t* static_i, void* snap,
                              int64_t ld_snap, void* drift, int64_t ld_drift,
                              hipStream_t stream) {
  const int64_t grid = (ncol + 255) / 256;
  if (grid == 0) return hipSuccess;
  if (precision == 4)
    hipLaunchKernelGGL(state_drift_kernel<float>, dim3((unsigned)grid), dim3(256), 0, stream,
                       ncol, ld, static_cast<const float*>(state), isnow, static_i,
                       static_cast<float*>(snap), ld_snap, static_cast<float*>(drift), ld_drift);
  else
    hipLaunchKernelGGL(state_drift_kernel<double>, dim3((unsigned)grid), dim3(256), 0, stream,
                       ncol, ld, static_cast<const double*>(state), isnow, static_i,
                       static_cast<double*>(snap), ld_snap, static_cast<double*>(drift),
                       ld_drift);
  return hipGetLastError();
}

namespace {

constexpr int kWave = 64;
constexpr int kPerLane = NMP_DRIFT_CHUNK / kWave;  // 4 columns per lane
constexpr int kWavesPerBlock = 4;
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

__device__ __forceinline__ int64_t shfl_xor_i64(int64_t x, int s) {
  return (int64_t)__shfl_xor((long long)x, s, kWave);
}

// FULL: no column of the chunk is left out, so loads and adds carry no
// predicate -- the same operations in the same order; with predicates the
// compiler branches around every load and waits for each (regions.hip
// measured 2.3x the time in fp32).
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
#pragma unroll
    for (int s = kWave / 2; s >= 1; s >>= 1) {
      x = x + __shfl_xor(x, s, kWave);
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
#pragma unroll
  for (int s = kWave / 2; s >= 1; s >>= 1) x = x + __shfl_xor(x, s, kWave);
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
  // wave-uniform: no lane of this chunk leaves a column out
  if (__all(ok[0] && ok[1] && ok[2] && ok[3]))
    reduce_chunk<T, true>(drift, ld_drift, col, ok, w, tol, lane, part, nchunk);
  else
    reduce_chunk<T, false>(drift, ld_drift, col, ok, w, tol, lane, part, nchunk);
}

// One wavefront per output.  Waves 0..7: the sum of row t of the partials
// (the 7 weighted sums, then the weights'), from +0.0 in chunk order -- the
// lanes load 64 consecutive partials at once, the next 64 while these are
// added, and every lane adds them in order from the lanes' registers
// (region_pass2_wave_kernel's sequence).  Waves 8..14: group t - 8's max, arg
// and count, the lanes striding over the chunks.
__global__ __launch_bounds__(kWave* kWavesPerBlock) void drift_pass2_kernel(
    int64_t nchunk, const double* __restrict__ partial, double* __restrict__ out_max,
    int64_t* __restrict__ out_arg, double* __restrict__ out_wsum, int64_t* __restrict__ out_count,
    double* __restrict__ out_wtot) {
  const int lane = threadIdx.x % kWave;
  const int t = blockIdx.x * kWavesPerBlock + threadIdx.x / kWave;
  if (t > 2 * kNG) return;
  if (t <= kNG) {
    const double* p = partial + (int64_t)(kRowSum + t) * nchunk;
    double sum = 0.0;
    double v = lane < nchunk ? p[lane] : 0.0;
    for (int64_t k = 0; k < nchunk; k += kWave) {
      const double next = k + kWave + lane < nchunk ? p[k + kWave + lane] : 0.0;
      // lane i's partial to every lane (i is uniform: two v_readlane_b32)
      const int lo = __double2loint(v), hi = __double2hiint(v);
      const int m = nchunk - k >= kWave ? kWave : (int)(nchunk - k);
      for (int i = 0; i < m; ++i)
        sum = sum + __hiloint2double(__builtin_amdgcn_readlane(hi, i),
                                     __builtin_amdgcn_readlane(lo, i));
      v = next;
    }
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

hipError_t launch_drift_reduce(int precision, int64_t ncol, int64_t ld_drift, const void* drift,
                               const double* weight, const double* tol, void* partial,
                               double* out_max, int64_t* out_arg, double* out_wsum,
                               int64_t* out_count, double* out_wtot, hipStream_t stream) {
  const int64_t nchunk = (ncol + NMP_DRIFT_CHUNK - 1) / NMP_DRIFT_CHUNK;
  double* part = static_cast<double*>(partial);
  if (nchunk > 0) {
    const int64_t grid1 = (nchunk + kWavesPerBlock - 1) / kWavesPerBlock;
    if (precision == 4)
      hipLaunchKernelGGL(drift_pass1_kernel<float>, dim3((unsigned)grid1),
                         dim3(kWave * kWavesPerBlock), 0, stream, ncol, ld_drift,
                         static_cast<const float*>(drift), weight, tol, nchunk, part);
    else
      hipLaunchKernelGGL(drift_pass1_kernel<double>, dim3((unsigned)grid1),
                         dim3(kWave * kWavesPerBlock), 0, stream, ncol, ld_drift,
                         static_cast<const double*>(drift), weight, tol, nchunk, part);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  // without a column pass 2 alone writes the empty result
  const int grid2 = (2 * kNG + 1 + kWavesPerBlock - 1) / kWavesPerBlock;
  hipLaunchKernelGGL(drift_pass2_kernel, dim3(grid2), dim3(kWave * kWavesPerBlock), 0, stream,
                     nchunk, part, out_max, out_arg, out_wsum, out_count, out_wtot);
  return hipGetLastError();
}

}  // namespace nmp
