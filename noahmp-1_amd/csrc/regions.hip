// Region-aggregated output (nmp_region_reduce): weighted sums and means of the
// fields of a field-major SoA block over the columns of each region -- basin
// means of an output step's fluxes -- formed on the device, so nfield x nreg
// doubles leave it instead of nfield x npts words.  No reference counterpart.
//
// The summation tree is fixed by the plan alone and is part of the interface
// (include/noahmp_engine.h states it; tests/test_gpu_regions.py restates it in
// numpy).  It does not depend on the launch shape, the stream or the engine
// precision's width, there are no atomics and no completion flags, and every
// operation is one IEEE double operation (the build has -ffp-contract=off),
// so a host reproduces every bit.  Its pieces are col_math.h's:
//
//   pass 1  one wavefront per chunk of NMP_REGION_CHUNK plan entries; the
//           terms are the rounded products (double)v * w (pad entries,
//           entry_col < 0, are skipped: not loaded, not multiplied); lane 0
//           writes partial[f*nchunk + k].
//   pass 2  per (region, field), by one thread or, for plans of long regions,
//           one wavefront (the same sequence): the region's chunk partials
//           added in chunk order; sums[f*nreg + r], and, where asked,
//           means[f*nreg + r] = sum / wsum[r] (one division; 0/0 = NaN for a
//           region without chunks).
//
// NaN and the night-time ALBEDO = -999.9 (hazard H8) reduce as the values
// they are: nothing is masked.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <mutex>

#include "col_math.h"
#include "engine_impl.h"

namespace nmp {

namespace {

static_assert(NMP_REGION_CHUNK == kWave * kPerLane, "one wavefront per chunk");

// G fields of one chunk: all of the lane's loads first (G x 4 independent
// nontemporal loads in flight), then each field's four adds and its butterfly.
// FULL: the chunk has no pad (every chunk of a region but its last, as a
// rule; col_math.h chunk_full).
template <class T, int G, bool FULL>
__device__ __forceinline__ void reduce_fields(const T* __restrict__ fields, int64_t ld, int f0,
                                              const int32_t (&col)[kPerLane],
                                              const double (&w)[kPerLane], int lane,
                                              double* __restrict__ out, int64_t nchunk) {
  T v[G][kPerLane];
#pragma unroll
  for (int j = 0; j < kPerLane; ++j) {
    // one predicate around the G loads of entry j, not one around each
    if (FULL || col[j] >= 0) {
#pragma unroll
      for (int g = 0; g < G; ++g)
        v[g][j] = __builtin_nontemporal_load(fields + (int64_t)(f0 + g) * ld + col[j]);
    } else {
#pragma unroll
      for (int g = 0; g < G; ++g) v[g][j] = (T)0;
    }
  }
#pragma unroll
  for (int g = 0; g < G; ++g) {
    double x = 0.0;
#pragma unroll
    for (int j = 0; j < kPerLane; ++j)
      if (FULL || col[j] >= 0) x = x + (double)v[g][j] * w[j];
    x = wave_sum(x);
    if (lane == 0) out[(int64_t)(f0 + g) * nchunk] = x;
  }
}

template <class T, bool FULL>
__device__ __forceinline__ void reduce_chunk(const T* __restrict__ fields, int64_t ld, int nfield,
                                             const int32_t (&col)[kPerLane],
                                             const double (&w)[kPerLane], int lane,
                                             double* __restrict__ out, int64_t nchunk) {
  int f = 0;
  for (; f + 8 <= nfield; f += 8)
    reduce_fields<T, 8, FULL>(fields, ld, f, col, w, lane, out, nchunk);
  if (f + 4 <= nfield) {
    reduce_fields<T, 4, FULL>(fields, ld, f, col, w, lane, out, nchunk);
    f += 4;
  }
  for (; f < nfield; ++f) reduce_fields<T, 1, FULL>(fields, ld, f, col, w, lane, out, nchunk);
}

// The plan's entries are read once per chunk, not once per field.  An
// entry_col outside [0, ncol) is treated as a pad: the kernel never reads
// outside the block it was given.
template <class T>
__global__ __launch_bounds__(kWave* kWavesPerBlock) void region_pass1_kernel(
    int64_t ncol, int64_t ld, int nfield, const T* __restrict__ fields, int64_t nchunk,
    const int32_t* __restrict__ entry_col, const double* __restrict__ entry_w,
    double* __restrict__ partial) {
  const int lane = threadIdx.x % kWave;
  const int64_t k = (int64_t)blockIdx.x * kWavesPerBlock + threadIdx.x / kWave;
  if (k >= nchunk) return;  // whole waves leave: the butterfly below is over full waves
  int32_t col[kPerLane];
  double w[kPerLane];
#pragma unroll
  for (int j = 0; j < kPerLane; ++j) {
    const int64_t e = k * NMP_REGION_CHUNK + j * kWave + lane;
    const int32_t c = __builtin_nontemporal_load(entry_col + e);
    col[j] = (c >= 0 && (int64_t)c < ncol) ? c : -1;
    w[j] = __builtin_nontemporal_load(entry_w + e);
  }
  double* out = partial + k;
  const bool ok[kPerLane] = {col[0] >= 0, col[1] >= 0, col[2] >= 0, col[3] >= 0};
  if (chunk_full(ok))
    reduce_chunk<T, true>(fields, ld, nfield, col, w, lane, out, nchunk);
  else
    reduce_chunk<T, false>(fields, ld, nfield, col, w, lane, out, nchunk);
}

// Thread t is (region t % nreg, field t / nreg): neighbouring threads read
// neighbouring regions' partials.  A chunk range outside [0, nchunk] is clipped.
__global__ __launch_bounds__(256) void region_pass2_kernel(
    int nfield, int64_t nchunk, int64_t nreg, const int64_t* __restrict__ region_chunk0,
    const double* __restrict__ wsum, const double* __restrict__ partial,
    double* __restrict__ sums, double* __restrict__ means) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= nreg * nfield) return;
  const int64_t r = t % nreg, f = t / nreg;
  int64_t k0 = region_chunk0[r], k1 = region_chunk0[r + 1];
  if (k0 < 0) k0 = 0;
  if (k1 > nchunk) k1 = nchunk;
  const double* p = partial + f * nchunk;
  double sum = 0.0;
  int64_t k = k0;
  // the loads of a batch do not depend on the adds: 16 in flight, added in order
  for (; k + 16 <= k1; k += 16) {
    double v[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) v[i] = p[k + i];
#pragma unroll
    for (int i = 0; i < 16; ++i) sum = sum + v[i];
  }
  for (; k < k1; ++k) sum = sum + p[k];
  sums[f * nreg + r] = sum;
  if (means) means[f * nreg + r] = sum / wsum[r];
}

// The same sums for plans of long regions (one basin over a million columns
// is 4,096 partials): one wavefront per (region, field), the sequential tree
// of region_pass2_kernel, bit for bit.
__global__ __launch_bounds__(kWave* kWavesPerBlock) void region_pass2_wave_kernel(
    int nfield, int64_t nchunk, int64_t nreg, const int64_t* __restrict__ region_chunk0,
    const double* __restrict__ wsum, const double* __restrict__ partial,
    double* __restrict__ sums, double* __restrict__ means) {
  const int lane = threadIdx.x % kWave;
  const int64_t t = (int64_t)blockIdx.x * kWavesPerBlock + threadIdx.x / kWave;
  if (t >= nreg * nfield) return;
  const int64_t r = t % nreg, f = t / nreg;
  int64_t k0 = region_chunk0[r], k1 = region_chunk0[r + 1];
  if (k0 < 0) k0 = 0;
  if (k1 > nchunk) k1 = nchunk;
  const double sum = wave_ordered_sum(partial + f * nchunk, k0, k1, lane);
  if (lane == 0) {
    sums[f * nreg + r] = sum;
    if (means) means[f * nreg + r] = sum / wsum[r];
  }
}

// average chunks per region from which pass 2 runs one wave per (region, field)
constexpr int64_t kPass2WaveMinChunks = 32;
// most fields one nmp_region_reduce call takes (its launches count
// nreg x nfield threads in 64 bits and blocks in 32)
constexpr int kMaxRegionFields = 1024;

}  // namespace

}  // namespace nmp

extern "C" {

int nmp_region_reduce(nmp_engine* eng, int64_t ncol, int64_t ld, int nfield, const void* fields,
                      int64_t nchunk, const int32_t* entry_col, const double* entry_w,
                      int64_t nreg, const int64_t* region_chunk0, const double* wsum,
                      double* partial, double* sums, double* means, void* stream) {
  using namespace nmp;
  if (!eng || ncol < 0 || bad_ld(ld, ncol) || nfield < 1 || nfield > kMaxRegionFields ||
      nchunk < 0 || nchunk >= kMaxColumns || nreg < 0 || nreg >= kMaxColumns ||
      nreg * nfield / 256 >= INT32_MAX)
    return NMP_E_ARG;
  if (nchunk == 0 || nreg == 0) return NMP_OK;
  if (!fields || !entry_col || !entry_w || !region_chunk0 || !wsum || !partial || !sums)
    return NMP_E_ARG;
  if (int rc = ensure_device(eng->device)) return rc;
  // the two passes of one call are enqueued back to back
  std::lock_guard<std::mutex> lk(eng->host_mu);
  const hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 block(kWave * kWavesPerBlock);
  const dim3 grid1((unsigned)((nchunk + kWavesPerBlock - 1) / kWavesPerBlock));
  if (eng->precision == 4)
    hipLaunchKernelGGL(region_pass1_kernel<float>, grid1, block, 0, st, ncol, ld, nfield,
                       static_cast<const float*>(fields), nchunk, entry_col, entry_w, partial);
  else
    hipLaunchKernelGGL(region_pass1_kernel<double>, grid1, block, 0, st, ncol, ld, nfield,
                       static_cast<const double*>(fields), nchunk, entry_col, entry_w, partial);
  if (int rc = rc_of(hipGetLastError())) return rc;
  // which of the two pass-2 kernels runs changes the time, never a bit
  if (nchunk >= kPass2WaveMinChunks * nreg) {
    const int64_t grid2 = (nreg * nfield + kWavesPerBlock - 1) / kWavesPerBlock;
    hipLaunchKernelGGL(region_pass2_wave_kernel, dim3((unsigned)grid2), block, 0, st, nfield,
                       nchunk, nreg, region_chunk0, wsum, partial, sums, means);
  } else {
    const int64_t grid2 = (nreg * nfield + 255) / 256;
    hipLaunchKernelGGL(region_pass2_kernel, dim3((unsigned)grid2), dim3(256), 0, st, nfield,
                       nchunk, nreg, region_chunk0, wsum, partial, sums, means);
  }
  return rc_of(hipGetLastError());
}

}  // extern "C"

