// Vegetation fraction through the year: row NMP_F_SHDFAC of static_f for a
// date, from the resident 12-month GREENFRAC climatology (nmp_static_monthly).
//
// One lane per column and coalesced dword rows, as interp.hip's kernels.  Every
// operation is one IEEE double operation in the order the header documents (no
// contraction: the build keeps -ffp-contract=off); the result is rounded once
// to fp32 and then widened to the engine precision, which the numpy
// restatement in noahmp-1_amd/vegclim.py follows operation for operation.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "engine_impl.h"

namespace nmp {

// m0 and m1 are launch-uniform: the two rows' bases are scalar.  No special
// case: w == 0, NaN, -0 and subnormals go through the formula.
template <class T>
__global__ __launch_bounds__(256) void static_monthly_kernel(int64_t ncol,
                                                             const float* __restrict__ row0,
                                                             const float* __restrict__ row1,
                                                             double u, double w,
                                                             T* __restrict__ out) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= ncol) return;
  const double a = (double)row0[c];
  const double b = (double)row1[c];
  const float r = (float)(u * a + w * b);
  out[c] = (T)r;
}

}  // namespace nmp

extern "C" {

int nmp_static_monthly(nmp_engine* eng, int64_t ncol, int64_t ld_tab, const float* table12,
                       int m0, int m1, double w, void* out_row, void* stream) {
  if (!eng || ncol < 0 || nmp::bad_ld(ld_tab, ncol)) return NMP_E_ARG;
  if (m0 < 0 || m0 > 11 || m1 < 0 || m1 > 11) return NMP_E_ARG;
  // the negated form also refuses NaN
  if (!(w >= 0.0 && w < 1.0)) return NMP_E_ARG;
  if (ncol == 0) return NMP_OK;
  if (!table12 || !out_row) return NMP_E_ARG;
  if (int rc = nmp::ensure_device(eng->device)) return rc;
  const double u = 1.0 - w;
  const float* row0 = table12 + (int64_t)m0 * ld_tab;
  const float* row1 = table12 + (int64_t)m1 * ld_tab;
  return nmp::launch_cols(eng->precision, ncol, stream, nmp::static_monthly_kernel<float>,
                          nmp::static_monthly_kernel<double>, ncol, row0, row1, u, w, out_row);
}

}  // extern "C"
