// Test-side library (tests/lib/libnmp_libm_inrange.so, tests/test_gpu_libm_inrange.py):
// the device build of the Newton loops' in-range libm cores -- through
// nmp::MthInRange32 after stage_math_tables(), as sfcdif1 and ragrb call them,
// atanf's division by DivFast32 -- against the host build of the same header
// (atanf's division IEEE), bit for bit.
//
//   li_sweep(fn, first, count, stride, threads, res)
// compares the `count` float bit patterns first, first + stride, ... and fills
// res = {inputs compared, mismatches, first bad input, its device bits, its
// host bits}.  Returns 0, or a negative number on a HIP error.
#include <hip/hip_runtime.h>

#include <vector>

#include "sflx_math.h"

enum { F_EXP = 0, F_LOG, F_POW_Q, F_POW_MQ, F_ATAN, F_N };

static const gm::GmTables kT = {GM_EXP2F_TAB, GM_LOGF_TAB, GM_POWF_TAB};

static float host_fn(int fn, float x) {
  switch (fn) {
    case F_EXP: return gm::expf_inrange(x, kT);
    case F_LOG: return gm::logf_inrange(x, kT);
    case F_POW_Q: return gm::powf_inrange(x, 0.25f, kT);
    case F_POW_MQ: return gm::powf_inrange(x, -0.25f, kT);
    default: return gm::atanf_ge1(x, gm::DivIeee{});
  }
}

__global__ void k_inrange(int fn, unsigned n, unsigned first, unsigned stride, unsigned* out) {
  typedef nmp::MthInRange32 M;
  nmp::stage_math_tables();
  __syncthreads();
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float x = __uint_as_float(first + i * stride);
  float r;
  switch (fn) {
    case F_EXP: r = M::exp(x); break;
    case F_LOG: r = M::log(x); break;
    case F_POW_Q: r = M::pow_q(x); break;
    case F_POW_MQ: r = M::pow_mq(x); break;
    default: r = M::atan(x); break;
  }
  out[i] = __float_as_uint(r);
}

extern "C" int li_sweep(int fn, unsigned first, unsigned long long count, unsigned stride,
                        int threads, unsigned long long* res) {
  if (fn < 0 || fn >= F_N || threads <= 0 || threads > 1024) return -1;
  const unsigned CH = 1u << 22;
  unsigned* d = nullptr;
  if (hipMalloc(&d, CH * sizeof(unsigned)) != hipSuccess) return -2;
  std::vector<unsigned> dev(CH);
  for (int k = 0; k < 5; ++k) res[k] = 0;
  int rc = 0;
  for (unsigned long long done = 0; done < count && rc == 0; done += CH) {
    const unsigned n = (unsigned)(count - done < CH ? count - done : CH);
    const unsigned f0 = first + (unsigned)(done * stride);
    hipLaunchKernelGGL(k_inrange, dim3((n + threads - 1) / threads), dim3(threads), 0, 0, fn, n, f0,
                       stride, d);
    if (hipGetLastError() != hipSuccess ||
        hipMemcpy(dev.data(), d, n * sizeof(unsigned), hipMemcpyDeviceToHost) != hipSuccess) {
      rc = -4;
      break;
    }
    for (unsigned i = 0; i < n; ++i) {
      const unsigned u = f0 + i * stride;
      const unsigned h = gm::asuint(host_fn(fn, gm::asfloat(u)));
      if (h != dev[i]) {
        if (!res[1]) {
          res[2] = u;
          res[3] = dev[i];
          res[4] = h;
        }
        res[1]++;
      }
    }
    res[0] += n;
  }
  (void)hipFree(d);
  return rc;
}
