// Test-side library (tests/lib/libnmp_libm_outloop.so and, built with
// -DNMP_COUNT_FALLBACK, libnmp_libm_outloop_count.so;
// tests/test_gpu_libm_outloop.py): the device build of nmp::MthGuard32, the
// math policy of the fp32 libm calls outside the Newton loops, after
// stage_math_tables(), against the host build of the full functions of the same
// header (gm::expf, logf, log10f, powf, powf_pair), bit for bit.
//
//   lo_eval(fn, n, threads, x, y, y2, active, out, out2, host, host2, counts)
// runs function fn on the n inputs (float bit patterns; y for pow and pow_pair,
// y2 for pow_pair) in blocks of `threads`.  Where `active` is non-null only the
// lanes with active[i] != 0 make the call, under a divergent branch, and only
// they write out[i] (and out2[i]): the caller pre-fills both.  host / host2
// receive the host build's results for every i.  counts[0..1]: the counting
// build's wave-level calls and those that took the full function (zero in the
// plain build).  Returns 0, or a negative number on a HIP error.
#include <hip/hip_runtime.h>

#include "sflx_math.h"

enum { F_EXP = 0, F_LOG, F_LOG10, F_POW, F_POW_PAIR, F_N };

static const gm::GmTables kT = {GM_EXP2F_TAB, GM_LOGF_TAB, GM_POWF_TAB};

__global__ void k_outloop(int fn, unsigned n, const unsigned* x, const unsigned* y,
                          const unsigned* y2, const unsigned char* active, unsigned* out,
                          unsigned* out2) {
  typedef nmp::GuardMth<float, true>::type M;
  nmp::stage_math_tables();
  __syncthreads();
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  // every lane's operands are in registers before the branch: an inactive
  // lane's stay there, whatever they hold
  const float xv = __uint_as_float(x[i]), yv = __uint_as_float(y[i]), y2v = __uint_as_float(y2[i]);
  if (!active || active[i]) {
    float r, r2 = 0.0f;
    switch (fn) {
      case F_EXP: r = M::exp(xv); break;
      case F_LOG: r = M::log(xv); break;
      case F_LOG10: r = M::log10(xv); break;
      case F_POW: r = M::pow(xv, yv); break;
      default: nmp::pow_pair<float, true, M>(xv, yv, y2v, r, r2); break;
    }
    out[i] = __float_as_uint(r);
    if (fn == F_POW_PAIR) out2[i] = __float_as_uint(r2);
  }
}

#define LO_OK(e) ((e) == hipSuccess)

extern "C" int lo_eval(int fn, unsigned n, int threads, const unsigned* x, const unsigned* y,
                       const unsigned* y2, const unsigned char* active, unsigned* out,
                       unsigned* out2, unsigned* host, unsigned* host2, unsigned long long* counts) {
  if (fn < 0 || fn >= F_N || n == 0 || threads <= 0 || threads > 1024 || threads % 64) return -1;
  const size_t nb = (size_t)n * sizeof(unsigned);
  unsigned *dx = nullptr, *dy = nullptr, *dy2 = nullptr, *dout = nullptr, *dout2 = nullptr;
  unsigned char* dact = nullptr;
  int rc = 0;
  if (!LO_OK(hipMalloc(&dx, nb)) || !LO_OK(hipMalloc(&dy, nb)) || !LO_OK(hipMalloc(&dy2, nb)) ||
      !LO_OK(hipMalloc(&dout, nb)) || !LO_OK(hipMalloc(&dout2, nb)) ||
      (active && !LO_OK(hipMalloc(&dact, n))))
    rc = -2;
  if (!rc && (!LO_OK(hipMemcpy(dx, x, nb, hipMemcpyHostToDevice)) ||
              !LO_OK(hipMemcpy(dy, y, nb, hipMemcpyHostToDevice)) ||
              !LO_OK(hipMemcpy(dy2, y2, nb, hipMemcpyHostToDevice)) ||
              !LO_OK(hipMemcpy(dout, out, nb, hipMemcpyHostToDevice)) ||
              !LO_OK(hipMemcpy(dout2, out2, nb, hipMemcpyHostToDevice)) ||
              (active && !LO_OK(hipMemcpy(dact, active, n, hipMemcpyHostToDevice)))))
    rc = -3;
  counts[0] = counts[1] = 0;
#ifdef NMP_COUNT_FALLBACK
  const unsigned int zero[64] = {0};
  if (!rc && !LO_OK(hipMemcpyToSymbol(HIP_SYMBOL(nmp::nmp_fb_reason), zero, sizeof(zero)))) rc = -5;
#endif
  if (!rc) {
    hipLaunchKernelGGL(k_outloop, dim3((n + threads - 1) / threads), dim3(threads), 0, 0, fn, n, dx,
                       dy, dy2, dact, dout, dout2);
    if (!LO_OK(hipGetLastError()) || !LO_OK(hipMemcpy(out, dout, nb, hipMemcpyDeviceToHost)) ||
        !LO_OK(hipMemcpy(out2, dout2, nb, hipMemcpyDeviceToHost)))
      rc = -4;
  }
#ifdef NMP_COUNT_FALLBACK
  unsigned int why[64];
  if (!rc) {
    if (!LO_OK(hipMemcpyFromSymbol(why, HIP_SYMBOL(nmp::nmp_fb_reason), sizeof(why)))) rc = -5;
    else counts[0] = why[40 + 2 * fn], counts[1] = why[41 + 2 * fn];
  }
#endif
  (void)hipFree(dx), (void)hipFree(dy), (void)hipFree(dy2);
  (void)hipFree(dout), (void)hipFree(dout2), (void)hipFree(dact);
  for (unsigned i = 0; i < n; ++i) {
    const float xv = gm::asfloat(x[i]), yv = gm::asfloat(y[i]), y2v = gm::asfloat(y2[i]);
    float r, r2 = 0.0f;
    switch (fn) {
      case F_EXP: r = gm::expf(xv, kT); break;
      case F_LOG: r = gm::logf(xv, kT); break;
      case F_LOG10: r = gm::log10f(xv, kT); break;
      case F_POW: r = gm::powf(xv, yv, kT); break;
      default: gm::powf_pair(xv, yv, y2v, kT, r, r2); break;
    }
    host[i] = gm::asuint(r);
    host2[i] = gm::asuint(r2);
  }
  return rc;
}

extern "C" int lo_counting(void) {
#ifdef NMP_COUNT_FALLBACK
  return 1;
#else
  return 0;
#endif
}
