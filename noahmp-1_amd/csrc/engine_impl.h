// The engine as its own translation units see it: the handle behind the C
// ABI's opaque nmp_engine, and what every entry (include/noahmp_engine.h)
// does before and around its launch.  An entry lives in the file of its
// kernel and refuses in this order, touching no device before the last step:
//   1. a NULL engine, bad counts or strides          NMP_E_ARG
//   2. nothing to do (ncol == 0, as a rule)          NMP_OK
//   3. NULL pointers                                 NMP_E_ARG
//   4. the engine's device cannot be made current    NMP_E_DEVICE
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <mutex>

#include "dev_params.h"
#include "noahmp_engine.h"

struct nmp_engine {
  int device;
  int precision;
  int math;  // 0 = reference-rounded transcendentals (parity), 1 = fast (fp32 only)
  int cpw;   // columns per wave: 8..64, or 0 = chosen per launch from ncol
  int simds; // SIMDs on the device (CUs x 4)
  int os;    // compiled option set matching opts (sflx_kernel.hip kOptionSet), 0 = none
  int variant;  // NMP_LAUNCH_AUTO | SMALL | FULL: occupancy instantiation per launch
  nmp_options opts;
  nmp::DevParams* dparams;
  // the synchronous host entries (nmp_sflx_columns, nmp_*_host): a private
  // non-blocking stream, so they neither wait for nor stall the caller's
  // streams, and device scratch kept across calls (grown on demand), so a
  // scalar call from a Fortran loop pays no allocation
  hipStream_t hstream;
  char* scratch;
  size_t scratch_bytes;
  // the host entries share hstream and scratch: one at a time per engine
  // (two threads calling them on one engine are serialized here); the
  // two-pass reductions hold it while their passes are enqueued back to back
  std::mutex host_mu;
};

namespace nmp {

// largest column stride: the kernels form a column's byte offset from a
// field's base in 32 bits (2^29 columns of 8-byte fp64 values = 4 GiB)
constexpr int64_t kMaxColumns = int64_t(1) << 29;

// a leading dimension that does not hold ncol columns, or past the limit
inline bool bad_ld(int64_t ld, int64_t ncol) { return ld < ncol || ld >= kMaxColumns; }

inline int rc_of(hipError_t e) { return e == hipSuccess ? NMP_OK : NMP_E_DEVICE; }

// the engine's device made current for the calling thread
inline int ensure_device(int dev) {
  int cur = -1;
  if (hipGetDevice(&cur) != hipSuccess) return NMP_E_DEVICE;
  if (cur != dev && hipSetDevice(dev) != hipSuccess) return NMP_E_DEVICE;
  return NMP_OK;
}

// One lane per column: `kernel` over ncol columns in workgroups of 256 on
// `stream` (nothing is launched for no column), every argument converted to
// the kernel's own parameter type -- a void* block to the T* the kernel takes.
template <class... P, class... A>
int launch_cols(int64_t ncol, void* stream, void (*kernel)(P...), A... args) {
  static_assert(sizeof...(P) == sizeof...(A), "one argument per kernel parameter");
  if (ncol <= 0) return NMP_OK;
  hipLaunchKernelGGL(kernel, dim3((unsigned)((ncol + 255) / 256)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), static_cast<P>(args)...);
  return rc_of(hipGetLastError());
}

// The same for a kernel of the engine precision: its float instantiation for
// precision 4, its double one otherwise.
template <class... PF, class... PD, class... A>
int launch_cols(int precision, int64_t ncol, void* stream, void (*kernel_f)(PF...),
                void (*kernel_d)(PD...), A... args) {
  return precision == 4 ? launch_cols(ncol, stream, kernel_f, args...)
                        : launch_cols(ncol, stream, kernel_d, args...);
}

// csrc/routines.hip: the reference's public routines frh2o / calhum over n
// elements (device pointers, engine precision; math 0 = the fp32 "ref" policy)
hipError_t launch_frh2o(int precision, int math, const DevParams* P, int64_t n,
                        const int32_t* sltyp, const void* tkelv, const void* smc, const void* sh2o,
                        void* out, int32_t* status, hipStream_t stream);
hipError_t launch_calhum(int precision, int math, int64_t n, const void* sfctmp,
                         const void* sfcprs, void* q2sat, void* dqsdt2, hipStream_t stream);

}  // namespace nmp
