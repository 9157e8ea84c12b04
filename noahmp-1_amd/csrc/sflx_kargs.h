// Kernel argument block shared by the launch site (engine.hip) and the
// kernel (sflx_kernel.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dev_params.h"

// workgroup size of the step kernel (256: DESIGN.md "Occupancy")
#ifndef NMP_BLOCK
#define NMP_BLOCK 256
#endif

namespace nmp {

struct Opt {
  int veg, crs, btr, run, sfc, frz, inf, rad, alb, snf, tbot, stc;
};

template <class T>
struct KArgs {
  int64_t ncol, ld;
  float zsoil[4];
  float dt, julian;
  int yearlen;
  int diag_level;
  float c_exp_m4, c_albdecay;  // host-precomputed EXP(-4.0), EXP(-0.01*DT/3600) (fp32 ref)
  Opt o;
  T* state;
  int32_t* isnow;
  const T* static_f;
  const int32_t* static_i;
  const T* forcing;
  T* diag;
  int32_t* status;
  // column re-binning (nmp_step_binned): lane i steps column order[i] when
  // order is set; cost (if set) receives each column's loop-cost key
  const int32_t* order;
  uint8_t* cost;
  // noahmp_sflx's FICEOLD argument (3 x ld), or NULL: derived from
  // SNICE/SNLIQ at step start (offline-driver convention)
  const T* ficeold;
  // columns stepped per 64-lane wave (8..64, a multiple of 8): below 64 the
  // launch spreads a small column set over more waves (small-N latency hiding)
  int cpw;
#ifdef NMP_TRUNC_RUNTIME
  int trunc_at;  // (probe builds) phase mark the step returns at (sflx_kernel.hip)
#endif
};

template <class T, bool R>
hipError_t launch_sflx(const DevParams* dparams, const KArgs<T>& a, hipStream_t stream,
                       bool small, int os);

}  // namespace nmp
