// TEST LIBRARY -- per-routine checks of the step kernel's device routines.
//
// The step kernel (noahmp-1_amd/csrc/sflx_kernel.hip) is one fused launch, so
// a bit difference can otherwise only be seen end to end.  This library runs
// single device routines from csrc/sflx_routines.h -- the SAME code the
// kernel inlines, in the default fp32 "ref" math -- over arrays of inputs:
//   esat   func.f90:3692-3736   saturation vapour pressure and derivatives
//   tdfcnd func.f90:1500-1595   soil thermal conductivity
//   frh2o  func.f90:4494-4598   supercooled soil water (Newton + Flerchinger)
//   rosr12 func.f90:4240-4288   tridiagonal (Thomas) solve on layers kt..6
//   dv     the fp64 Newton-loop division (csrc/sflx_math.h), against IEEE `/`
//   sqrt_normal32 / DivFast32: the short fp32 sqrt and division of the
//          range-proven sites, exhaustively / at the edges of their exact region
//   math   the exact float libm (csrc/glibc_math.h) through Mth<float, true> and
//          pow_pair, against the host compilation of the same header (sweep and
//          list entries, tests/test_gpu_math.py); Mth<double, true>'s functions
//          as a list entry (tests/test_gpu_math64.py, against mpmath goldens)
// tests/test_gpu_routines.py compares them bit for bit with the oracle's C
// restatement of each routine, and frh2o also with the reference's own
// (public) frh2o.  Built by __graft_entry__.build() into tests/lib/.
#include <hip/hip_runtime.h>

#include <vector>

#include "sflx_routines.h"

namespace {

using nmp::DevParams;

__global__ void k_esat(int n, const float* t, float* out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float esw, esi, desw, desi;
  nmp::esat<float>(t[i], esw, esi, desw, desi);
  out[4 * i] = esw;
  out[4 * i + 1] = esi;
  out[4 * i + 2] = desw;
  out[4 * i + 3] = desi;
}

__global__ void k_tdfcnd(const DevParams* P, int n, const int* sltyp, const float* smc,
                         const float* sh2o, float* out) {
  nmp::stage_math_tables();
  __syncthreads();
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  out[i] = nmp::tdfcnd<float, true>(P->soil[sltyp[i] - 1], smc[i], sh2o[i]);
}

__global__ void k_frh2o(const DevParams* P, int n, const int* sltyp, const float* tk,
                        const float* smc, const float* sh2o, float* out, int* status) {
  nmp::stage_math_tables();
  __syncthreads();
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const nmp::SoilRec& S = P->soil[sltyp[i] - 1];
  int st = 0;
  out[i] = nmp::frh2o<float, true>((float)S.smcmax, (float)S.psisat, (float)S.bexp, tk[i], smc[i],
                                   sh2o[i], st);
  status[i] = st;
}

// one 7-layer system per thread: a, b, c, d in, p (solution) and delta out
__global__ void k_rosr12(int n, const int* kt, const float* a, const float* b, float* c,
                         const float* d, float* p, float* delta) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float pa[7], aa[7], bb[7], cc[7], dd[7], de[7];
#pragma unroll
  for (int k = 0; k < 7; ++k) {
    aa[k] = a[7 * i + k];
    bb[k] = b[7 * i + k];
    cc[k] = c[7 * i + k];
    dd[k] = d[7 * i + k];
    pa[k] = 0.0f;
    de[k] = 0.0f;
  }
  nmp::rosr12<float, 7>(pa, aa, bb, cc, dd, de, kt[i]);
#pragma unroll
  for (int k = 0; k < 7; ++k) {
    p[7 * i + k] = pa[k];
    delta[7 * i + k] = de[k];
    c[7 * i + k] = cc[k];  // intent(inout) in the reference
  }
}

__global__ void k_dv64(int n, const double* a, const double* b, double* q, double* ieee) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  q[i] = nmp::dv<double>(a[i], b[i]);
  ieee[i] = a[i] / b[i];
}

// the range-proven short sqrt (sflx_math.h sqrt_normal32) beside IEEE sqrtf
__global__ void k_sqrt32(int n, const float* x, float* s, float* ieee) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  s[i] = nmp::sqrt_normal32(x[i]);
  ieee[i] = ::sqrtf(x[i]);
}

// Exhaustive sqrt check: every bit pattern u in [lo, hi] (a grid-stride loop),
// sqrt_normal32 against the device's IEEE sqrtf and against the double square
// root rounded to float (correctly rounded: 53 >= 2*24 + 2 bits).  Mismatches
// are counted per thread and added once; the smallest mismatching pattern is
// kept.
__global__ void k_sqrt32_all(unsigned lo, unsigned hi, unsigned long long* bad, unsigned* first) {
  const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t nthr = (uint64_t)gridDim.x * blockDim.x;
  unsigned long long n = 0;
  for (uint64_t u = lo + tid; u <= hi; u += nthr) {
    const float x = __uint_as_float((unsigned)u);
    const unsigned s = __float_as_uint(nmp::sqrt_normal32(x));
    const unsigned w = __float_as_uint(::sqrtf(x));
    const unsigned d = __float_as_uint((float)::sqrt((double)x));
    if (s != w || s != d) {
      ++n;
      atomicMin(first, (unsigned)u);
    }
  }
  if (n) atomicAdd(bad, n);
}

// DivFast32 at the edges of its exact region (sflx_math.h and
// tools/div_proof.py: |b| in [2^-126, 2^126], a = 0 or |a| >= 2^-102, |a/b| in
// [2^-126, 2^126]).  Operands
// a = +-(1 + ia/2^23) 2^ea, b = (1 + ib/2^23) 2^eb for ia over [0, 2^23) in
// steps of sa and ib over [0, 2^23) in steps of sb (offsets oa, ob); pairs
// whose IEEE quotient lies outside [2^-126, 2^126] are outside the region:
// not counted in cnt[0]/cnt[1], but their mismatches are counted in cnt[2]
// (above 2^126 the product a*r can round past FLT_MAX and the short sequence
// then differs, which is why the proof's region stops at 2^126).  Each thread
// takes one ib value and a chunk of 2^14 consecutive ia steps.
// cnt[0] pairs checked, cnt[1] mismatches (short sequence vs IEEE a/b).
constexpr unsigned kDivChunk = 1u << 14;
__global__ void k_div32_edge(int ea, int eb, unsigned sa, unsigned oa, unsigned sb, unsigned ob,
                             unsigned nchunk, unsigned long long* cnt, unsigned* first) {
  const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t ib = ob + (k / nchunk) * (uint64_t)sb;
  if (ib >= (1u << 23)) return;
  const float b = ldexpf(__uint_as_float(0x3f800000u | (unsigned)ib), eb);
  const nmp::DivFast32 d;
  const nmp::Recip<float> R = d.rec(b);
  unsigned long long n = 0, nb = 0, nout = 0;
  const uint64_t i0 = oa + (k % nchunk) * (uint64_t)kDivChunk * sa;
  for (uint64_t j = 0, ia = i0; j < kDivChunk && ia < (1u << 23); ++j, ia += sa) {
    const float m = __uint_as_float(0x3f800000u | (unsigned)ia);
    const float a = ldexpf((ia & 1) ? -m : m, ea);
    const float w = a / b;
    const float aw = fabsf(w);
    if (!(aw >= 0x1p-126f && aw <= 0x1p126f)) {
      if (aw <= 3.40282347e38f && __float_as_uint(d.div(a, R)) != __float_as_uint(w)) ++nout;
      continue;
    }
    ++n;
    if (__float_as_uint(d.div(a, R)) != __float_as_uint(w)) {
      ++nb;
      atomicMin(first, (unsigned)ib);
    }
  }
  if (n) atomicAdd(&cnt[0], n);
  if (nb) atomicAdd(&cnt[1], nb);
  if (nout) atomicAdd(&cnt[2], nout);
}

// ---- the math primitives on their own ---------------------------------------
// Function ids shared by the fp32 and fp64 entries below.
enum MathFn {
  M_EXP = 0, M_EXP2, M_LOG, M_LOG10, M_TANH, M_ATAN, M_TAN, M_ACOS, M_COS,
  M_EXPM1_OR_SQRT,  // fp32: gm::expm1f (tanhf's helper); fp64: Mth::sqrt
  M_POW, M_POW_Q, M_POW_MQ, M_POW_PAIR, M_NFN
};

// fp32: the exact float libm (csrc/glibc_math.h) as the step kernel calls it,
// tables staged in LDS by the workgroup, through Mth<float, true> and pow_pair
using M32 = nmp::Mth<float, true>;
template <int FN>
__device__ __forceinline__ void m32_dev(float x, float y1, float y2, float& r1, float& r2) {
  r2 = 0.0f;
  if constexpr (FN == M_EXP) r1 = M32::exp(x);
  else if constexpr (FN == M_EXP2) r1 = M32::exp2(x);
  else if constexpr (FN == M_LOG) r1 = M32::log(x);
  else if constexpr (FN == M_LOG10) r1 = M32::log10(x);
  else if constexpr (FN == M_TANH) r1 = M32::tanh(x);
  else if constexpr (FN == M_ATAN) r1 = M32::atan(x);
  else if constexpr (FN == M_TAN) r1 = M32::tan(x);
  else if constexpr (FN == M_ACOS) r1 = M32::acos(x);
  else if constexpr (FN == M_COS) r1 = M32::cos(x);
  else if constexpr (FN == M_EXPM1_OR_SQRT) r1 = gm::expm1f(x);
  else if constexpr (FN == M_POW) r1 = M32::pow(x, y1);
  else if constexpr (FN == M_POW_Q) r1 = M32::pow_q(x);
  else if constexpr (FN == M_POW_MQ) r1 = M32::pow_mq(x);
  else nmp::pow_pair<float, true>(x, y1, y2, r1, r2);
}

// The same header as compiled for the host (the __host__ half of GM_HD), with
// a static table: the reference of the fp32 entries.  pow_q / pow_mq are by
// definition pow(x, +-0.25f).
const gm::GmTables kHostTab = {GM_EXP2F_TAB, GM_LOGF_TAB, GM_POWF_TAB};
void m32_host(int fn, float x, float y1, float y2, float& r1, float& r2) {
  r2 = 0.0f;
  switch (fn) {
    case M_EXP: r1 = gm::expf(x, kHostTab); break;
    case M_EXP2: r1 = gm::exp2f(x, kHostTab); break;
    case M_LOG: r1 = gm::logf(x, kHostTab); break;
    case M_LOG10: r1 = gm::log10f(x, kHostTab); break;
    case M_TANH: r1 = gm::tanhf(x); break;
    case M_ATAN: r1 = gm::atanf(x); break;
    case M_TAN: r1 = gm::tanf(x); break;
    case M_ACOS: r1 = gm::acosf(x); break;
    case M_COS: r1 = gm::cosf(x); break;
    case M_EXPM1_OR_SQRT: r1 = gm::expm1f(x); break;
    case M_POW: r1 = gm::powf(x, y1, kHostTab); break;
    case M_POW_Q: r1 = gm::powf(x, 0.25f, kHostTab); break;
    case M_POW_MQ: r1 = gm::powf(x, -0.25f, kHostTab); break;
    default: gm::powf_pair(x, y1, y2, kHostTab, r1, r2); break;
  }
}

// Input i is the bit pattern xs[i] (list) or, with xs null, first +
// (base + i) * stride modulo 2^32 (sweep); the exponents are y1s[i] / y2s[i]
// where those arrays are given, the scalars otherwise.  Result bits out.
template <int FN>
__global__ void k_m32(unsigned n, const unsigned* xs, const unsigned* y1s, const unsigned* y2s,
                      unsigned first, unsigned stride, unsigned long long base, float y1, float y2,
                      unsigned* o1, unsigned* o2) {
  nmp::stage_math_tables();
  __syncthreads();
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const unsigned u = xs ? xs[i] : first + (unsigned)((base + i) * stride);
  if (y1s) y1 = __uint_as_float(y1s[i]);
  if (y2s) y2 = __uint_as_float(y2s[i]);
  float r1, r2;
  m32_dev<FN>(__uint_as_float(u), y1, y2, r1, r2);
  o1[i] = __float_as_uint(r1);
  if (FN == M_POW_PAIR) o2[i] = __float_as_uint(r2);
}

using K32 = void (*)(unsigned, const unsigned*, const unsigned*, const unsigned*, unsigned,
                     unsigned, unsigned long long, float, float, unsigned*, unsigned*);
K32 m32_kernel(int fn) {
  static const K32 k[M_NFN] = {k_m32<0>, k_m32<1>, k_m32<2>,  k_m32<3>,  k_m32<4>,
                               k_m32<5>, k_m32<6>, k_m32<7>,  k_m32<8>,  k_m32<9>,
                               k_m32<10>, k_m32<11>, k_m32<12>, k_m32<13>};
  return k[fn];
}

// fp64: Mth<double, true> and pow_pair<double, true>, the fp64 engine's math
using M64 = nmp::Mth<double, true>;
template <int FN>
__global__ void k_m64(unsigned n, const double* xs, const double* y1s, const double* y2s,
                      double* o1, double* o2) {
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double x = xs[i], y1 = y1s ? y1s[i] : 0.0, y2 = y2s ? y2s[i] : 0.0;
  double r1, r2 = 0.0;
  if constexpr (FN == M_EXP) r1 = M64::exp(x);
  else if constexpr (FN == M_EXP2) r1 = M64::exp2(x);
  else if constexpr (FN == M_LOG) r1 = M64::log(x);
  else if constexpr (FN == M_LOG10) r1 = M64::log10(x);
  else if constexpr (FN == M_TANH) r1 = M64::tanh(x);
  else if constexpr (FN == M_ATAN) r1 = M64::atan(x);
  else if constexpr (FN == M_TAN) r1 = M64::tan(x);
  else if constexpr (FN == M_ACOS) r1 = M64::acos(x);
  else if constexpr (FN == M_COS) r1 = M64::cos(x);
  else if constexpr (FN == M_EXPM1_OR_SQRT) r1 = M64::sqrt(x);
  else if constexpr (FN == M_POW) r1 = M64::pow(x, y1);
  else if constexpr (FN == M_POW_Q) r1 = M64::pow_q(x);
  else if constexpr (FN == M_POW_MQ) r1 = M64::pow_mq(x);
  else nmp::pow_pair<double, true>(x, y1, y2, r1, r2);
  o1[i] = r1;
  if (FN == M_POW_PAIR) o2[i] = r2;
}

using K64 = void (*)(unsigned, const double*, const double*, const double*, double*, double*);
K64 m64_kernel(int fn) {
  static const K64 k[M_NFN] = {k_m64<0>, k_m64<1>, k_m64<2>,  k_m64<3>,  k_m64<4>,
                               k_m64<5>, k_m64<6>, k_m64<7>,  k_m64<8>,  k_m64<9>,
                               k_m64<10>, k_m64<11>, k_m64<12>, k_m64<13>};
  return k[fn];
}

bool math_args_ok(int fn, int threads) {
  return fn >= 0 && fn < M_NFN && threads >= 1 && threads <= 1024;
}
unsigned f2u(float f) { return __builtin_bit_cast(unsigned, f); }
float u2f(unsigned u) { return __builtin_bit_cast(float, u); }
// the checkers' equality: equal bits, or both NaN
bool same32(unsigned a, unsigned b) {
  return a == b || ((a & 0x7fffffffu) > 0x7f800000u && (b & 0x7fffffffu) > 0x7f800000u);
}

// host helpers: device copies in, one launch, results out (synchronous)
struct Dev {
  std::vector<void*> ptrs;
  ~Dev() {
    for (void* p : ptrs) (void)hipFree(p);
  }
  template <class X>
  X* in(const X* h, size_t n) {
    void* d = nullptr;
    if (hipMalloc(&d, n * sizeof(X) + 16) != hipSuccess) return nullptr;
    ptrs.push_back(d);
    if (h && hipMemcpy(d, h, n * sizeof(X), hipMemcpyHostToDevice) != hipSuccess) return nullptr;
    return static_cast<X*>(d);
  }
};

int finish(Dev&, float* hout, const float* dout, size_t n) {
  if (hipDeviceSynchronize() != hipSuccess) return -4;
  return hipMemcpy(hout, dout, n * sizeof(float), hipMemcpyDeviceToHost) == hipSuccess ? 0 : -4;
}

const DevParams* dev_params(Dev& D, const nmp_params* p) {
  DevParams h{};
  nmp::pack_dev_params(*p, h);
  return D.in(&h, 1);
}

}  // namespace

extern "C" {

int rt_esat(int n, const float* t, float* out4) {
  Dev D;
  const float* dt = D.in(t, n);
  float* dout = D.in<float>(nullptr, 4 * (size_t)n);
  if (!dt || !dout) return -4;
  hipLaunchKernelGGL(k_esat, dim3((n + 255) / 256), dim3(256), 0, 0, n, dt, dout);
  return finish(D, out4, dout, 4 * (size_t)n);
}

int rt_tdfcnd(const nmp_params* p, int n, const int* sltyp, const float* smc, const float* sh2o,
              float* out) {
  Dev D;
  const DevParams* P = dev_params(D, p);
  const int* ds = D.in(sltyp, n);
  const float *dm = D.in(smc, n), *dh = D.in(sh2o, n);
  float* dout = D.in<float>(nullptr, n);
  if (!P || !ds || !dm || !dh || !dout) return -4;
  hipLaunchKernelGGL(k_tdfcnd, dim3((n + 255) / 256), dim3(256), 0, 0, P, n, ds, dm, dh, dout);
  return finish(D, out, dout, n);
}

int rt_frh2o(const nmp_params* p, int n, const int* sltyp, const float* tk, const float* smc,
             const float* sh2o, float* out, int* status) {
  Dev D;
  const DevParams* P = dev_params(D, p);
  const int* ds = D.in(sltyp, n);
  const float *dt = D.in(tk, n), *dm = D.in(smc, n), *dh = D.in(sh2o, n);
  float* dout = D.in<float>(nullptr, n);
  int* dst = D.in<int>(nullptr, n);
  if (!P || !ds || !dt || !dm || !dh || !dout || !dst) return -4;
  hipLaunchKernelGGL(k_frh2o, dim3((n + 255) / 256), dim3(256), 0, 0, P, n, ds, dt, dm, dh, dout,
                     dst);
  if (finish(D, out, dout, n) != 0) return -4;
  return hipMemcpy(status, dst, n * sizeof(int), hipMemcpyDeviceToHost) == hipSuccess ? 0 : -4;
}

int rt_rosr12(int n, const int* kt, const float* a, const float* b, float* c, const float* d,
              float* p, float* delta) {
  Dev D;
  const size_t m = 7 * (size_t)n;
  const int* dk = D.in(kt, n);
  const float *da = D.in(a, m), *db = D.in(b, m), *dd = D.in(d, m);
  float* dc = D.in(c, m);
  float *dp = D.in<float>(nullptr, m), *de = D.in<float>(nullptr, m);
  if (!dk || !da || !db || !dc || !dd || !dp || !de) return -4;
  hipLaunchKernelGGL(k_rosr12, dim3((n + 255) / 256), dim3(256), 0, 0, n, dk, da, db, dc, dd, dp,
                     de);
  if (finish(D, p, dp, m) != 0) return -4;
  if (hipMemcpy(c, dc, m * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) return -4;
  return hipMemcpy(delta, de, m * sizeof(float), hipMemcpyDeviceToHost) == hipSuccess ? 0 : -4;
}

int rt_dv64(int n, const double* a, const double* b, double* q, double* ieee) {
  Dev D;
  const double *da = D.in(a, n), *db = D.in(b, n);
  double *dq = D.in<double>(nullptr, n), *di = D.in<double>(nullptr, n);
  if (!da || !db || !dq || !di) return -4;
  hipLaunchKernelGGL(k_dv64, dim3((n + 255) / 256), dim3(256), 0, 0, n, da, db, dq, di);
  if (hipDeviceSynchronize() != hipSuccess) return -4;
  if (hipMemcpy(q, dq, n * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) return -4;
  return hipMemcpy(ieee, di, n * sizeof(double), hipMemcpyDeviceToHost) == hipSuccess ? 0 : -4;
}

int rt_sqrt32(int n, const float* x, float* s, float* ieee) {
  Dev D;
  const float* dx = D.in(x, n);
  float *ds = D.in<float>(nullptr, n), *di = D.in<float>(nullptr, n);
  if (!dx || !ds || !di) return -4;
  hipLaunchKernelGGL(k_sqrt32, dim3((n + 255) / 256), dim3(256), 0, 0, n, dx, ds, di);
  if (hipDeviceSynchronize() != hipSuccess) return -4;
  if (hipMemcpy(s, ds, n * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) return -4;
  return hipMemcpy(ieee, di, n * sizeof(float), hipMemcpyDeviceToHost) == hipSuccess ? 0 : -4;
}

// mismatches of sqrt_normal32 over every bit pattern in [lo, hi]; *first = the
// smallest mismatching pattern (0xffffffff if none)
int rt_sqrt32_all(unsigned lo, unsigned hi, unsigned long long* bad, unsigned* first) {
  Dev D;
  unsigned long long* db = D.in<unsigned long long>(nullptr, 1);
  unsigned* df = D.in<unsigned>(nullptr, 1);
  if (!db || !df) return -4;
  const unsigned none = 0xffffffffu;
  if (hipMemset(db, 0, sizeof(*db)) != hipSuccess ||
      hipMemcpy(df, &none, sizeof(none), hipMemcpyHostToDevice) != hipSuccess)
    return -4;
  hipLaunchKernelGGL(k_sqrt32_all, dim3(65536), dim3(256), 0, 0, lo, hi, db, df);
  if (hipDeviceSynchronize() != hipSuccess) return -4;
  if (hipMemcpy(bad, db, sizeof(*db), hipMemcpyDeviceToHost) != hipSuccess) return -4;
  return hipMemcpy(first, df, sizeof(*df), hipMemcpyDeviceToHost) == hipSuccess ? 0 : -4;
}

// DivFast32 vs IEEE division on one exponent pair (k_div32_edge); cnt3 =
// {pairs in the region, mismatches there, mismatches outside it}
int rt_div32_edge(int ea, int eb, unsigned sa, unsigned oa, unsigned sb, unsigned ob,
                  unsigned long long* cnt3, unsigned* first) {
  if (sa == 0 || sb == 0 || oa >= sa || ob >= sb) return -1;
  Dev D;
  unsigned long long* dc = D.in<unsigned long long>(nullptr, 3);
  unsigned* df = D.in<unsigned>(nullptr, 1);
  if (!dc || !df) return -4;
  const unsigned none = 0xffffffffu;
  if (hipMemset(dc, 0, 3 * sizeof(*dc)) != hipSuccess ||
      hipMemcpy(df, &none, sizeof(none), hipMemcpyHostToDevice) != hipSuccess)
    return -4;
  const uint64_t nbv = ((1u << 23) - ob + sb - 1) / sb;               // b values
  const uint64_t nav = ((1u << 23) - oa + sa - 1) / sa;               // a values
  const unsigned nchunk = (unsigned)((nav + kDivChunk - 1) / kDivChunk);
  const uint64_t nthr = nbv * nchunk;
  hipLaunchKernelGGL(k_div32_edge, dim3((unsigned)((nthr + 255) / 256)), dim3(256), 0, 0, ea, eb,
                     sa, oa, sb, ob, nchunk, dc, df);
  if (hipDeviceSynchronize() != hipSuccess) return -4;
  if (hipMemcpy(cnt3, dc, 3 * sizeof(*dc), hipMemcpyDeviceToHost) != hipSuccess) return -4;
  return hipMemcpy(first, df, sizeof(*df), hipMemcpyDeviceToHost) == hipSuccess ? 0 : -4;
}

// fp32 math, sweep form: function `fn` (MathFn) over the `count` bit patterns
// first, first + stride, ... (modulo 2^32), exponents y1 (pow) or y1, y2
// (pow_pair), launched with `threads` per block; the device's result bits
// against the host compilation of the same header.  dom120 != 0 leaves inputs
// that are not |x| < 120 out of the comparison (gm::cosf / gm::tanf restate
// glibc only there).  res7 = {inputs compared, mismatching results, first
// mismatching input pattern, its device bits, its host bits, host results that
// are subnormal and nonzero, which result of a pair (0 / 1) mismatched}.
int rt_math32_sweep(int fn, unsigned first, unsigned long long count, unsigned stride, float y1,
                    float y2, int dom120, int threads, unsigned long long* res7) {
  if (!math_args_ok(fn, threads) || count == 0 || count > (1ull << 32)) return -1;
  constexpr unsigned kChunk = 1u << 22;
  const bool pair = fn == M_POW_PAIR;
  Dev D;
  const size_t cap = count < kChunk ? (size_t)count : kChunk;
  unsigned *d1 = D.in<unsigned>(nullptr, cap), *d2 = D.in<unsigned>(nullptr, cap);
  if (!d1 || !d2) return -4;
  std::vector<unsigned> g1(cap), g2(cap), h1(cap), h2(cap);
  for (int k = 0; k < 7; ++k) res7[k] = 0;
  const K32 kern = m32_kernel(fn);
  for (unsigned long long base = 0; base < count; base += kChunk) {
    const unsigned n = (unsigned)(count - base < kChunk ? count - base : kChunk);
    hipLaunchKernelGGL(kern, dim3((n + threads - 1) / threads), dim3(threads), 0, 0, n,
                       (const unsigned*)nullptr, (const unsigned*)nullptr, (const unsigned*)nullptr,
                       first, stride, base, y1, y2, d1, d2);
    if (hipGetLastError() != hipSuccess) return -4;
    // the host's results while the device works on its own
    for (unsigned i = 0; i < n; ++i) {
      float r1, r2;
      m32_host(fn, u2f(first + (unsigned)((base + i) * stride)), y1, y2, r1, r2);
      h1[i] = f2u(r1);
      h2[i] = f2u(r2);
    }
    if (hipDeviceSynchronize() != hipSuccess) return -4;
    if (hipMemcpy(g1.data(), d1, n * sizeof(unsigned), hipMemcpyDeviceToHost) != hipSuccess)
      return -4;
    if (pair && hipMemcpy(g2.data(), d2, n * sizeof(unsigned), hipMemcpyDeviceToHost) != hipSuccess)
      return -4;
    for (unsigned i = 0; i < n; ++i) {
      const unsigned u = first + (unsigned)((base + i) * stride);
      if (dom120 && !(fabsf(u2f(u)) < 120.0f)) continue;
      ++res7[0];
      for (int j = 0; j < (pair ? 2 : 1); ++j) {
        const unsigned g = j ? g2[i] : g1[i], h = j ? h2[i] : h1[i];
        if ((h & 0x7f800000u) == 0 && (h & 0x007fffffu) != 0) ++res7[5];
        if (same32(g, h)) continue;
        if (res7[1]++ == 0) {
          res7[2] = u;
          res7[3] = g;
          res7[4] = h;
          res7[6] = j;
        }
      }
    }
  }
  return 0;
}

// fp32 math, list form: inputs x[i] (and y1[i], y2[i] where the function takes
// them; null otherwise) as bit patterns in, device bits and host bits out
// (dev2 / host2: pow_pair's second result, null otherwise)
int rt_math32_list(int fn, int n, const unsigned* x, const unsigned* y1, const unsigned* y2,
                   int threads, unsigned* dev1, unsigned* host1, unsigned* dev2, unsigned* host2) {
  if (!math_args_ok(fn, threads) || n <= 0) return -1;
  const bool pair = fn == M_POW_PAIR;
  if ((fn >= M_POW && fn != M_POW_Q && fn != M_POW_MQ && !y1) || (pair && (!y2 || !dev2 || !host2)))
    return -1;
  Dev D;
  const unsigned* dx = D.in(x, n);
  const unsigned* dy1 = y1 ? D.in(y1, n) : nullptr;
  const unsigned* dy2 = y2 ? D.in(y2, n) : nullptr;
  unsigned *d1 = D.in<unsigned>(nullptr, n), *d2 = D.in<unsigned>(nullptr, n);
  if (!dx || (y1 && !dy1) || (y2 && !dy2) || !d1 || !d2) return -4;
  hipLaunchKernelGGL(m32_kernel(fn), dim3(((unsigned)n + threads - 1) / threads), dim3(threads), 0,
                     0, (unsigned)n, dx, dy1, dy2, 0u, 0u, 0ull, 0.0f, 0.0f, d1, d2);
  if (hipGetLastError() != hipSuccess) return -4;
  for (int i = 0; i < n; ++i) {
    float r1, r2;
    m32_host(fn, u2f(x[i]), y1 ? u2f(y1[i]) : 0.0f, y2 ? u2f(y2[i]) : 0.0f, r1, r2);
    host1[i] = f2u(r1);
    if (pair) host2[i] = f2u(r2);
  }
  if (hipDeviceSynchronize() != hipSuccess) return -4;
  if (hipMemcpy(dev1, d1, n * sizeof(unsigned), hipMemcpyDeviceToHost) != hipSuccess) return -4;
  if (pair && hipMemcpy(dev2, d2, n * sizeof(unsigned), hipMemcpyDeviceToHost) != hipSuccess)
    return -4;
  return 0;
}

// fp64 math, list form: Mth<double, true> (fn 9 = sqrt) and pow_pair<double,
// true> on x[i] (, y1[i], y2[i]); the results out (out2: pow_pair's second)
int rt_math64_list(int fn, int n, const double* x, const double* y1, const double* y2, int threads,
                   double* out1, double* out2) {
  if (!math_args_ok(fn, threads) || n <= 0) return -1;
  const bool pair = fn == M_POW_PAIR;
  if (((fn == M_POW || pair) && !y1) || (pair && (!y2 || !out2))) return -1;
  Dev D;
  const double* dx = D.in(x, n);
  const double* dy1 = y1 ? D.in(y1, n) : nullptr;
  const double* dy2 = y2 ? D.in(y2, n) : nullptr;
  double *d1 = D.in<double>(nullptr, n), *d2 = D.in<double>(nullptr, n);
  if (!dx || (y1 && !dy1) || (y2 && !dy2) || !d1 || !d2) return -4;
  hipLaunchKernelGGL(m64_kernel(fn), dim3(((unsigned)n + threads - 1) / threads), dim3(threads), 0,
                     0, (unsigned)n, dx, dy1, dy2, d1, d2);
  if (hipGetLastError() != hipSuccess) return -4;
  if (hipDeviceSynchronize() != hipSuccess) return -4;
  if (hipMemcpy(out1, d1, n * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) return -4;
  if (pair && hipMemcpy(out2, d2, n * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess)
    return -4;
  return 0;
}

}  // extern "C"
