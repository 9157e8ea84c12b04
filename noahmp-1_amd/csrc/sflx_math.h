// Arithmetic helpers for the sflx kernel (device side).
//
// Transcendental policy:
//  - Mth<float, true>  "ref":  bit-exact restatements of the glibc 2.35 float
//    libm the reference's compiled physics calls (glibc_math.h: expf, exp2f,
//    logf, powf, tanhf, atanf, log10f, acosf, cosf, tanf).  Each is checked
//    against the host libm over all 2^32 inputs (powf: 26e9 samples), so the
//    kernel's elementary functions return exactly what the reference's do.
//    Their small tables (768 B) are staged per workgroup in LDS.  Default.
//  - Mth<float, false> "fast": ocml single-precision functions (<= ~1-2 ulp).
//  - Mth<double, *>:          ocml double functions (fp64 engine).
// Division and sqrt are IEEE correctly rounded in every policy (hipcc default
// -fhip-fp32-correctly-rounded-divide-sqrt), and the kernel is compiled with
// -ffp-contract=off so products and sums round exactly like the reference.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include <type_traits>

#include "glibc_math.h"
#include "vege_domain.h"

#define NMP_MATH_FN static __device__ __forceinline__

namespace nmp {

template <class T, bool REF>
struct Mth;

template <bool REF>
struct Mth<double, REF> {
  NMP_MATH_FN double exp(double x) { return ::exp(x); }
  NMP_MATH_FN double exp2(double x) { return ::exp2(x); }
  NMP_MATH_FN double log(double x) { return ::log(x); }
  NMP_MATH_FN double log10(double x) { return ::log10(x); }
  // x**y as exp(y log x): with log within E_log ulp and exp within E_exp ulp
  // (ocml's measured maxima: profiles/math64/ulp.json), t = y log x carries a
  // relative error <= (E_log + 0.5) 2^-52, which exp turns into at most
  // 2 (E_log + 0.5) |y log x| + E_exp ulp of the correctly rounded pow
  // (tests/test_gpu_math64.py asserts it): NOT "within |y log x| ulp", the
  // error grows with |y log x| and does not vanish with it.  That is still far
  // inside the fp64 path's tolerances, at about half the cost of ocml's double pow
  // (that one carries log x in double-double).  Every base in the kernel is
  // >= 0; 0**y (y > 0) -> exp(-inf) = 0 as pow gives.
  NMP_MATH_FN double pow(double x, double y) { return exp(y * ::log(x)); }
  // x**0.25 and x**(-0.25): the fp64 path is held to a tolerance, not to bits
  // (DESIGN.md "fp64"), so the fourth root is two correctly rounded square
  // roots (<= 1.5 ulp from the correctly rounded pow; the reciprocal's rounding
  // makes pow_mq <= 2.5 ulp; ~10x cheaper than ocml's double pow)
  NMP_MATH_FN double pow_q(double x) { return ::sqrt(::sqrt(x)); }
  NMP_MATH_FN double pow_mq(double x) { return 1.0 / ::sqrt(::sqrt(x)); }
  NMP_MATH_FN double tanh(double x) { return ::tanh(x); }
  NMP_MATH_FN double atan(double x) { return ::atan(x); }
  NMP_MATH_FN double tan(double x) { return ::tan(x); }
  NMP_MATH_FN double acos(double x) { return ::acos(x); }
  NMP_MATH_FN double cos(double x) { return ::cos(x); }
  static __device__ __forceinline__ double sqrt(double x) { return ::sqrt(x); }
};

template <>
struct Mth<float, false> {
  NMP_MATH_FN float exp(float x) { return ::expf(x); }
  NMP_MATH_FN float exp2(float x) { return ::exp2f(x); }
  NMP_MATH_FN float log(float x) { return ::logf(x); }
  NMP_MATH_FN float log10(float x) { return ::log10f(x); }
  NMP_MATH_FN float pow(float x, float y) { return ::powf(x, y); }
  NMP_MATH_FN float pow_q(float x) { return ::powf(x, 0.25f); }
  NMP_MATH_FN float pow_mq(float x) { return ::powf(x, -0.25f); }
  NMP_MATH_FN float tanh(float x) { return ::tanhf(x); }
  NMP_MATH_FN float atan(float x) { return ::atanf(x); }
  NMP_MATH_FN float tan(float x) { return ::tanf(x); }
  NMP_MATH_FN float acos(float x) { return ::acosf(x); }
  NMP_MATH_FN float cos(float x) { return ::cosf(x); }
  static __device__ __forceinline__ float sqrt(float x) { return ::sqrtf(x); }
};

// glibc libm tables: one __constant__ master copy, staged into LDS by every
// workgroup's prologue (stage_math_tables) before first use.
static __shared__ gm::GmTables gm_lds;
static __constant__ gm::GmTables gm_const = {GM_EXP2F_TAB, GM_LOGF_TAB, GM_POWF_TAB};

__device__ __forceinline__ void stage_math_tables() {
  constexpr int NW = sizeof(gm::GmTables) / sizeof(int4);
  static_assert(sizeof(gm::GmTables) % sizeof(int4) == 0, "table size");
  const int4* src = reinterpret_cast<const int4*>(&gm_const);
  int4* dst = reinterpret_cast<int4*>(&gm_lds);
  for (int i = threadIdx.x; i < NW; i += blockDim.x) dst[i] = src[i];
}

template <>
struct Mth<float, true> {
  NMP_MATH_FN float exp(float x) { return gm::expf(x, gm_lds); }
  NMP_MATH_FN float exp2(float x) { return gm::exp2f(x, gm_lds); }
  NMP_MATH_FN float log(float x) { return gm::logf(x, gm_lds); }
  NMP_MATH_FN float log10(float x) { return gm::log10f(x, gm_lds); }
  NMP_MATH_FN float pow(float x, float y) { return gm::powf(x, y, gm_lds); }
  // bit-exact fp32: the reference's powf itself
  NMP_MATH_FN float pow_q(float x) { return gm::powf(x, 0.25f, gm_lds); }
  NMP_MATH_FN float pow_mq(float x) { return gm::powf(x, -0.25f, gm_lds); }
  NMP_MATH_FN float tanh(float x) { return gm::tanhf(x); }
  NMP_MATH_FN float atan(float x) { return gm::atanf(x); }
  NMP_MATH_FN float tan(float x) { return gm::tanf(x); }
  NMP_MATH_FN float acos(float x) { return gm::acosf(x); }
  NMP_MATH_FN float cos(float x) { return gm::cosf(x); }
  static __device__ __forceinline__ float sqrt(float x) { return ::sqrtf(x); }
};

// x**y1 and x**y2 with one base (wdfcnd1/wdfcnd2's WDF and WCND): each equal
// to Mth::pow's result bit for bit.  The fp32 "ref" path forms powf's log2 of
// x once (gm::powf_pair, or the policy's own pow_pair: MthGuard32 below); the
// fp64 path (exp(y log x)) its log once.
template <class T, bool R, class M = Mth<T, R>>
__device__ __forceinline__ void pow_pair(T x, T y1, T y2, T& r1, T& r2) {
  if constexpr (sizeof(T) == 4 && R) {
    if constexpr (std::is_same<M, Mth<T, R>>::value)
      gm::powf_pair(x, y1, y2, gm_lds, r1, r2);
    else
      M::pow_pair(x, y1, y2, r1, r2);
    return;
  }
  if constexpr (sizeof(T) == 8) {
    const double lx = ::log(x);
    r1 = Mth<double, R>::exp(y1 * lx);
    r2 = Mth<double, R>::exp(y2 * lx);
    return;
  }
  r1 = Mth<T, R>::pow(x, y1);
  r2 = Mth<T, R>::pow(x, y2);
}

template <class T>
__device__ __forceinline__ T rmax(T a, T b) { return a > b ? a : b; }
template <class T>
__device__ __forceinline__ T rmin(T a, T b) { return a < b ? a : b; }
// x is +0: the bit pattern, so -0 is not (the tests that admit "0 or in range"
// numerators to DivFast32::divn, which needs a numerator that is never -0)
template <class T>
__device__ __forceinline__ bool is_pzero(T x) {
  if constexpr (sizeof(T) == 4) return __builtin_bit_cast(uint32_t, x) == 0u;
  else return __builtin_bit_cast(uint64_t, x) == 0ull;
}
// integer powers as the reference's compiler lowers them: sequential products
template <class T>
__device__ __forceinline__ T p2(T x) { return x * x; }
template <class T>
__device__ __forceinline__ T p3(T x) { return x * (x * x); }
template <class T>
__device__ __forceinline__ T p4(T x) { return x * p3(x); }
template <class T>
__device__ __forceinline__ T p5(T x) { return x * p4(x); }

// Division in the Newton loops (vege_flux, bare_flux, sfcdif1, ragrb).  fp32
// (the bit-exact path): IEEE `/`, except at the range-proven sites that go
// through DivFast32 (below).  fp64 (held to tolerances, not bits): the
// reciprocal from v_rcp_f64 refined by two Newton steps, times the numerator,
// plus one residual correction -- within 1 ulp of the IEEE quotient, in 9
// instructions instead of the div_scale/div_fmas/div_fixup sequence's 13, and
// without its vcc chain.  v_div_fixup_f64 gives zero, infinite and NaN
// operands (and overflow) their IEEE results and the quotient its sign.  (A
// branch back to IEEE `/` for non-finite results instead measured slower than
// plain `/`: profiles/r02/fp64_div.txt.)
// Valid range: the 1-ulp bound needs 1/b normal and the quotient and the
// residual b*q - a clear of underflow, i.e. 2^-1021 < |b| < 2^1021 and a
// normal quotient.  For |b| >= 2^1022 the reciprocal is subnormal or flushes
// and for subnormal b it overflows, so the result is NOT the IEEE quotient
// there (tests/test_gpu_routines.py pins both sides).  Every divisor these
// loops see is a physical resistance, conductance, temperature or height,
// many decades inside the range.
template <class T>
__device__ __forceinline__ T dv(T a, T b) {
  return a / b;
}
template <>
__device__ __forceinline__ double dv<double>(double a, double b) {
  double r = __builtin_amdgcn_rcp(b);
  double e = __builtin_fma(-b, r, 1.0);
  r = __builtin_fma(r, e, r);
  e = __builtin_fma(-b, r, 1.0);
  r = __builtin_fma(r, e, r);
  double q = a * r;
  e = __builtin_fma(-b, q, a);
  q = __builtin_fma(e, r, q);
  return __builtin_amdgcn_div_fixup(q, b, a);
}

// ---------------------------------------------------------------------------
// Division policies of the canopy Newton loop (vege_flux, with its sfcdif1 and
// ragrb).  Every a/b there goes through a policy object `d`:
//   Recip<T> R = d.rec(b);  the denominator and its reciprocal (shared by every
//                           division by the same value)
//   d.div(a, R)             a/b for any numerator
//   d.divk(a, R)            a/b for a numerator that is a constant or was passed
//                           through d.chk() (loop-invariant)
// DivRef is the reference's rounding: IEEE `/` in fp32 (the compiler's
// div_scale / div_fmas / div_fixup sequence, 11 instructions and a vcc chain
// per division), `dv` in fp64.
//
// DivFast32 below is the faster fp32 policy.  Round 3 guarded it dynamically
// (a per-division range check) and removed it: no faster than IEEE once
// guarded.  Round 4 proves its operands in range statically (tools/div_proof.py
// over the domain of vege_domain.h), checks that domain once per column plus a
// few windows per iteration, and re-runs the loop through DivRef for a lane
// outside it (DESIGN.md "Division in the Newton loops").
template <class T>
struct Recip {
  T b, r;
};

template <class T>
struct DivRef {
  __device__ __forceinline__ Recip<T> rec(T b) const { return {b, b}; }
  __device__ __forceinline__ T div(T a, const Recip<T>& R) const { return dv(a, R.b); }
  __device__ __forceinline__ T divk(T a, const Recip<T>& R) const { return dv(a, R.b); }
  __device__ __forceinline__ T divn(T a, const Recip<T>& R) const { return dv(a, R.b); }
  __device__ __forceinline__ void chk(T) const {}
  // the reference's SQRT: IEEE correctly rounded
  __device__ __forceinline__ static T sqrt(T x) {
    if constexpr (sizeof(T) == 4) return ::sqrtf(x);
    else return ::sqrt(x);
  }
};

// sqrt of a finite x >= 2^-96: the compiler's
// correctly rounded fp32 sqrt sequence without its scaling of x < 2^-96 and
// its zero / infinity / NaN select, neither of which changes a result in that
// range.  v_sqrt_f32, then the two neighbour tests: s - 1 ulp if
// fma(-(s-ulp), s, x) <= 0, s + 1 ulp if fma(-(s+ulp), s, x) > 0 -- the same
// instructions in the same order as the IEEE lowering (tests/test_gpu_routines.py
// compares it with sqrtf over the range).
__device__ __forceinline__ float sqrt_normal32(float x) {
  const float s = __builtin_amdgcn_sqrtf(x);
  const float sm = __builtin_bit_cast(float, __builtin_bit_cast(uint32_t, s) - 1u);
  const float vm = __builtin_fmaf(-sm, s, x);
  float r = (vm <= 0.0f) ? sm : s;
  const float sp = __builtin_bit_cast(float, __builtin_bit_cast(uint32_t, s) + 1u);
  const float vp = __builtin_fmaf(-sp, s, x);
  return (vp > 0.0f) ? sp : r;
}

// DivFast32: the short exact sequence, used where the operands are proven to
// lie in its exact region (DESIGN.md "Division in the canopy loop").  The
// reciprocal r = fma(fma(-b, r0, 1), r0, r0) from v_rcp_f32 (shared by every
// division by the same b), then q = a*r, one fma residual correction and
// v_div_fixup_f32, which gives zero, infinite and NaN operands their IEEE
// results.  It equals IEEE a/b bit for bit whenever |b| is in [2^-126, 2^126]
// (normal, with a normal reciprocal), the residual a - b*q is not subnormal
// (a = 0 or |a| >= 2^-102) and |a/b| is in [2^-126, 2^126]
// (tools/fdiv_exhaust.hip: every normal b, every pair of significands, exact
// scaling by powers of two; profiles/r03/fdiv_exhaust2.txt; and the region's
// exponent edges, tests/test_gpu_routines.py).  The region stops short of
// FLT_MAX on purpose: for quotients within an ulp or two of it the product
// a*r can round past FLT_MAX and the sequence differs.
#ifdef NMP_COUNT_FALLBACK
// the counters of the counting builds: 0..39 sflx_kernel.hip's fallback
// reasons, 40..49 MthGuard32's calls, 50..57 DivFast32::divn's quotients
static __device__ unsigned int nmp_fb_reason[64];
// divn's groups of sites: the canopy loop (with its sfcdif1, ragrb and stomata
// bisection), the bare loop (with its sfcdif1), the soil sub-steps, atanf_ge1
enum { NMP_DIVN_CANOPY = 0, NMP_DIVN_BARE, NMP_DIVN_SOIL, NMP_DIVN_ATAN };
#endif
struct DivFast32 {
#ifdef NMP_COUNT_FALLBACK
  // The counting build forms the fix-up's result beside every divn quotient
  // and counts, per lane, the quotients formed and those whose bits the fix-up
  // would have changed.  The caller adds them to the group's counters
  // (nmp_fb_reason[50 + 2 grp], [51 + 2 grp]) once it knows that the lane keeps
  // the quotients: flush(ok) after a Newton loop, drop_last() on the soil
  // sub-steps' IEEE arm.  atanf_ge1's functor has no caller to do so and adds
  // at once, discarded loops included.
  int grp = NMP_DIVN_CANOPY;
  mutable unsigned nf = 0, nc = 0;
  mutable bool last = false;
  __device__ __forceinline__ void flush(bool keep) const {
    if (keep && nf) atomicAdd(&nmp_fb_reason[50 + 2 * grp], nf);
    if (keep && nc) atomicAdd(&nmp_fb_reason[51 + 2 * grp], nc);
    nf = nc = 0;
  }
  __device__ __forceinline__ void drop_last() const {
    nf -= 1;
    nc -= last;
  }
#endif
  __device__ __forceinline__ static float recip(float b) {
    float r = __builtin_amdgcn_rcpf(b);
    const float e = __builtin_fmaf(-b, r, 1.0f);
    return __builtin_fmaf(e, r, r);
  }
  __device__ __forceinline__ Recip<float> rec(float b) const { return {b, recip(b)}; }
  __device__ __forceinline__ float div(float a, const Recip<float>& R) const {
    float q = a * R.r;
    const float e = __builtin_fmaf(-R.b, q, a);
    q = __builtin_fmaf(e, R.r, q);
    return __builtin_amdgcn_div_fixupf(q, R.b, a);
  }
  __device__ __forceinline__ float divk(float a, const Recip<float>& R) const { return div(a, R); }
  // a/b without the closing v_div_fixup_f32.  Region: DivFast32's (|b| in
  // [2^-126, 2^126], a = 0 or |a| >= 2^-102, |a/b| in [2^-126, 2^126]), both
  // operands finite, and a never -0.  There the fix-up is the identity: for
  // a != 0 the fma already carries the quotient's sign, +0 / b gives +0 for
  // b > 0 and -0 for b < 0, and -0 / b gives +0 for b < 0.  The one case it
  // changed is a = -0 with b > 0, where this returns +0 and IEEE -0
  // (tests/test_gpu_div_nofix.py pins all four); tools/div_proof.py tracks the
  // sign of every numerator's zero and declares which sites may call this.
  // NaN or infinite operands give NaN here where the fix-up gave IEEE's
  // infinity: only lanes already outside a window see them, and their loop is
  // discarded.
  __device__ __forceinline__ float divn(float a, const Recip<float>& R) const {
    float q = a * R.r;
    const float e = __builtin_fmaf(-R.b, q, a);
    q = __builtin_fmaf(e, R.r, q);
#ifdef NMP_COUNT_FALLBACK
    const float qf = __builtin_amdgcn_div_fixupf(q, R.b, a);
    last = __builtin_bit_cast(uint32_t, qf) != __builtin_bit_cast(uint32_t, q);
    nf += 1;
    nc += last;
    if (grp == NMP_DIVN_ATAN) flush(true);
#endif
    return q;
  }
  __device__ __forceinline__ void chk(float) const {}
  // at the range-proven sqrt sites (tools/div_proof.py): x finite and >= 2^-96
  __device__ __forceinline__ static float sqrt(float x) { return sqrt_normal32(x); }
};

// One math policy per division policy (sfcdif1 and ragrb, the libm callers of
// the Newton loops).  With DivRef the loops call the full functions of Mth.
// With DivFast32 they call the in-range cores of glibc_math.h: the same main
// paths without the special-case exits, so an inlined call is straight-line
// code with no exec-mask branch.  tools/div_proof.py ("libm sites") derives
// every argument's interval from the domain of vege_domain.h and its windows
// on MOZ, MOZ2 and MOZG; a lane outside them re-runs its loop with DivRef and
// the full functions.  atanf's one division has a denominator >= 1 and a
// numerator that is -1, 0 or in [2^-23, 1): inside DivFast32's exact region.
template <class T, bool R, class D>
struct LoopMth {
  typedef Mth<T, R> type;
};
struct MthInRange32 : Mth<float, true> {
  NMP_MATH_FN float exp(float x) { return gm::expf_inrange(x, gm_lds); }
  NMP_MATH_FN float log(float x) { return gm::logf_inrange(x, gm_lds); }
  NMP_MATH_FN float pow_q(float x) { return gm::powf_inrange(x, 0.25f, gm_lds); }
  NMP_MATH_FN float pow_mq(float x) { return gm::powf_inrange(x, -0.25f, gm_lds); }
  struct Div {
    __device__ __forceinline__ float operator()(float a, float b) const {
      DivFast32 d;  // the numerator is never -0 (tools/div_proof.py)
#ifdef NMP_COUNT_FALLBACK
      d.grp = NMP_DIVN_ATAN;
#endif
      return d.divn(a, d.rec(b));
    }
  };
  NMP_MATH_FN float atan(float x) { return gm::atanf_ge1(x, Div{}); }
};
template <>
struct LoopMth<float, true, DivFast32> {
  typedef MthInRange32 type;
};

// The math policy of the fp32 "ref" call sites outside the Newton loops
// (GuardMth<T, R>::type; fp64 and "fast" math resolve to Mth<T, R>).  Those
// arguments carry no range proof.  Each call instead tests its argument
// against the in-range core's interval (vege_domain.h NMP_DOM_EXPF_HI, ...)
// across the wave: one ballot and a scalar branch.  If no active lane is
// outside, the wave runs the core, straight-line; otherwise it runs the full
// function.  Both arms return the full function's bits on the core's interval
// (tests/test_glibc_math_inrange.py, tests/test_glibc_math_outloop.py), so the
// results are exact by construction, whatever the limits.  The tests are
// written negated so that NaN counts as outside; the ballot sees active lanes
// only, so a call under a divergent branch is not slowed by what the inactive
// lanes' registers hold.
//   exp:   x < 88, -inf included        -> gm::expf_below88: the core, and the
//          underflow exit as a select.  One-sided because arguments far below
//          -88 are everyday values here (EXP(PSI G / (RV TG)) over dry soil,
//          EXP(-6 (ZWT - 2)) over a deep water table, EXP(-EXT VAI) at
//          sunrise): with |x| < 88 as the test, 7.6 % of the wave-level calls
//          took the full function (profiles/libm_outloop/fallback_rate.txt).
//   log:   x positive, normal, finite   -> gm::logf_inrange
//   log10: the same                     -> gm::log10f_inrange (logf's core)
//   pow:   x positive, normal, finite and y finite, nonzero (no lane needs
//          powf's special-case block) -> powf_log2, then powf_tail_sel: powf's
//          own functions in powf's order, the tail's overflow / underflow
//          exits (reachable: 0.01**26 in dry soil) as selects.
// NMP_COUNT_FALLBACK builds count, per function, the wave-level calls and
// those that took the full function (nmp_fb_reason 40..49, declared above
// DivFast32).
struct MthGuard32 : Mth<float, true> {
  // true when any active lane of the wave has `outside`; `slot`: the counters
  static __device__ __forceinline__ bool any_outside(bool outside, int slot) {
    const bool slow = __builtin_amdgcn_ballot_w64(outside) != 0;
#ifdef NMP_COUNT_FALLBACK
    const int lane = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
    if (__builtin_amdgcn_readfirstlane(lane) == lane) {  // the first active lane
      atomicAdd(&nmp_fb_reason[slot], 1u);
      if (slow) atomicAdd(&nmp_fb_reason[slot + 1], 1u);
    }
#else
    (void)slot;
#endif
    return slow;
  }
  static __device__ __forceinline__ bool pow_base_outside(float x) {
    return !(x >= NMP_DOM_POWF_LO && x <= NMP_DOM_POWF_HI);
  }
  // (the full function's arm is marked unlikely, so block placement keeps it
  // out of the straight-line path)
  NMP_MATH_FN float exp(float x) {
    const bool slow = any_outside(!(x < NMP_DOM_EXPF_HI), 40);
    if (__builtin_expect(slow, 0)) return gm::expf(x, gm_lds);
    return gm::expf_below88(x, gm_lds);
  }
  NMP_MATH_FN float log(float x) {
    const bool slow = any_outside(!(x >= NMP_DOM_LOGF_LO && x <= NMP_DOM_LOGF_HI), 42);
    if (__builtin_expect(slow, 0)) return gm::logf(x, gm_lds);
    return gm::logf_inrange(x, gm_lds);
  }
  NMP_MATH_FN float log10(float x) {
    const bool slow = any_outside(!(x >= NMP_DOM_LOGF_LO && x <= NMP_DOM_LOGF_HI), 44);
    if (__builtin_expect(slow, 0)) return gm::log10f(x, gm_lds);
    return gm::log10f_inrange(x, gm_lds);
  }
  NMP_MATH_FN float pow(float x, float y) {
    const bool slow =
        any_outside(pow_base_outside(x) || gm::powf_zeroinfnan(gm::asuint(y)), 46);
    if (__builtin_expect(slow, 0)) return gm::powf(x, y, gm_lds);
    return gm::powf_tail_sel(y, gm::powf_log2(gm::asuint(x), gm_lds), gm_lds);
  }
  static __device__ __forceinline__ void pow_pair(float x, float y1, float y2, float& r1,
                                                  float& r2) {
    const bool slow = any_outside(pow_base_outside(x) || gm::powf_zeroinfnan(gm::asuint(y1)) ||
                                      gm::powf_zeroinfnan(gm::asuint(y2)), 48);
    if (__builtin_expect(slow, 0)) {
      gm::powf_pair(x, y1, y2, gm_lds, r1, r2);
    } else {
      const double logx = gm::powf_log2(gm::asuint(x), gm_lds);
      r1 = gm::powf_tail_sel(y1, logx, gm_lds);
      r2 = gm::powf_tail_sel(y2, logx, gm_lds);
    }
  }
};
template <class T, bool R>
struct GuardMth {
  typedef Mth<T, R> type;
};
template <>
struct GuardMth<float, true> {
  typedef MthGuard32 type;
};

// Register-array access with a runtime index, lowered to a select chain so the
// array itself stays in VGPRs (a dynamic subscript would demote it to scratch).
// The empty asm pins each element as a register value: without it InstCombine
// folds the select chain back into one dynamically indexed load (a[i]), which
// forces the whole enclosing aggregate (the column struct) into scratch.
template <class T>
__device__ __forceinline__ T pin(T v) {
  __asm__ volatile("" : "+v"(v));
  return v;
}
template <class T, int N>
__device__ __forceinline__ T dget(const T (&a)[N], int i) {
  T r = pin(a[0]);
  // every element pinned unconditionally, then selected: one v_cndmask each
#pragma unroll
  for (int k = 1; k < N; ++k) {
    const T v = pin(a[k]);
    r = (i == k) ? v : r;
  }
  return r;
}
template <class T, int N>
__device__ __forceinline__ void dset(T (&a)[N], int i, T v) {
#pragma unroll
  for (int k = 0; k < N; ++k)
    if (i == k) a[k] = v;
}
__device__ __forceinline__ float zget(const float (&a)[4], int i) {
  return i == 0 ? a[0] : i == 1 ? a[1] : i == 2 ? a[2] : a[3];
}

}  // namespace nmp

// literal in the working precision: fp32 literals are parsed as float (like the
// reference's default-real constants), fp64 literals as double
#define L(x) (sizeof(T) == 4 ? (T)(x##f) : (T)(x))
