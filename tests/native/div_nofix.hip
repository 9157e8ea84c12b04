// Test-side device entry points for DivFast32::divn (csrc/sflx_math.h), the
// short division without the closing v_div_fixup_f32
// (tests/test_gpu_div_nofix.py; built into tests/lib/libnmp_div_nofix.so by
// __graft_entry__.build()).  Everything is compared as raw 32-bit patterns
// against the device's IEEE a / b and against DivFast32::div.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sflx_math.h"

namespace {

struct Buf {
  void* p = nullptr;
  explicit Buf(size_t bytes) {
    if (hipMalloc(&p, bytes) != hipSuccess) p = nullptr;
  }
  ~Buf() {
    if (p) (void)hipFree(p);
  }
};

__device__ __forceinline__ bool in_region(float w) {
  const float aw = fabsf(w);
  return aw >= 0x1p-126f && aw <= 0x1p126f;
}

// cnt[0] pairs inside the region, cnt[1] divn != IEEE, cnt[2] divn != div;
// first[0..1]: the operands' bits of the smallest mismatching a pattern
__device__ __forceinline__ void check(float a, float b, const nmp::DivFast32& d,
                                      const nmp::Recip<float>& R, unsigned long long& n,
                                      unsigned long long& bad, unsigned long long& badd,
                                      unsigned* first) {
  const float w = a / b;
  // the region: |b| in [2^-126, 2^126], |a| >= 2^-102, |a/b| in [2^-126, 2^126]
  if (!in_region(b) || !(fabsf(a) >= 0x1p-102f) || !in_region(w)) return;
  ++n;
  const unsigned q = __float_as_uint(d.divn(a, R));
  if (q != __float_as_uint(d.div(a, R))) ++badd;
  if (q != __float_as_uint(w)) {
    ++bad;
    if (atomicMin(&first[0], __float_as_uint(a)) > __float_as_uint(a)) first[1] = __float_as_uint(b);
  }
}

// Every exponent pair eb in [-126, 126] x ea in [-102, 127], nsig significand
// pairs (sa[i], sb[i]) each, all four sign combinations.  One thread per
// (exponent pair, significand pair).
__global__ void k_exp_pairs(unsigned nsig, const unsigned* sa, const unsigned* sb,
                            unsigned long long* cnt, unsigned* first) {
  constexpr int NEB = 253, NEA = 230;
  const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= (uint64_t)NEB * NEA * nsig) return;
  const unsigned i = (unsigned)(k % nsig);
  const int ea = -102 + (int)((k / nsig) % NEA), eb = -126 + (int)(k / nsig / NEA);
  const float ma = ldexpf(__uint_as_float(0x3f800000u | (sa[i] & 0x7fffffu)), ea);
  const float mb = ldexpf(__uint_as_float(0x3f800000u | (sb[i] & 0x7fffffu)), eb);
  // (2^126 itself is b's upper end: only its significand 0 is inside)
  if (!(mb <= 0x1p126f)) return;
  const nmp::DivFast32 d;
  unsigned long long n = 0, bad = 0, badd = 0;
  for (int s = 0; s < 4; ++s) {
    const float a = (s & 1) ? -ma : ma, b = (s & 2) ? -mb : mb;
    check(a, b, d, d.rec(b), n, bad, badd, first);
  }
  if (n) atomicAdd(&cnt[0], n);
  if (bad) atomicAdd(&cnt[1], bad);
  if (badd) atomicAdd(&cnt[2], badd);
}

// Significand sweeps at one exponent pair: a = +-(1 + ia/2^23) 2^ea for ia =
// oa, oa + sta, ... and b = +-(1 + ib/2^23) 2^eb for ib = ob, ob + stb, ...;
// one thread per ib value and chunk of 2^12 ia steps; the signs alternate
// from one a value to the next and from one b value to the next.
constexpr unsigned kChunk = 1u << 12;
__global__ void k_edge(int ea, int eb, unsigned sta, unsigned oa, unsigned stb, unsigned ob,
                       unsigned nchunk, unsigned nb, unsigned long long* cnt, unsigned* first) {
  const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= (uint64_t)nb * nchunk) return;
  const uint64_t jb = k / nchunk;
  const uint64_t ib = ob + jb * (uint64_t)stb;
  if (ib >= (1u << 23)) return;
  const float mb = ldexpf(__uint_as_float(0x3f800000u | (unsigned)ib), eb);
  if (!(mb <= 0x1p126f)) return;
  const float b = (jb & 1) ? -mb : mb;
  const nmp::DivFast32 d;
  const nmp::Recip<float> R = d.rec(b);
  unsigned long long n = 0, bad = 0, badd = 0;
  uint64_t ia = oa + (k % nchunk) * (uint64_t)kChunk * sta;
  for (unsigned j = 0; j < kChunk && ia < (1u << 23); ++j, ia += sta) {
    const float m = ldexpf(__uint_as_float(0x3f800000u | (unsigned)ia), ea);
    check((j & 1) ? -m : m, b, d, R, n, bad, badd, first);
  }
  if (n) atomicAdd(&cnt[0], n);
  if (bad) atomicAdd(&cnt[1], bad);
  if (badd) atomicAdd(&cnt[2], badd);
}

// element by element: divn, div and IEEE a / b of the given bit patterns
__global__ void k_eval(unsigned n, const unsigned* a, const unsigned* b, unsigned* qn, unsigned* qd,
                       unsigned* qi) {
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float x = __uint_as_float(a[i]), y = __uint_as_float(b[i]);
  const nmp::DivFast32 d;
  const nmp::Recip<float> R = d.rec(y);
  qn[i] = __float_as_uint(d.divn(x, R));
  qd[i] = __float_as_uint(d.div(x, R));
  qi[i] = __float_as_uint(x / y);
}

int finish(const Buf& dc, const Buf& df, unsigned long long* cnt3, unsigned* first2) {
  if (hipDeviceSynchronize() != hipSuccess) return -4;
  if (hipMemcpy(cnt3, dc.p, 3 * sizeof(unsigned long long), hipMemcpyDeviceToHost) != hipSuccess)
    return -4;
  return hipMemcpy(first2, df.p, 2 * sizeof(unsigned), hipMemcpyDeviceToHost) == hipSuccess ? 0 : -4;
}

int start(const Buf& dc, const Buf& df) {
  const unsigned none[2] = {0xffffffffu, 0u};
  if (!dc.p || !df.p) return -4;
  if (hipMemset(dc.p, 0, 3 * sizeof(unsigned long long)) != hipSuccess) return -4;
  return hipMemcpy(df.p, none, sizeof(none), hipMemcpyHostToDevice) == hipSuccess ? 0 : -4;
}

}  // namespace

extern "C" {

int dn_exp_pairs(unsigned nsig, const unsigned* sa, const unsigned* sb, unsigned long long* cnt3,
                 unsigned* first2) {
  if (nsig == 0 || nsig > 4096) return -1;
  Buf dc(3 * sizeof(unsigned long long)), df(2 * sizeof(unsigned));
  Buf da(nsig * sizeof(unsigned)), db(nsig * sizeof(unsigned));
  if (start(dc, df) || !da.p || !db.p) return -4;
  if (hipMemcpy(da.p, sa, nsig * sizeof(unsigned), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(db.p, sb, nsig * sizeof(unsigned), hipMemcpyHostToDevice) != hipSuccess)
    return -4;
  const uint64_t nthr = (uint64_t)253 * 230 * nsig;
  hipLaunchKernelGGL(k_exp_pairs, dim3((unsigned)((nthr + 255) / 256)), dim3(256), 0, 0, nsig,
                     (const unsigned*)da.p, (const unsigned*)db.p, (unsigned long long*)dc.p,
                     (unsigned*)df.p);
  return finish(dc, df, cnt3, first2);
}

int dn_edge(int ea, int eb, unsigned sta, unsigned oa, unsigned stb, unsigned ob,
            unsigned long long* cnt3, unsigned* first2) {
  if (sta == 0 || stb == 0 || oa >= sta || ob >= stb) return -1;
  if (ea < -149 || ea > 127 || eb < -149 || eb > 127) return -1;
  Buf dc(3 * sizeof(unsigned long long)), df(2 * sizeof(unsigned));
  if (start(dc, df)) return -4;
  const uint64_t nbv = ((1u << 23) - ob + stb - 1) / stb;
  const uint64_t nav = ((1u << 23) - oa + sta - 1) / sta;
  const unsigned nchunk = (unsigned)((nav + kChunk - 1) / kChunk);
  const uint64_t nthr = nbv * nchunk;
  if (nthr > (1ull << 31)) return -1;
  hipLaunchKernelGGL(k_edge, dim3((unsigned)((nthr + 255) / 256)), dim3(256), 0, 0, ea, eb, sta, oa,
                     stb, ob, nchunk, (unsigned)nbv, (unsigned long long*)dc.p, (unsigned*)df.p);
  return finish(dc, df, cnt3, first2);
}

int dn_eval(unsigned n, const unsigned* a, const unsigned* b, unsigned* qn, unsigned* qd,
            unsigned* qi) {
  if (n == 0 || n > (1u << 24)) return -1;
  const size_t bytes = n * sizeof(unsigned);
  Buf da(bytes), db(bytes), d1(bytes), d2(bytes), d3(bytes);
  if (!da.p || !db.p || !d1.p || !d2.p || !d3.p) return -4;
  if (hipMemcpy(da.p, a, bytes, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(db.p, b, bytes, hipMemcpyHostToDevice) != hipSuccess)
    return -4;
  hipLaunchKernelGGL(k_eval, dim3((n + 255) / 256), dim3(256), 0, 0, n, (const unsigned*)da.p,
                     (const unsigned*)db.p, (unsigned*)d1.p, (unsigned*)d2.p, (unsigned*)d3.p);
  if (hipDeviceSynchronize() != hipSuccess) return -4;
  if (hipMemcpy(qn, d1.p, bytes, hipMemcpyDeviceToHost) != hipSuccess ||
      hipMemcpy(qd, d2.p, bytes, hipMemcpyDeviceToHost) != hipSuccess ||
      hipMemcpy(qi, d3.p, bytes, hipMemcpyDeviceToHost) != hipSuccess)
    return -4;
  return 0;
}

}  // extern "C"
