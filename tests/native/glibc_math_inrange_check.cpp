// The in-range cores of csrc/glibc_math.h (expf_inrange, logf_inrange,
// powf_inrange with y = +-0.25, atanf_ge1) against the host libm, bit for bit.
// usage: glibc_math_inrange_check <func> <first> <count> <stride>
//   compares the `count` float bit patterns first, first + stride, ...
//   -> prints "<func> mismatches N of M"; exit status 1 on any mismatch.
// The caller (tests/test_glibc_math_inrange.py) keeps every pattern inside the
// core's interval: outside it the cores are unspecified.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "glibc_math.h"

static const gm::GmTables T = {GM_EXP2F_TAB, GM_LOGF_TAB, GM_POWF_TAB};

typedef float (*ff)(float);
static float c_expf(float x) { return gm::expf_inrange(x, T); }
static float c_logf(float x) { return gm::logf_inrange(x, T); }
static float c_pow_q(float x) { return gm::powf_inrange(x, 0.25f, T); }
static float c_pow_mq(float x) { return gm::powf_inrange(x, -0.25f, T); }
static float c_atanf(float x) { return gm::atanf_ge1(x, gm::DivIeee{}); }
static float r_pow_q(float x) { return ::powf(x, 0.25f); }
static float r_pow_mq(float x) { return ::powf(x, -0.25f); }

struct Entry { const char* name; ff mine; ff ref; };
static const Entry FUNCS[] = {
    {"expf", c_expf, ::expf},       {"logf", c_logf, ::logf},    {"pow_q", c_pow_q, r_pow_q},
    {"pow_mq", c_pow_mq, r_pow_mq}, {"atanf", c_atanf, ::atanf},
};

int main(int argc, char** argv) {
  if (argc != 5) return 2;
  const unsigned long long first = strtoull(argv[2], 0, 0), count = strtoull(argv[3], 0, 0);
  const unsigned long long stride = strtoull(argv[4], 0, 0);
  for (const Entry& e : FUNCS) {
    if (strcmp(e.name, argv[1])) continue;
    unsigned long long bad = 0;
    unsigned first_bad = 0;
#pragma omp parallel for reduction(+ : bad) schedule(static, 65536)
    for (long long i = 0; i < (long long)count; ++i) {
      const unsigned u = (unsigned)(first + (unsigned long long)i * stride);
      float x;
      memcpy(&x, &u, 4);
      const float a = e.mine(x), b = e.ref(x);
      unsigned ua, ub;
      memcpy(&ua, &a, 4);
      memcpy(&ub, &b, 4);
      // (pow_q: x >= 1 gives a result >= 1, the floor tools/div_proof.py takes
      // for atanf_ge1's and logf_inrange's arguments in sfcdif1)
      const bool floor_ok = e.mine != c_pow_q || !(x >= 1.0f) || a >= 1.0f;
      if (ua != ub || !floor_ok) {  // inside the intervals no result is NaN: bits must match
        bad++;
#pragma omp critical
        if (!first_bad) {
          first_bad = u ? u : 1;
          fprintf(stderr, "first mismatch x=%a (0x%08x): mine %a ref %a\n", x, u, a, b);
        }
      }
    }
    printf("%s mismatches %llu of %llu\n", e.name, bad, count);
    return bad ? 1 : 0;
  }
  fprintf(stderr, "unknown function %s\n", argv[1]);
  return 2;
}
