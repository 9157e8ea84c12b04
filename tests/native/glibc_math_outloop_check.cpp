// The main paths that csrc/sflx_math.h MthGuard32 runs outside the Newton loops
// and that tests/test_glibc_math_inrange.py does not cover, against the host
// libm, bit for bit:
//   powf's main path in both forms of its tail, powf_tail(y, powf_log2(ix), 0)
//   (the exits as branches) and powf_tail_sel (as selects), against powf(x, y);
//   log10f_inrange against log10f;
//   expf_below88 (the core with the underflow exit as a select) against expf.
// usage:
//   glibc_math_outloop_check pow <first> <count> <stride> <ybits>...
//     the `count` float bit patterns first, first + stride, ... as x, each with
//     every y given (as float bit patterns)
//   glibc_math_outloop_check powxy <xbits> <ybits> [<xbits> <ybits>]...
//     explicit pairs
//   glibc_math_outloop_check log10 <first> <count> <stride>
//   glibc_math_outloop_check expneg <first> <count> <stride>
//     expf_below88 against expf; the caller keeps x < 88 (negative patterns, -inf
//     included)
// -> prints "<mode> mismatches N of M overflow O underflow U" (the last two:
//    samples that took the tail's overflow / underflow exit); exit status 1 on
//    any mismatch.  The caller keeps x positive, normal and finite and y finite
//    and nonzero: outside that the main paths are unspecified.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "glibc_math.h"

static const gm::GmTables T = {GM_EXP2F_TAB, GM_LOGF_TAB, GM_POWF_TAB};

static float f_of(unsigned u) {
  float x;
  memcpy(&x, &u, 4);
  return x;
}
static unsigned u_of(float x) {
  unsigned u;
  memcpy(&u, &x, 4);
  return u;
}

struct Tally {
  unsigned long long n = 0, bad = 0, over = 0, under = 0;
};

// one (x, y): both forms of the tail against powf
static inline void pow_one(float x, float y, unsigned long long& bad, unsigned long long& over,
                           unsigned long long& under) {
  const double logx = gm::powf_log2(u_of(x), T);
  const unsigned a = u_of(gm::powf_tail(y, logx, 0, T));
  const unsigned s = u_of(gm::powf_tail_sel(y, logx, T));
  const unsigned r = u_of(::powf(x, y));
  const double ylogx = (double)y * logx;
  over += ylogx > 0x1.fffffffd1d571p+6;
  under += ylogx <= -150.0;
  if (a != r || s != r) {
#pragma omp critical
    if (!bad)
      fprintf(stderr, "first mismatch x=%a y=%a: tail %a select %a powf %a\n", x, y, f_of(a),
              f_of(s), f_of(r));
    bad++;
  }
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  Tally t;
  if (!strcmp(argv[1], "pow") && argc >= 6) {
    const unsigned long long first = strtoull(argv[2], 0, 0), count = strtoull(argv[3], 0, 0);
    const unsigned long long stride = strtoull(argv[4], 0, 0);
    std::vector<float> ys;
    for (int i = 5; i < argc; ++i) ys.push_back(f_of((unsigned)strtoull(argv[i], 0, 0)));
    unsigned long long bad = 0, over = 0, under = 0;
#pragma omp parallel for reduction(+ : bad, over, under) schedule(static, 65536)
    for (long long i = 0; i < (long long)count; ++i) {
      const float x = f_of((unsigned)(first + (unsigned long long)i * stride));
      for (float y : ys) pow_one(x, y, bad, over, under);
    }
    t.n = count * ys.size();
    t.bad = bad, t.over = over, t.under = under;
  } else if (!strcmp(argv[1], "powxy") && argc >= 4 && argc % 2 == 0) {
    for (int i = 2; i + 1 < argc; i += 2) {
      pow_one(f_of((unsigned)strtoull(argv[i], 0, 0)), f_of((unsigned)strtoull(argv[i + 1], 0, 0)),
              t.bad, t.over, t.under);
      t.n++;
    }
  } else if (!strcmp(argv[1], "log10") && argc == 5) {
    const unsigned long long first = strtoull(argv[2], 0, 0), count = strtoull(argv[3], 0, 0);
    const unsigned long long stride = strtoull(argv[4], 0, 0);
    unsigned long long bad = 0;
#pragma omp parallel for reduction(+ : bad) schedule(static, 65536)
    for (long long i = 0; i < (long long)count; ++i) {
      const float x = f_of((unsigned)(first + (unsigned long long)i * stride));
      const unsigned a = u_of(gm::log10f_inrange(x, T)), r = u_of(::log10f(x));
      if (a != r) {
#pragma omp critical
        if (!bad) fprintf(stderr, "first mismatch x=%a: mine %a ref %a\n", x, f_of(a), f_of(r));
        bad++;
      }
    }
    t.n = count, t.bad = bad;
  } else if (!strcmp(argv[1], "expneg") && argc == 5) {
    const unsigned long long first = strtoull(argv[2], 0, 0), count = strtoull(argv[3], 0, 0);
    const unsigned long long stride = strtoull(argv[4], 0, 0);
    unsigned long long bad = 0, under = 0;
#pragma omp parallel for reduction(+ : bad, under) schedule(static, 65536)
    for (long long i = 0; i < (long long)count; ++i) {
      const float x = f_of((unsigned)(first + (unsigned long long)i * stride));
      const unsigned a = u_of(gm::expf_below88(x, T)), r = u_of(::expf(x));
      under += x < -0x1.9fe368p6f;
      if (a != r) {
#pragma omp critical
        if (!bad) fprintf(stderr, "first mismatch x=%a: mine %a ref %a\n", x, f_of(a), f_of(r));
        bad++;
      }
    }
    t.n = count, t.bad = bad, t.under = under;
  } else {
    fprintf(stderr, "bad arguments\n");
    return 2;
  }
  printf("%s mismatches %llu of %llu overflow %llu underflow %llu\n", argv[1], t.bad, t.n, t.over,
         t.under);
  return t.bad ? 1 : 0;
}
