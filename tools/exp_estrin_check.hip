// fp64 exp_estrin (below) against the host exp over [-750, 710] and the
// special cases (GPU box; built by hand: hipcc -O3 --offload-arch=gfx950
// -o tools/exp_estrin_check tools/exp_estrin_check.hip).  Prints the maximum
// relative error in ulp.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cmath>
#include <vector>

// fp64 exp with a short dependent chain, a round-5 experiment for config #2's
// one-wave-per-SIMD kernel (no gain: profiles/r05/f64_estrin_ab.txt): ocml's own
// reduction (k = rint(x/ln2), r = x - k ln2 in two parts) and its degree-11
// Taylor coefficients, but the polynomial evaluated by Estrin's scheme (depth
// 4 instead of 11 dependent FMAs) and rebuilt with ldexp; within an ulp or two
// of ocml's result.
__device__ __forceinline__ double exp_estrin(double x) {
  const double k = __builtin_rint(x * 1.4426950408889634);     // x / ln2
  double r = __builtin_fma(k, -0.6931471805599453, x);          // ln2, then its tail
  r = __builtin_fma(k, -2.3190468138462996e-17, r);
  const double r2 = r * r, r4 = r2 * r2, r8 = r4 * r4;
  // ocml's coefficients c0..c11 (c0 = c1 = 1), paired by Estrin's scheme
  const double q0 = __builtin_fma(r, 1.0, 1.0);
  const double q1 = __builtin_fma(r, 0.16666666666666477, 0.5000000000000012);
  const double q2 = __builtin_fma(r, 0.008333333333455043, 0.041666666666519754);
  const double q3 = __builtin_fma(r, 0.00019841269589115522, 0.0013888888945916382);
  const double q4 = __builtin_fma(r, 2.755751454582531e-06, 2.480149103909504e-05);
  const double q5 = __builtin_fma(r, 2.502232256764614e-08, 2.7630903490112654e-07);
  const double s0 = __builtin_fma(r2, q1, q0);
  const double s1 = __builtin_fma(r2, q3, q2);
  const double s2 = __builtin_fma(r2, q5, q4);
  const double p = __builtin_fma(r8, s2, __builtin_fma(r4, s1, s0));
  const double e = __builtin_ldexp(p, (int)k);
  // ocml's limits: +inf above 1024, 0 below -1075 (ldexp saturates between);
  // NaN propagates through r
  return x > 1024.0 ? __builtin_inf() : (x < -1075.0 ? 0.0 : e);
}
__global__ void k(int n, const double* x, double* a, double* b) {
  int i = blockIdx.x * blockDim.x + threadIdx.x; if (i >= n) return;
  a[i] = exp_estrin(x[i]); b[i] = exp(x[i]);
}
int main() {
  const int n = 1 << 22; std::vector<double> x(n), a(n), b(n);
  for (int i = 0; i < n; ++i) x[i] = -750.0 + 1460.0 * (double)i / n;
  x[0] = 0; x[1] = NAN; x[2] = INFINITY; x[3] = -INFINITY; x[4] = 1e-300; x[5] = 709.7; x[6]=-745.0;
  double *dx, *da, *db; hipMalloc(&dx, n*8); hipMalloc(&da, n*8); hipMalloc(&db, n*8);
  hipMemcpy(dx, x.data(), n*8, hipMemcpyHostToDevice);
  hipLaunchKernelGGL(k, dim3(n/256), dim3(256), 0, 0, n, dx, da, db);
  hipMemcpy(a.data(), da, n*8, hipMemcpyDeviceToHost); hipMemcpy(b.data(), db, n*8, hipMemcpyDeviceToHost);
  double maxrel = 0; long bad = 0;
  for (int i = 0; i < n; ++i) {
    double ref = std::exp(x[i]);
    if (std::isnan(ref)) { if (!std::isnan(a[i])) ++bad; continue; }
    if (ref == 0 || std::isinf(ref)) { if (a[i] != ref && std::fabs(ref) > 1e-300) ++bad; continue; }
    if (ref < 1e-300) continue;
    double rel = std::fabs(a[i] - ref) / ref; if (rel > maxrel) maxrel = rel;
  }
  printf("exp_estrin: max rel err vs host exp %.3g (%.2f ulp), special-case mismatches %ld\n", maxrel, maxrel / 2.22e-16, bad);
  return 0;
}
