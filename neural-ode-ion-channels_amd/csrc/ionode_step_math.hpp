// ionode_step_math.hpp -- what the optimiser steps (ionode_lm.hpp, ionode_cmaes.hpp, ionode_mcmc.hpp, ionode_mala.hpp, ionode_ensemble.hpp) share on both sides of the
// bit-for-bit contract: the fp64 predicates, lm_exp, cm_log and the Philox / AS241 generator.  Every function is compiled for the
// kernel and for the host mirror from this one text; each has ONE written operation sequence (fma only inside lm_exp, no libm / ocml
// call).  The trial-row writers and the packed Cholesky loops stay per step: shared copies moved the kernels' register figures
// (profiles/step_refactor.md).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ionode.h"

namespace ionode {

constexpr int kLmMaxFree = IONODE_LM_MAX_FREE;

__host__ __device__ inline double lm_inf() { return __builtin_inf(); }
__host__ __device__ inline bool lm_finite(double x) { return __builtin_fabs(x) < __builtin_inf(); }   // false for NaN
__host__ __device__ inline double lm_pow2i(int k) { return __builtin_bit_cast(double, (long long)(k + 1023) << 52); }

// det_exp (ionode_math.hpp), operation for operation, compiled for both sides
__host__ __device__ inline double lm_exp(double x) {
  if (x != x) return x;
  if (x > 709.782712893384) return __builtin_inf();
  if (x < -745.1332191019412) return 0.0;
  const double kf = __builtin_rint(x * 0x1.71547652b82fep+0);
  double r = __builtin_fma(-kf, 0x1.62e42fee00000p-1, x);
  r = __builtin_fma(-kf, 0x1.a39ef35793c76p-33, r);
  double p = 1.0 / 6227020800.0;
  p = __builtin_fma(p, r, 1.0 / 479001600.0);
  p = __builtin_fma(p, r, 1.0 / 39916800.0);
  p = __builtin_fma(p, r, 1.0 / 3628800.0);
  p = __builtin_fma(p, r, 1.0 / 362880.0);
  p = __builtin_fma(p, r, 1.0 / 40320.0);
  p = __builtin_fma(p, r, 1.0 / 5040.0);
  p = __builtin_fma(p, r, 1.0 / 720.0);
  p = __builtin_fma(p, r, 1.0 / 120.0);
  p = __builtin_fma(p, r, 1.0 / 24.0);
  p = __builtin_fma(p, r, 1.0 / 6.0);
  p = __builtin_fma(p, r, 0.5);
  p = __builtin_fma(p, r, 1.0);
  p = __builtin_fma(p, r, 1.0);
  const int k = (int)kf;
  const int k1 = k / 2;
  return (p * lm_pow2i(k1)) * lm_pow2i(k - k1);
}

// ---- the generator ----

// Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11)
__host__ __device__ inline void cm_philox(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t (&out)[4]) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// ln x with one written operation sequence: exponent by bit extraction, mantissa reduced to [sqrt(1/2), sqrt(2)], then
// ln m = 2 atanh(s), s = (m - 1) / (m + 1), |s| <= 0.1716: s^2 <= 0.02944 and the series to s^23 leaves a truncation below 2^-60.
// A few ulp (measured against numpy.log: tests/test_cmaes_host.py); it only has to be the same on both sides.
__host__ __device__ inline double cm_log(double x) {
  if (x != x || x < 0.0) return __builtin_nan("");
  if (x == 0.0) return -__builtin_inf();
  if (x == __builtin_inf()) return x;
  int e = 0;
  uint64_t b = __builtin_bit_cast(uint64_t, x);
  if ((b >> 52) == 0) {   // subnormal: scaled by 2^54 exactly
    x = x * 0x1p54;
    b = __builtin_bit_cast(uint64_t, x);
    e = -54;
  }
  e += (int)(b >> 52) - 1023;
  double m = __builtin_bit_cast(double, (b & 0x000FFFFFFFFFFFFFull) | 0x3FF0000000000000ull);   // [1, 2)
  if (m > 0x1.6a09e667f3bcdp+0) {
    m = m * 0.5;
    e += 1;
  }
  const double s = (m - 1.0) / (m + 1.0);
  const double z = s * s;
  double p = 1.0 / 23.0;
  p = p * z + 1.0 / 21.0;
  p = p * z + 1.0 / 19.0;
  p = p * z + 1.0 / 17.0;
  p = p * z + 1.0 / 15.0;
  p = p * z + 1.0 / 13.0;
  p = p * z + 1.0 / 11.0;
  p = p * z + 1.0 / 9.0;
  p = p * z + 1.0 / 7.0;
  p = p * z + 1.0 / 5.0;
  p = p * z + 1.0 / 3.0;
  const double lm = 2.0 * s + (2.0 * s) * (z * p);
  const double ed = (double)e;
  return (ed * 0x1.62e42fee00000p-1 + lm) + ed * 0x1.a39ef35793c76p-33;   // (the high part of ln 2 has 21 trailing zero bits: e times it is exact)
}

// Wichura, "Algorithm AS 241: the percentage points of the normal distribution", Appl. Statist. 37 (1988): PPND16
__host__ __device__ inline double cm_ppnd16(double p) {
  const double q = p - 0.5;
  if (__builtin_fabs(q) <= 0.425) {
    const double r = 0.180625 - q * q;
    const double num = (((((((2509.0809287301226727 * r + 33430.575583588128105) * r + 67265.770927008700853) * r + 45921.953931549871457) * r +
                           13731.693765509461125) * r + 1971.5909503065514427) * r + 133.14166789178437745) * r + 3.387132872796366608);
    const double den = (((((((5226.495278852545925 * r + 28729.085735721942674) * r + 39307.89580009271061) * r + 21213.794301586595867) * r +
                           5394.1960214247511077) * r + 687.1870074920579083) * r + 42.313330701600911252) * r + 1.0);
    return q * num / den;
  }
  double r = q < 0.0 ? p : 1.0 - p;
  r = __builtin_sqrt(-cm_log(r));
  double v;
  if (r <= 5.0) {
    r = r - 1.6;
    const double num = (((((((7.7454501427834140764e-4 * r + 0.0227238449892691845833) * r + 0.24178072517745061177) * r + 1.27045825245236838258) * r +
                           3.64784832476320460504) * r + 5.7694972214606914055) * r + 4.6303378461565452959) * r + 1.42343711074968357734);
    const double den = (((((((1.05075007164441684324e-9 * r + 5.475938084995344946e-4) * r + 0.0151986665636164571966) * r + 0.14810397642748007459) * r +
                           0.68976733498510000455) * r + 1.6763848301838038494) * r + 2.05319162663775882187) * r + 1.0);
    v = num / den;
  } else {
    r = r - 5.0;
    const double num = (((((((2.01033439929228813265e-7 * r + 2.71155556874348757815e-5) * r + 0.0012426609473880784386) * r + 0.026532189526576123093) * r +
                           0.29656057182850489123) * r + 1.7848265399172913358) * r + 5.4637849111641143699) * r + 6.6579046435011037772);
    const double den = (((((((2.04426310338993978564e-15 * r + 1.4215117583164458887e-7) * r + 1.8463183175100546818e-5) * r + 7.868691311456132591e-4) * r +
                           0.0148753612908506148525) * r + 0.13692988092273580531) * r + 0.59983224863253602715) * r + 1.0);
    v = num / den;
  }
  return q < 0.0 ? -v : v;
}

__host__ __device__ inline double cm_uniform(uint32_t hi, uint32_t lo) {   // 53 bits, in (0, 1): never 0, never 1
  return ((double)(((uint64_t)hi << 21) | (uint64_t)(lo >> 11)) + 0.5) * 0x1p-53;
}

// the two normal deviates of (seed, run, generation, candidate, coordinate pair, attempt)
__host__ __device__ inline void cm_normal_pair(uint32_t seed_lo, uint32_t seed_hi, int run, int gen, int cand, int pair, int attempt, double &z0,
                                               double &z1) {
  uint32_t w[4];
  cm_philox((uint32_t)run, (uint32_t)gen, (uint32_t)cand, (uint32_t)pair + 65536u * (uint32_t)attempt, seed_lo, seed_hi, w);
  z0 = cm_ppnd16(cm_uniform(w[0], w[1]));
  z1 = cm_ppnd16(cm_uniform(w[2], w[3]));
}

}  // namespace ionode
