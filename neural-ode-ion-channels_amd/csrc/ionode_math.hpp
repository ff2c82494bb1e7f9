// ionode_math.hpp -- device arithmetic shared by every kernel: the Dormand-Prince tableau, the deterministic exp / fifth root, the
// correctly rounded divisions, the cross-lane helpers, LeakyReLU and the diagnostic build's phase stamps.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ionode {

using f32x4 = __attribute__((ext_vector_type(4))) float;
typedef float f32x2 __attribute__((ext_vector_type(2)));

// Dormand-Prince / Shampine coefficients.
__device__ constexpr double kAlpha[6] = {1.0 / 5, 3.0 / 10, 4.0 / 5, 8.0 / 9, 1.0, 1.0};
__device__ constexpr double kBeta[6][6] = {
    {1.0 / 5, 0, 0, 0, 0, 0},
    {3.0 / 40, 9.0 / 40, 0, 0, 0, 0},
    {44.0 / 45, -56.0 / 15, 32.0 / 9, 0, 0, 0},
    {19372.0 / 6561, -25360.0 / 2187, 64448.0 / 6561, -212.0 / 729, 0, 0},
    {9017.0 / 3168, -355.0 / 33, 46732.0 / 5247, 49.0 / 176, -5103.0 / 18656, 0},
    {35.0 / 384, 0.0, 500.0 / 1113, 125.0 / 192, -2187.0 / 6784, 11.0 / 84},
};
__device__ constexpr double kCerr[7] = {
    35.0 / 384 - 1951.0 / 21600,       0.0,
    500.0 / 1113 - 22642.0 / 50085,    125.0 / 192 - 451.0 / 720,
    -2187.0 / 6784 - -12231.0 / 42400, 11.0 / 84 - 649.0 / 6300,
    -1.0 / 60.0,
};
__device__ constexpr double kCmid[7] = {
    6025192743.0 / 30085553152.0 / 2,     0.0,
    51252292925.0 / 65400821598.0 / 2,    -2691868925.0 / 45128329728.0 / 2,
    187940372067.0 / 1594534317056.0 / 2, -1776094331.0 / 19743644256.0 / 2,
    11237099.0 / 235043384.0 / 2,
};

// Deterministic exp() and fifth root (DESIGN.md "Deterministic transcendentals"): dopri5's controller
// amplifies last-ulp differences of these two functions chaotically, so results are only reproducible
// across devices/libraries if both are fixed IEEE operation sequences.  < 1 ulp / <= 2 ulp accurate: det_exp over its whole
// domain, subnormal results (in units of 2^-1074) and both edges included; det_root5 for NORMAL x -- for subnormal x seven Newton steps
// from the exponent-field guess do not converge (det_root5(5e-324) = 5.5e-63 for 2.2e-65; harmless, the controller clamps the
// factor), there it only equals the oracle's.  tests/test_gpu_math_probe.py checks every function of this header on the device.
__device__ __forceinline__ double pow2i(int k) { return __longlong_as_double((long long)(k + 1023) << 52); }

// fma(p, r, c) with the constant c as a SCALAR operand.  Left to itself hipcc emits v_fmac_f64 with c copied into the destination
// register first (two v_mov_b32 per constant and use -- or, with machine-LICM, every constant hoisted into a VGPR pair that is
// then spilled); both are VALU instructions on the pipe the f32 MFMA shares.  An SGPR pair costs two s_mov_b32.
__device__ __forceinline__ double fma_sc(double p, double r, double c) {
  double d;
  asm("v_fma_f64 %0, %1, %2, %3" : "=v"(d) : "v"(p), "v"(r), "s"(c));
  return d;
}

__device__ __forceinline__ double det_exp(double x) {
  if (x != x) return x;
  if (x > 709.782712893384) return __builtin_inf();
  if (x < -745.1332191019412) return 0.0;
  const double kf = rint(x * 0x1.71547652b82fep+0);
  double r = fma(-kf, 0x1.62e42fee00000p-1, x);
  r = fma(-kf, 0x1.a39ef35793c76p-33, r);
  double p = 1.0 / 6227020800.0;
  p = fma(p, r, 1.0 / 479001600.0);
  p = fma(p, r, 1.0 / 39916800.0);
  p = fma(p, r, 1.0 / 3628800.0);
  p = fma(p, r, 1.0 / 362880.0);
  p = fma(p, r, 1.0 / 40320.0);
  p = fma(p, r, 1.0 / 5040.0);
  p = fma(p, r, 1.0 / 720.0);
  p = fma(p, r, 1.0 / 120.0);
  p = fma(p, r, 1.0 / 24.0);
  p = fma(p, r, 1.0 / 6.0);
  p = fma(p, r, 0.5);
  p = fma(p, r, 1.0);
  p = fma(p, r, 1.0);
  const int k = (int)kf;
  const int k1 = k / 2;
  return (p * pow2i(k1)) * pow2i(k - k1);
}
__device__ __forceinline__ float det_expf(float x) { return (float)det_exp((double)x); }

// The same function for the closed-form kernels' stage loop, where exp is a third of the issue work: the two power-of-two
// multiplications (p * 2^k1) * 2^(k - k1) are one v_ldexp_f64.  Bit-identical: p * 2^k is exact while the result is normal,
// and where it is subnormal or overflows both forms round exactly once (the first factor of the product form is always exact).
__device__ __forceinline__ double det_exp_ldexp(double x) {
  if (x != x) return x;
  if (x > 709.782712893384) return __builtin_inf();
  if (x < -745.1332191019412) return 0.0;
  const double kf = rint(x * 0x1.71547652b82fep+0);
  double r = fma(-kf, 0x1.62e42fee00000p-1, x);
  r = fma(-kf, 0x1.a39ef35793c76p-33, r);
  // addend constants as SCALAR operands (fma_sc): left to itself hipcc writes each of them into a VGPR pair first (v_fmac_f64 has
  // its addend tied to the destination) -- 20 v_mov_b32 per call, a third of the closed-form stage loop's vector instructions
  double p = 1.0 / 6227020800.0;
  p = fma_sc(p, r, 1.0 / 479001600.0);
  p = fma_sc(p, r, 1.0 / 39916800.0);
  p = fma_sc(p, r, 1.0 / 3628800.0);
  p = fma_sc(p, r, 1.0 / 362880.0);
  p = fma_sc(p, r, 1.0 / 40320.0);
  p = fma_sc(p, r, 1.0 / 5040.0);
  p = fma_sc(p, r, 1.0 / 720.0);
  p = fma_sc(p, r, 1.0 / 120.0);
  p = fma_sc(p, r, 1.0 / 24.0);
  p = fma_sc(p, r, 1.0 / 6.0);
  p = fma(p, r, 0.5);
  p = fma(p, r, 1.0);
  p = fma(p, r, 1.0);
  return __builtin_ldexp(p, (int)kf);
}

// det_exp_ldexp() for arguments already known to be in [-708, 708] (no NaN, no overflow, result normal): the same operation
// sequence without the three range cases.  closed_rates() tests the wavefront's arguments of a stage together (one compare each,
// one ballot) and takes this path when every lane qualifies -- always, on physical parameters.
__device__ __forceinline__ double det_exp_inrange(double x) {
  const double kf = rint(x * 0x1.71547652b82fep+0);
  double r = fma(-kf, 0x1.62e42fee00000p-1, x);
  r = fma(-kf, 0x1.a39ef35793c76p-33, r);
  double p = 1.0 / 6227020800.0;
  p = fma_sc(p, r, 1.0 / 479001600.0);
  p = fma_sc(p, r, 1.0 / 39916800.0);
  p = fma_sc(p, r, 1.0 / 3628800.0);
  p = fma_sc(p, r, 1.0 / 362880.0);
  p = fma_sc(p, r, 1.0 / 40320.0);
  p = fma_sc(p, r, 1.0 / 5040.0);
  p = fma_sc(p, r, 1.0 / 720.0);
  p = fma_sc(p, r, 1.0 / 120.0);
  p = fma_sc(p, r, 1.0 / 24.0);
  p = fma_sc(p, r, 1.0 / 6.0);
  p = fma(p, r, 0.5);
  p = fma(p, r, 1.0);
  p = fma(p, r, 1.0);
  return __builtin_ldexp(p, (int)kf);
}

// det_exp for the MLP kernels' rate terms: same operation sequence, constants as scalar operands (fma_sc), scaling by one
// v_ldexp_f64 (bit-identical, det_exp_ldexp below) -- 36 instead of 62 vector instructions per call.
__device__ __forceinline__ double det_exp_s(double x) {
  // branch-free: the range cases are selects behind the polynomial (in-range arguments take the same operations as det_exp;
  // out-of-range arguments compute a discarded value), so two calls interleave instead of running under exec masks
  const double kf = rint(x * 0x1.71547652b82fep+0);
  double r = fma(-kf, 0x1.62e42fee00000p-1, x);
  r = fma(-kf, 0x1.a39ef35793c76p-33, r);
  double p = 1.0 / 6227020800.0;
  p = fma_sc(p, r, 1.0 / 479001600.0);
  p = fma_sc(p, r, 1.0 / 39916800.0);
  p = fma_sc(p, r, 1.0 / 3628800.0);
  p = fma_sc(p, r, 1.0 / 362880.0);
  p = fma_sc(p, r, 1.0 / 40320.0);
  p = fma_sc(p, r, 1.0 / 5040.0);
  p = fma_sc(p, r, 1.0 / 720.0);
  p = fma_sc(p, r, 1.0 / 120.0);
  p = fma_sc(p, r, 1.0 / 24.0);
  p = fma_sc(p, r, 1.0 / 6.0);
  p = fma(p, r, 0.5);
  p = fma(p, r, 1.0);
  p = fma(p, r, 1.0);
  double e = __builtin_ldexp(p, (int)kf);  // == (p * 2^k1) * 2^(k - k1), see det_exp_ldexp
  e = (x > 709.782712893384) ? __builtin_inf() : e;
  e = (x < -745.1332191019412) ? 0.0 : e;
  return (x != x) ? x : e;
}

// a / b when rb = RN(1 / b) is at hand: q0 = RN(a * rb) is a faithful quotient, and one correction step with the exact
// remainder r = a - b*q0 (fma) gives RN(a / b) -- the correctly rounded IEEE quotient, bit for bit what `a / b` returns
// (Markstein 1990; holds barring over/underflow: operands here are times in ms, voltages in mV and O(1) ratios).  Three
// fp64 VALU operations instead of the ~12-instruction v_div_scale / v_rcp / Newton / v_div_fmas / v_div_fixup sequence;
// the divisions by prot_dt (2 per protocol lookup), by 5 (det_root5) and by the step length (every dense-output sample)
// were ~3/4 of the closed-form kernels' issue work.  Zero, infinite and NaN quotients are passed through unchanged
// (the correction would turn inf into NaN and lose the sign of a zero).
__device__ __forceinline__ double div_by(double a, double b, double rb) {
  const double q0 = a * rb;
  const double r = fma(-b, q0, a);
  const double q1 = fma(r, rb, q0);
  const double aq = __builtin_fabs(q0);
  return (aq > 0.0 && aq < __builtin_inf()) ? q1 : q0;
}

// a / b for 0 <= a <= b with b a finite positive step length (every dense-output sample: x = (t_k - t0) / (t1 - t0), t_k in
// (t0, t1]): the quotient is 0 or in [2^-70, 1], so the pass-through guard of div_by() -- four vector instructions of the ~45 a
// dense-output sample costs -- is dead weight.  A zero stays +0 through both fma.
__device__ __forceinline__ double div_pos(double a, double b, double rb) {
  const double q0 = a * rb;
  return fma(fma(-b, q0, a), rb, q0);
}

// a / b for a compile-time constant b (rb = RN(1 / b)): the same correction step, with the true division kept for the quotients
// the proof excludes (zero, subnormal range, overflow).  fp32: checked against x / 1000.0f for all 2^32 inputs -- they differ only
// where |quotient| < 2^-126 (67 108 inputs, all |x| < 9.5e-38); the guards below are far inside the safe range
// (tests/test_gpu_math_probe.py runs that sweep with the guards in place: no input differs).
__device__ __forceinline__ double div_const(double a, double b, double rb) {
  const double q0 = a * rb;
  const double r = fma(-b, q0, a);
  const double q1 = fma(r, rb, q0);
  const double aq = __builtin_fabs(q0);
  return (aq > 0x1p-900 && aq < 0x1p+900) ? q1 : a / b;
}
__device__ __forceinline__ float div_constf(float a, float b, float rb) {
  const float q0 = a * rb;
  const float r = fmaf(-b, q0, a);
  const float q1 = fmaf(r, rb, q0);
  const float aq = __builtin_fabsf(q0);
  return (aq > 0x1p-100f && aq < 0x1p+100f) ? q1 : a / b;
}

__device__ __forceinline__ double det_root5(double x) {
  if (!(x < __builtin_inf()) || !(x > 0.0)) return x;
  unsigned long long u = (unsigned long long)__double_as_longlong(x);
  u = u / 5ull + 0x3325999999999999ull;
  double y = __longlong_as_double((long long)u);
#pragma unroll
  for (int it = 0; it < 7; ++it) {
    const double y2 = y * y;
    const double y4 = y2 * y2;
    y = div_by(4.0 * y + x / y4, 5.0, 0.2);  // 0.2 == RN(1/5)
  }
  return y;
}

template <typename S> struct Real;
template <> struct Real<float> {
  static __device__ __forceinline__ float sqrt_(float x) { return sqrtf(x); }
  static __device__ __forceinline__ float prev_(float x) { return nextafterf(x, x - 1.0f); }
};
template <> struct Real<double> {
  static __device__ __forceinline__ double sqrt_(double x) { return sqrt(x); }
  static __device__ __forceinline__ double prev_(double x) { return nextafter(x, x - 1.0); }
};

// Diagnostic build only (make EXTRA=-DIONODE_STAMPS): s_memtime phase stamps of workgroup 0 / wavefront 0, summed
// in SGPR-side 64-bit counters and written to step_log[0..15] at kernel end (no stamp executes in the real build).
#ifdef IONODE_STAMPS
struct Stamps {
  unsigned long long acc[16];
  unsigned long long last;
};
__device__ __forceinline__ unsigned long long stamp_now() {
  unsigned long long t;
  asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
  return t;
}
#define STAMP_DECL Stamps stamps_; for (int i_ = 0; i_ < 16; ++i_) stamps_.acc[i_] = 0; stamps_.last = stamp_now();
#define STAMP(st, slot) do { __builtin_amdgcn_sched_barrier(0); const unsigned long long n_ = stamp_now(); (st).acc[slot] += n_ - (st).last; (st).last = n_; __builtin_amdgcn_sched_barrier(0); } while (0)
#define MSTAMP(slot) STAMP(*sp, slot)   // inside a net struct (its sp member)
#else
#define STAMP_DECL
#define STAMP(st, slot) do { } while (0)
#define MSTAMP(slot) do { } while (0)
#endif

__device__ __forceinline__ double bcast_f64(double x, int src) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(x), src);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(x), src);
  return __hiloint2double(hi, lo);
}
__device__ __forceinline__ float bcast_f32(float x, int src) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), src));
}
template <typename S> __device__ __forceinline__ S bcast(S x, int src);
template <> __device__ __forceinline__ double bcast<double>(double x, int src) { return bcast_f64(x, src); }
template <> __device__ __forceinline__ float bcast<float>(float x, int src) { return bcast_f32(x, src); }

// x moved across lanes by a DPP row operation (VALU speed; __shfl_xor takes two LDS-crossbar round trips for a double)
template <int CTRL, int ROWMASK> __device__ __forceinline__ double dpp_f64(double x) {
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(x), CTRL, ROWMASK, 0xf, false);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(x), CTRL, ROWMASK, 0xf, false);
  return __hiloint2double(hi, lo);
}

// Sum over each group of 8 consecutive lanes (3 DPP steps); every lane of the group holds the group's sum.
__device__ __forceinline__ double group8_sum_f64(double x) {
  x = x + dpp_f64<0xB1, 0xf>(x);   // quad_perm [1,0,3,2]
  x = x + dpp_f64<0x4E, 0xf>(x);   // quad_perm [2,3,0,1]
  x = x + dpp_f64<0x141, 0xf>(x);  // row_half_mirror
  return x;
}

// Number of set bits of m below this lane (+ acc): v_mbcnt_lo / v_mbcnt_hi chain.
__device__ __forceinline__ int mbcnt(unsigned long long m, int acc = 0) {
  return __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, acc));
}

// nn.LeakyReLU(0.01): x > 0 ? x : 0.01*x  ==  max(x, 0.01*x) for every input (incl. +-0, NaN): 2 VALU ops
// fmaxf() makes hipcc canonicalise its operands first (v_max_f32 x, x, x: one dead vector instruction per MFMA result register -- 1280
// in the N <= 16 kernel at 64 per wavefront); the v_max_f32 instruction itself returns the same bits for every non-NaN input and quiets
// NaNs on its own (IEEE mode), so it is issued directly.  The multiply stays hipcc's: it is the first reader of the MFMA result and
// gets the required wait states; the asm reads its output, so it can only follow it.
__device__ __forceinline__ float lrelu(float x) {
  const float t = x * 0.01f;
  float h;
  asm("v_max_f32 %0, %1, %2" : "=v"(h) : "v"(x), "v"(t));
  return h;
}

template <typename S, int D> __device__ __forceinline__ S rms_norm(const S *x) {
  S s = x[0] * x[0];
#pragma unroll
  for (int i = 1; i < D; ++i) s = s + x[i] * x[i];
  s = s / (S)D;
  return Real<S>::sqrt_(s);
}
template <typename S> __device__ __forceinline__ S abs_(S x) { return x < 0 ? -x : x; }

}  // namespace ionode
