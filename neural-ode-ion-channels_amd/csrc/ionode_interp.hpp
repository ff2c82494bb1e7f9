// ionode_interp.hpp -- torchdiffeq's 4th-order dense-output interpolant and the observation model, defined ONCE for the forward solve
// (ionode_attempt_body.hpp, every emission path), the deferred expansion (ionode_dense_expand.hpp) and the fused sum-of-squares
// gradient (ionode_grad.hpp, ionode_grad_gc.hpp, ionode_grad_sweep_body.hpp).  Every output bit of the forward depends on this
// arithmetic and the gradient re-evaluates the forward's samples from a step's checkpoint, so the bit parity between them comes from
// calling the routines below -- under one set of build flags (-ffp-contract=off) -- and not from keeping copies in step.
//   fit       (y0, y1, k1, k7, y_mid) -> five coefficients (e, d, c, b, a) per component, in the state dtype (_interp_fit)
//   evaluate  x = (t_k - t0) / (t1 - t0) in fp64, cast to the state dtype; running powers (_interp_evaluate)
//   observe   i = g gate(y) (V - E)
// and the layout in which a step's interpolant travels: an LDS row of the lane-wise kernels, a record of the deferring tile.
#pragma once

#include "ionode_math.hpp"

namespace ionode {

// Doubles of one step's interpolant, for a D known at run time only (the host-side LDS plan); InterpRow<D> otherwise.
__host__ __device__ constexpr int interp_row_doubles(int D) { return 4 + 5 * D; }

// The row: [T0] t0  [DEN] t1 - t0  [RDEN] 1 / den  [SPARE] 8 bytes of the holder's own (an output cursor)  [coef(c, d)] coefficient
// c of component d.  Coefficients are stored as doubles and cast back to the state dtype (exact for fp32).  16-byte chunks: the
// header is chunks 0 and 1, component pairs (d, d + 1) of one coefficient share a chunk.
template <int D> struct InterpRow {
  static constexpr int ROW = interp_row_doubles(D);
  static constexpr int BYTES = ROW * 8;
  static constexpr int CHUNKS = ROW / 2;
  static constexpr int T0 = 0, DEN = 1, RDEN = 2, SPARE = 3, COEF = 4;
  static __host__ __device__ constexpr int coef(int c, int d) { return COEF + c * D + d; }
  static_assert(D % 2 == 0, "rows hold component pairs in whole 16-byte chunks");
};

// ---- fit ----
// The five coefficients c5[0..4] of component d (a constant once unrolled), given the weights of the midpoint state
// bm[j] = dts c_mid[j]: y_mid = y0 + sum_j bm[j] k_j.  One component per call: the lane-wise kernels fit two at a time, so that at
// most 10 of the 5 x D coefficients are live.
template <typename S, int D>
__device__ __forceinline__ void interp_fit(S dts, const S (&bm)[7], const S *y0, const S *y1, const S (&k)[7][D], int d, S *c5) {
  S s = k[0][d] * bm[0];
#pragma unroll
  for (int jx = 1; jx < 7; ++jx) s = s + k[jx][d] * bm[jx];
  const S YM = y0[d] + s;
  const S F0 = k[0][d], F1 = k[6][d], Y0 = y0[d], Y1 = y1[d];
  c5[4] = ((S)2 * dts) * (F1 - F0) - (S)8 * (Y1 + Y0) + (S)16 * YM;
  c5[3] = dts * ((S)5 * F0 - (S)3 * F1) + (S)18 * Y0 + (S)14 * Y1 - (S)32 * YM;
  c5[2] = dts * (F1 - (S)4 * F0) - (S)11 * Y0 - (S)5 * Y1 + (S)16 * YM;
  c5[1] = dts * F0;
  c5[0] = Y0;
}

// ... of every component
template <typename S, int D>
__device__ __forceinline__ void interp_fit_all(S dts, const S *y0, const S *y1, const S (&k)[7][D], S (&cf)[5][D]) {
  S bm[7];
#pragma unroll
  for (int jx = 0; jx < 7; ++jx) bm[jx] = dts * (S)kCmid[jx];
#pragma unroll
  for (int d = 0; d < D; ++d) {
    S c5[5];
    interp_fit<S, D>(dts, bm, y0, y1, k, d, c5);
#pragma unroll
    for (int c = 0; c < 5; ++c) cf[c][d] = c5[c];
  }
}

// The step's end state in the forward's order, y1 = y0 + sum_j (beta5[j] dts) k_j, for a reader that has the checkpoint only
// (the trajectory's last step: no next record holds it).
template <typename S, int D> __device__ __forceinline__ void interp_y1(S dts, const S *y0, const S (&k)[7][D], S *y1) {
  S bd[6];
#pragma unroll
  for (int jx = 0; jx < 6; ++jx) bd[jx] = (S)kBeta[5][jx] * dts;
#pragma unroll
  for (int d = 0; d < D; ++d) {
    S sm = k[0][d] * bd[0];
#pragma unroll
    for (int jx = 1; jx < 6; ++jx) sm = sm + k[jx][d] * bd[jx];
    y1[d] = y0[d] + sm;
  }
}

// ---- evaluate ----
// x of output time tk: the fp64 quotient (tk - t0) / den, correctly rounded through the step's one reciprocal rden = 1 / den
// (div_pos), THEN cast to the state dtype.
template <typename S> __device__ __forceinline__ S interp_x(double tk, double t0, double den, double rden) {
  return (S)div_pos(tk - t0, den, rden);
}

// out = cb0 + x cb1 + x^2 cb2 + x^3 cb3 + x^4 cb4 by running powers, in this order and unfused.  X: one sample (S) or several (an
// ext_vector_type of S: the work-list emission).
template <typename S, int D, typename X> __device__ __forceinline__ void interp_eval(const S (&cb)[5][D], X x, X (&out)[D]) {
  X xp = x;
#pragma unroll
  for (int d = 0; d < D; ++d) out[d] = cb[0][d] + x * cb[1][d];
#pragma unroll
  for (int c = 2; c < 5; ++c) {
    xp = xp * x;
#pragma unroll
    for (int d = 0; d < D; ++d) out[d] = out[d] + xp * cb[c][d];
  }
}

// ---- observe ----
// i = g gate(y) (V - E): gate and conductance in the state dtype, the driving force in fp64.  A: KArgs or GArgs.
template <typename S, int D, typename A> __device__ __forceinline__ double obs_current(const A &a, const S *y, double v) {
  S gate;
  if (a.obs_open) gate = y[D - 1]; else gate = y[0] * y[1];
  if (a.obs_g != 1.0) gate = (S)a.obs_g * gate;
  return (double)gate * (v - a.obs_e);
}

// ---- the fused objective's residual term ----
// What one sample's residual rr = i_k - ref_k adds to its trajectory's sum: rr^2 (obj_abs == 0, the sum of squares) or |rr| (1, the
// reference's prediction loss torch.mean(torch.abs(pred_yo - data)) times the sample count).  obj_abs is wave-uniform (KArgs), read at
// run time: the summation trees around the term are the same for both kinds, and a kind per instantiation would double the kernels.
// A wave-uniform BRANCH, which the empty asm keeps hipcc from turning into a select: as a select (an and, two v_cndmask per sample)
// the squares of the 6-state table kernel, which runs one wavefront per SIMD and pays for every instruction, came out 2.8 % slower
// (profiles/objective_kinds.md).  Kernels whose KernelForm::objective_kinds is false pass 0 and keep the multiply alone.
__device__ __forceinline__ double residual_term(double rr, int obj_abs) {
  if (__builtin_expect(obj_abs != 0, 0)) {
    asm volatile("");
    return fabs(rr);
  }
  return rr * rr;
}
// ... of the N residuals a lane holds for one chunk of the work-list emission, in place: one branch for the N of them.
template <int N> __device__ __forceinline__ void residual_terms(double (&rr)[N], int obj_abs) {
  if (__builtin_expect(obj_abs != 0, 0)) {
#pragma unroll
    for (int u = 0; u < N; ++u) rr[u] = residual_term(rr[u], 1);
  } else {
#pragma unroll
    for (int u = 0; u < N; ++u) rr[u] = residual_term(rr[u], 0);
  }
}

// ... and in the gradient: d term / d rr times the upstream scalar g = dL/dsum[b], the adjoint weight of the sample's residual.
//   obj_abs == 0   (2 g) rr, in this order: the bits the backward sweep formed before it knew a second kind
//   obj_abs == 1   g sign(rr), with sign(0) = 0 and sign(NaN) = NaN as torch.abs's backward has them (rr itself is returned for
//                  both: g * (+-0) is the zero, g * NaN the NaN)
// The sweeps pass obj_abs as a literal from either side of ONE wave-uniform branch per step and trajectory (sse_step_samples,
// ionode_grad.hpp), so a sample pays no select; the sample-0 term, once per trajectory, passes KArgs::obj_abs itself.
__device__ __forceinline__ double residual_weight(double rr, double g, int obj_abs) {
  if (__builtin_expect(obj_abs != 0, 0)) {
    const double sg = rr > 0.0 ? 1.0 : (rr < 0.0 ? -1.0 : rr);
    return g * sg;
  }
  return (2.0 * g) * rr;
}

// ---- one step's interpolant, wave-uniform, as an emission loop holds it ----
template <typename S, int D> struct Interp {
  using R = InterpRow<D>;
  double t0, den, rden;
  S cb[5][D];

  // from a row in LDS, read at a uniform address (broadcast ds_read_b128)
  __device__ __forceinline__ void from_row(const double2 *rj) {
    const double2 h0 = rj[0];
    t0 = h0.x; den = h0.y; rden = rj[1].x;
#pragma unroll
    for (int c = 0; c < 5; ++c)
#pragma unroll
      for (int d = 0; d < D; d += 2) {
        const double2 cc = rj[R::coef(c, d) / 2];
        cb[c][d] = (S)cc.x; cb[c][d + 1] = (S)cc.y;
      }
  }
  // from lane jj's registers (the MLP tiles keep the fit there)
  __device__ __forceinline__ void from_lanes(double t0_, double den_, double rden_, const S (&ic)[5][D], int jj) {
    t0 = bcast_f64(t0_, jj); den = bcast_f64(den_, jj); rden = bcast_f64(rden_, jj);
#pragma unroll
    for (int c = 0; c < 5; ++c)
#pragma unroll
      for (int d = 0; d < D; ++d) cb[c][d] = bcast<S>(ic[c][d], jj);
  }
  // from a row held one double per lane (lane e has double e: one vector load per record)
  __device__ __forceinline__ void from_lane_doubles(double raw) {
    t0 = bcast_f64(raw, R::T0); den = bcast_f64(raw, R::DEN); rden = bcast_f64(raw, R::RDEN);
#pragma unroll
    for (int c = 0; c < 5; ++c)
#pragma unroll
      for (int d = 0; d < D; ++d) cb[c][d] = (S)bcast_f64(raw, R::coef(c, d));
  }
  __device__ __forceinline__ S x(double tk) const { return interp_x<S>(tk, t0, den, rden); }
};

}  // namespace ionode
