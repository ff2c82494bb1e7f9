// ionode_grad_gc.hpp -- the fused sum-of-squares objective in the two-phase sweep (NN-f / NN-d; ionode_grad.hpp).
//
// The two-phase sweep needs the output gradients dL/dy_k in one place only: the reduction of a step's samples into the
// interpolant-coefficient adjoints G_c[5][D] of the step's packet (pkt::GC), plus the sample-0 term of dL/dy0.  For the objective
// sse[b] = sum_k (i_k - ref_k)^2 both depend on the step's checkpoint, the protocol, the reference trace and the upstream scalar
// dL/dsse[b] -- not on the net and not on the adjoint.  ionode_grad_sse_gc_kernel forms them for every (trajectory, step) of a
// chunk: the recompute kernel then runs with grad_y == NULL (it leaves the GC slots alone) and the walk takes the sample-0 term
// from a [B][D] buffer, so no [B][Nt] array exists anywhere on the route.
//
// The step's dense-output fit and the per-sample term are the device functions below: the algebra of the closed-form one-phase
// sweep (ionode_grad_sweep_body.hpp, SSE = true), which keeps its own copy (it compiles to the code it had).
#pragma once

#include "ionode_grad.hpp"

namespace ionode {

// The dense-output coefficients (e, d, c, b, a) of an accepted step, fitted from its checkpoint record as the forward fitted them
// (ionode_attempt_body.hpp `fit`, state dtype: the same bits).  rec1: the next accepted step's record (its y is this step's y1), or
// NULL for the trajectory's last step, whose y1 is recomputed in the forward's order.
template <typename S, int D>
__device__ __forceinline__ void sse_fit_step(const double *__restrict__ rec, const double *__restrict__ rec1, S (&cf)[5][D]) {
  using CK = CkptRecord<D>;
  const S dts_s = (S)rec[CK::DT];
  S ys[D], y1[D], ks[7][D];
#pragma unroll
  for (int d = 0; d < D; ++d) ys[d] = (S)rec[CK::Y + d];
#pragma unroll
  for (int jx = 0; jx < 7; ++jx)
#pragma unroll
    for (int d = 0; d < D; ++d) ks[jx][d] = (S)rec[CK::K + jx * D + d];
  if (rec1) {
#pragma unroll
    for (int d = 0; d < D; ++d) y1[d] = (S)rec1[CK::Y + d];
  } else {
    S bd[6];
#pragma unroll
    for (int jx = 0; jx < 6; ++jx) bd[jx] = (S)kBeta[5][jx] * dts_s;
#pragma unroll
    for (int d = 0; d < D; ++d) {
      S sm = ks[0][d] * bd[0];
#pragma unroll
      for (int jx = 1; jx < 6; ++jx) sm = sm + ks[jx][d] * bd[jx];
      y1[d] = ys[d] + sm;
    }
  }
  S bm[7];
#pragma unroll
  for (int jx = 0; jx < 7; ++jx) bm[jx] = dts_s * (S)kCmid[jx];
#pragma unroll
  for (int d = 0; d < D; ++d) {
    S sm = ks[0][d] * bm[0];
#pragma unroll
    for (int jx = 1; jx < 7; ++jx) sm = sm + ks[jx][d] * bm[jx];
    const S YM = ys[d] + sm;
    const S F0 = ks[0][d], F1 = ks[6][d], Y0 = ys[d], Y1 = y1[d];
    cf[4][d] = ((S)2 * dts_s) * (F1 - F0) - (S)8 * (Y1 + Y0) + (S)16 * YM;
    cf[3][d] = dts_s * ((S)5 * F0 - (S)3 * F1) + (S)18 * Y0 + (S)14 * Y1 - (S)32 * YM;
    cf[2][d] = dts_s * (F1 - (S)4 * F0) - (S)11 * Y0 - (S)5 * Y1 + (S)16 * YM;
    cf[1][d] = dts_s * F0;
    cf[0][d] = Y0;
  }
}

// One output sample of the step: y_k from the interpolant at x (state dtype, the forward's running powers), its residual against
// `ref` at voltage v, and P[c][d] += g2 r_k dr_k/dy_d x^c in fp64 (g2 = 2 dL/dsse[b]).
template <typename S, int D>
__device__ __forceinline__ void sse_sample_term(const GArgs &a, const S (&cf)[5][D], S xs, double v, double ref, double g2, double (&P)[5][D]) {
  S out[D];
  S xq = xs;
#pragma unroll
  for (int d = 0; d < D; ++d) out[d] = cf[0][d] + xs * cf[1][d];
#pragma unroll
  for (int c = 2; c < 5; ++c) {
    xq = xq * xs;
#pragma unroll
    for (int d = 0; d < D; ++d) out[d] = out[d] + xq * cf[c][d];
  }
  double dr[D];
  const double gr = g2 * sse_residual<S, D>(a, out, v, ref, dr);
  const double x = (double)xs;
  double xp = 1.0;
#pragma unroll
  for (int c = 0; c < 5; ++c) {
#pragma unroll
    for (int d = 0; d < D; ++d) P[c][d] += (gr * dr[d]) * xp;
    xp *= x;
  }
}

constexpr int GRAD_GC_WAVES = 4;   // wavefronts (= iterations) per workgroup: grid.y stays inside HIP's 65535 for the chunks the recompute kernel takes

// G_c of the fused objective for every (trajectory, iteration) of the chunk [it_begin, it_end): grid (B, ceil(iterations / 4)),
// one wavefront per (trajectory b, step s = nacc[b] - 1 - it), lanes = the step's output samples, 64 per pass.  Everything of the
// trajectory and the step is wave-uniform (scalar loads, all of them in front of the kernel's stores); the ten sums meet through
// lane shuffles: no LDS, no scratch.  Lane 0 writes G_c into the packet the recompute kernel fills (zeros where there is no step
// or no sample); the wavefront of the sweep's last iteration also writes the sample-0 term of dL/dy0 into sse_y0[b].
template <typename S>
__global__ void __launch_bounds__(64 * GRAD_GC_WAVES) ionode_grad_sse_gc_kernel(const GArgs a) {
  constexpr int D = 2;
  using CK = CkptRecord<D>;
  constexpr int RECW = CK::WIDTH;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int b = blockIdx.x;
  const int it = a.it_begin + (int)blockIdx.y * GRAD_GC_WAVES + wave;
  if (b >= a.k.B || it >= a.it_end) return;   // (wave-uniform; the kernel has no barrier)
  const int Nt = a.k.Nt;
  const int nst = a.nacc[b];
  const int s = nst - 1 - it;
  const int pidx = a.k.prot_of_traj ? a.k.prot_of_traj[b] : (b % a.k.P);
  const double *__restrict__ pv = a.k.prot_v + (size_t)pidx * a.k.Np;
  const double *__restrict__ ref = a.sse_ref + (size_t)pidx * Nt;
  const double *__restrict__ vt = a.v_tab ? a.v_tab + (size_t)pidx * Nt : nullptr;
  const double *__restrict__ ck = a.ckpt + (size_t)b * a.ckpt_cap * RECW;
  const double g2 = 2.0 * a.grad_sse[b];

  double P[5][D];
#pragma unroll
  for (int c = 0; c < 5; ++c)
#pragma unroll
    for (int d = 0; d < D; ++d) P[c][d] = 0.0;
  if (s >= 0 && s < a.ckpt_cap) {
    const double *__restrict__ rec = ck + (size_t)s * RECW;
    const double t0 = rec[CK::T0], t1 = t0 + rec[CK::DT];
    const int oi = (int)rec[CK::OI], n = (int)rec[CK::NOUT];
    if (n > 0) {
      S cf[5][D];
      sse_fit_step<S, D>(rec, (s + 1 < nst && s + 1 < a.ckpt_cap) ? rec + RECW : nullptr, cf);
      const double den = t1 - t0, rden = 1.0 / den;   // the forward's reciprocal and div_pos: the same x bits
      for (int c0 = 0; c0 < n; c0 += 64) {
        const int idx = oi + c0 + lane;
        if (c0 + lane < n && idx >= 0 && idx < Nt) {
          const double tk = a.k.t_eval[idx];
          const S xs = (S)div_pos(tk - t0, den, rden);
          double vk;
          if (vt) vk = vt[idx];
          else protocol_v(a.k, pv, tk, vk);
          sse_sample_term<S, D>(a, cf, xs, vk, ref[idx], g2, P);
        }
      }
#pragma unroll
      for (int m = 32; m >= 1; m >>= 1)
#pragma unroll
        for (int c = 0; c < 5; ++c)
#pragma unroll
          for (int d = 0; d < D; ++d) P[c][d] += __shfl_xor(P[c][d], m);
    }
  }

  // sample 0 of the objective is y0 itself (the forward's initial residual); the first checkpoint holds y0
  const bool last = it == a.n_iter - 1;
  double s0[D];
#pragma unroll
  for (int d = 0; d < D; ++d) s0[d] = 0.0;
  if (last && nst > 0) {
    S y0s[D];
#pragma unroll
    for (int d = 0; d < D; ++d) y0s[d] = (S)ck[CK::Y + d];
    double v0;
    if (vt) v0 = vt[0];
    else protocol_v(a.k, pv, a.k.t_eval[0], v0);
    double dr[D];
    const double gr = g2 * sse_residual<S, D>(a, y0s, v0, ref[0], dr);
#pragma unroll
    for (int d = 0; d < D; ++d) s0[d] = gr * dr[d];
  }

  if (lane == 0) {
    const size_t tstep = (size_t)(b >> 4) * (a.it_end - a.it_begin) + (it - a.it_begin);   // the recompute kernel's packet address
    double *__restrict__ pk = a.packets + (tstep * 16 + (b & 15)) * GRAD_PACKET;
#pragma unroll
    for (int c = 0; c < 5; ++c)
#pragma unroll
      for (int d = 0; d < D; ++d) pk[pkt::GC + c * D + d] = P[c][d];
    if (last) {
#pragma unroll
      for (int d = 0; d < D; ++d) a.sse_y0[(size_t)b * D + d] = s0[d];
    }
  }
}

}  // namespace ionode
