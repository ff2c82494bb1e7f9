// ionode_grad_gc.hpp -- the fused sum-of-squares objective in the two-phase sweep (NN-f / NN-d; ionode_grad.hpp).
//
// The two-phase sweep needs the output gradients dL/dy_k in one place only: the reduction of a step's samples into the
// interpolant-coefficient adjoints G_c[5][D] of the step's packet (pkt::GC), plus the sample-0 term of dL/dy0.  For the objective
// sse[b] = sum_k (i_k - ref_k)^2 both depend on the step's checkpoint, the protocol, the reference trace and the upstream scalar
// dL/dsse[b] -- not on the net and not on the adjoint.  ionode_grad_sse_gc_kernel forms them for every (trajectory, step) of a
// chunk: the recompute kernel then runs with grad_y == NULL (it leaves the GC slots alone) and the walk takes the sample-0 term
// from a [B][D] buffer, so no [B][Nt] array exists anywhere on the route.  The sum of absolute values, sae[b] = sum_k |i_k - ref_k|
// (GArgs::k.obj_abs = 1, ionode_objective_backward_gc), differs in the samples' weights alone: residual_weight (ionode_interp.hpp).
//
// The step's dense-output fit and the per-sample term are sse_fit_step / sse_sample_term (ionode_grad.hpp), which the closed-form
// one-phase sweep (ionode_grad_sweep_body.hpp, SSE = true) calls too; both stand on the forward's interpolant (ionode_interp.hpp).
#pragma once

#include "ionode_grad.hpp"

namespace ionode {

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
  const double gb = a.grad_sse[b];

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
      double ys[D], ks[7][D];
#pragma unroll
      for (int d = 0; d < D; ++d) ys[d] = rec[CK::Y + d];
#pragma unroll
      for (int jx = 0; jx < 7; ++jx)
#pragma unroll
        for (int d = 0; d < D; ++d) ks[jx][d] = rec[CK::K + jx * D + d];
      S cf[5][D];
      sse_fit_step<S, D>(rec[CK::DT], ys, ks, (s + 1 < nst && s + 1 < a.ckpt_cap) ? rec + RECW + CK::Y : nullptr, cf);
      const double den = t1 - t0, rden = 1.0 / den;   // the forward's reciprocal and div_pos: the same x bits
      sse_step_samples(a.k.obj_abs, [&](auto kind) {
        for (int c0 = 0; c0 < n; c0 += 64) {
          const int idx = oi + c0 + lane;
          if (c0 + lane < n && idx >= 0 && idx < Nt) {
            const double tk = a.k.t_eval[idx];
            const S xs = interp_x<S>(tk, t0, den, rden);
            double vk;
            if (vt) vk = vt[idx];
            else protocol_v(a.k, pv, tk, vk);
            sse_sample_term<S, D, decltype(kind)::value>(a, cf, xs, vk, ref[idx], gb, P);
          }
        }
      });
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
    const double gr = residual_weight(sse_residual<S, D>(a, y0s, v0, ref[0], dr), gb, a.k.obj_abs);
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
