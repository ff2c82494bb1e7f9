// ionode_tangent_nn.hpp -- gfx950 device code of the TANGENT (forward-mode) sweep for NN-f / NN-d: the per-sample sensitivities
// dI(t_k)/dp_j of the current trace and their Gauss-Newton sums, as ionode_tangent.hpp has them for the closed-form models.
//
// No MLP work is in here.  The state the net sees is one scalar, a, and the two-phase reverse sweep's recompute kernel
// (ionode_grad_recompute_kernel, ionode_grad.hpp) already leaves the net's whole Jacobian with respect to it -- pkt::C, d net / d x1 at
// unit seed -- in the 64-double packet of every (trajectory, accepted step, stage), beside the stage voltage, the stage inputs and the
// rate exponentials (ionode_grad_step.hpp).  With grad_y == NULL and records == NULL that kernel writes exactly those and nothing else.
// What is left is sequential: ionode_tangent_walk_kernel walks the packets FORWARD in time.
//
// What is differentiated: what ionode_grad_walk_kernel differentiates, so that J^T w equals its dL/dp -- accepted steps (t0, dt) are
// constants, rejected attempts contribute nothing, FSAL and the 4th-order dense output are differentiated as written, the (float) casts
// on the net's inputs are the identity, the rates are k = p E with the packet's exponentials (dk/dp_2q = E, dk/dp_2q+1 = +-V k: no
// division by a parameter).  S = dy/dp is 2 x 8, zero at y0, fp64 whatever the state dtype; per parameter column j and stage i
// (packet slot e = 5 - i)
//     Yd_i        = S + dts sum_{m <= i} beta_im Kd_m+1
//     Kd_i+2 [a]  = (c_i / 1000 - [NN-d] (k1 + k2)) Yd_i[a] + [NN-d] df_a/dp_j (Y_i, V_i)
//     Kd_i+2 [r]  = -(k3 + k4) Yd_i[r] + df_r/dp_j (Y_i, V_i)
// with c_i / 1000 formed in fp64, Kd_1 the previous step's Kd_7 (first step: the INITEV packet's slot e = 0, the evaluation at
// (t_eval[0], y0), where S = 0) and S <- Yd_5.  NN-f: the columns p1..p4 are identically zero (its packets carry E1 = E2 = 0).
// Output samples: tangent_sample (ionode_tangent.hpp) on interp_fit / interp_eval of the tangents; y_k is re-evaluated from the step's
// checkpoint in the state dtype.  Checker: tests/tangent_nn_check.py.
//
// Execution model: ionode_tangent_sweep_kernel's 2-state mapping -- one lane per (trajectory, parameter), eight lanes per trajectory,
// eight trajectories per wavefront, a workgroup is one wavefront; J^T J rows through __shfl inside the group; no LDS, no atomics.
// A trajectory with nst accepted steps has its step s at iteration it = nst - 1 - s and its initial evaluation at it = nst (the
// reverse sweep's numbering: the packets' address), so forward in time is DESCENDING it; the trajectories of a wavefront sit at
// different steps of their own, finished or not yet started ones are predicated off.  Packets cost 8 KiB per (16-trajectory tile,
// iteration), so the sweep is chunked over iterations: chunks are visited from [n_iter - c, n_iter) down to [0, c), GArgs::state
// carries S, Kd_7 and the running sums per lane between the launches ([B][8][TANGENT_NN_LANE_STATE]), the launch with it_begin == 0
// writes jtr / jtj, di_dp rows are written as their steps are walked.  One summation order per trajectory (sample order), whatever
// the chunking and the batch around it.
#pragma once

#include "ionode_tangent.hpp"   // TArgs, tangent_pick, tangent_drate, tangent_sample

namespace ionode {

constexpr int TANGENT_NN_LANE_STATE = 2 * 2 + 1 + 8;                  // S[2], Kd_7[2], jtr, jtj row [8] of one (trajectory, parameter)
constexpr int TANGENT_NN_STATE = 8 * TANGENT_NN_LANE_STATE;           // doubles per trajectory

// inst_tangent_nn.hip: model IONODE_MODEL_NNF | IONODE_MODEL_NND.  a.g: packets, state, it_begin, it_end, n_iter beside what
// launch_tangent reads.
void launch_tangent_nn(int model, int f32, const TArgs &a, hipStream_t s);

template <int MODEL, typename S>
__global__ void __launch_bounds__(64) ionode_tangent_walk_kernel(const TArgs ta) {
  constexpr int D = ModelTraits<MODEL>::D, NPAR = ModelTraits<MODEL>::NPAR, NR = NPAR / 2;
  static_assert(ModelTraits<MODEL>::MLP && D == 2 && NPAR == 8, "NN-f / NN-d");
  constexpr bool NND = MODEL == IONODE_MODEL_NND;
  constexpr int GROUP = 8, TPW = 8;
  constexpr int HH = IONODE_MODEL_HH2;   // (the rate terms of the r gate, and NN-d's of the a gate, are the HH 2-state model's)
  using CK = CkptRecord<D>;
  constexpr int RECW = CK::WIDTH;
  const GArgs &a = ta.g;

  const int lane = threadIdx.x & 63;
  const int j = lane & (GROUP - 1);
  const int base = lane & ~(GROUP - 1);   // first lane of my group
  const int traj_raw = blockIdx.x * TPW + lane / GROUP;
  const bool valid = traj_raw < a.k.B;
  const int traj = valid ? traj_raw : a.k.B - 1;
  const int q = j >> 1;                   // my rate; my parameter is its amplitude (even) or its exponent (odd)
  const bool expo = (j & 1) != 0;
  const int Nt = a.k.Nt;

  double p[NPAR];
#pragma unroll
  for (int i = 0; i < NPAR; ++i) p[i] = a.k.params[(size_t)traj * a.k.n_params + i];
  const int pidx = a.k.prot_of_traj ? a.k.prot_of_traj[traj] : (traj % a.k.P);
  const double *__restrict__ pv = a.k.prot_v + (size_t)pidx * a.k.Np;
  const double *__restrict__ refb = a.sse_ref ? a.sse_ref + (size_t)pidx * Nt : nullptr;
  const double *__restrict__ vtb = a.v_tab ? a.v_tab + (size_t)pidx * Nt : nullptr;
  int nst = valid ? a.nacc[traj] : 0;
  nst = nst < 0 ? 0 : (nst > a.ckpt_cap ? a.ckpt_cap : nst);   // never past the records
  if (nst > a.n_iter - 1) nst = a.n_iter - 1;                  // ... nor past the packets (n_iter = max n_accepted + 1)
  const double *__restrict__ ck = a.ckpt + (size_t)traj * a.ckpt_cap * RECW;
  const bool sums = refb != nullptr && (ta.jtr != nullptr || ta.jtj != nullptr);   // wave-uniform
  double *__restrict__ tr_out = ta.di_dp ? ta.di_dp + (size_t)traj * Nt * NPAR + j : nullptr;
  const int n_chunk = a.it_end - a.it_begin;
  // my trajectory's packet of the chunk's first iteration (ionode_grad_recompute_kernel's address)
  const double *__restrict__ pk0 = a.packets + ((size_t)(traj >> 4) * n_chunk * 16 + (traj & 15)) * GRAD_PACKET;
  double *__restrict__ st = a.state + ((size_t)traj * GROUP + j) * TANGENT_NN_LANE_STATE;
  const bool first = a.it_end >= a.n_iter;   // the sweep's first launch: nothing carried yet

  // sample 0 is y0: zero sensitivity; a trajectory without steps (failed, empty) has zero rows throughout
  if (first && tr_out && valid) {
    const int rows = nst == 0 ? Nt : 1;
    for (int idx = 0; idx < rows; ++idx) tr_out[(size_t)idx * NPAR] = 0.0;
  }

  double Sd[D], Kc[D];   // S column j at the step's start; Kd_7 of the previous step (FSAL)
  double jtr_acc, jtj_acc[NPAR];
#pragma unroll
  for (int d = 0; d < D; ++d) { Sd[d] = first ? 0.0 : st[d]; Kc[d] = first ? 0.0 : st[D + d]; }
  jtr_acc = first ? 0.0 : st[2 * D];
#pragma unroll
  for (int l = 0; l < NPAR; ++l) jtj_acc[l] = first ? 0.0 : st[2 * D + 1 + l];

  // One stage's packet slot: the rates, and Kd = A(V) Yd + (df/dp_j)(Y, V) for my parameter
  auto stage_deriv = [&](const double *__restrict__ q8, const double (&Yd)[D], double (&Kd)[D]) {
    const double v = q8[pkt::V];
    const double Yi[D] = {q8[pkt::Y0], q8[pkt::Y1]};
    const double E[NR] = {NND ? q8[pkt::E1] : 0.0, NND ? q8[pkt::E2] : 0.0, q8[pkt::E3], q8[pkt::E4]};
    const double kk[NR] = {p[0] * E[0], p[2] * E[1], p[4] * E[2], p[6] * E[3]};
    const double cn = (double)q8[pkt::C] / 1000.0;
    double g[D];
    tangent_drate<HH>(q, Yi, g);
    const double kq = tangent_pick(kk, q);
    double c = expo ? ((q & 1) ? -v : v) * kq : tangent_pick(E, q);
    if (!NND && q < 2) c = 0.0;   // NN-f has no p1..p4
    const double fa = NND ? (cn - (kk[0] + kk[1])) * Yd[0] : cn * Yd[0];
    const double fr = -(kk[2] + kk[3]) * Yd[1];
    Kd[0] = fa + c * g[0];
    Kd[1] = fr + c * g[1];
  };

  for (int it = a.it_end - 1; it >= a.it_begin; --it) {
    const int s = nst - 1 - it;
    if (nst == 0 || s < -1) continue;   // failed, or not started yet (uniform over a group: the cross-lane reads below stay inside it)
    const double *__restrict__ pk = pk0 + (size_t)(it - a.it_begin) * (16 * GRAD_PACKET);
    if (s < 0) {   // the evaluation at (t_eval[0], y0): Kd_1 of the first step; S = 0 there
      const double zero[D] = {0.0, 0.0};
      stage_deriv(pk + pkt::STAGE, zero, Kc);
      continue;
    }
    const double *__restrict__ rec = ck + (size_t)s * RECW;
    const double t0 = rec[CK::T0], dt = rec[CK::DT];
    int oi = (int)rec[CK::OI], nout = (int)rec[CK::NOUT];
    const double t1 = t0 + dt;
    const double dts = (double)(S)dt;

    double Kd[7][D];
#pragma unroll
    for (int d = 0; d < D; ++d) Kd[0][d] = Kc[d];
    double Yd[D];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
#pragma unroll
      for (int d = 0; d < D; ++d) {
        double tacc = 0.0;
#pragma unroll
        for (int jx = 0; jx <= i; ++jx) tacc += Kd[jx][d] * (kBeta[i][jx] * dts);
        Yd[d] = Sd[d] + tacc;
      }
      stage_deriv(pk + pkt::STAGE + pkt::STAGE_W * (5 - i), Yd, Kd[i + 1]);
    }
    // Yd is now the tangent of y1

    if (oi < 1 || oi >= Nt) nout = 0;
    if (nout > Nt - oi) nout = Nt - oi;
    if (nout > 0) {
      // the step's interpolant as the forward fitted it (state dtype), and its tangent: the same formulas in fp64
      double y[D], k[7][D];
#pragma unroll
      for (int d = 0; d < D; ++d) y[d] = rec[CK::Y + d];
#pragma unroll
      for (int jx = 0; jx < 7; ++jx)
#pragma unroll
        for (int d = 0; d < D; ++d) k[jx][d] = rec[CK::K + jx * D + d];
      S cf[5][D];
      sse_fit_step<S, D>(dt, y, k, (s + 1 < nst) ? rec + RECW + CK::Y : nullptr, cf);
      double tcf[5][D];
      interp_fit_all<double, D>(dts, Sd, Yd, Kd, tcf);
      const double den = t1 - t0, rden = 1.0 / den;   // the forward's reciprocal and div_pos: the same x bits
      for (int n = 0; n < nout; ++n) {
        const int idx = oi + n;
        const double tk = a.k.t_eval[idx];
        double vk;
        if (vtb) vk = vtb[idx];
        else protocol_v(a.k, pv, tk, vk);
        double ik;
        const double sj = tangent_sample<S, D>(a, cf, tcf, interp_x<S>(tk, t0, den, rden), vk, ik);
        if (tr_out) tr_out[(size_t)idx * NPAR] = sj;
        if (sums) {
          jtr_acc += sj * (ik - refb[idx]);
#pragma unroll
          for (int l = 0; l < NPAR; ++l) jtj_acc[l] += sj * __shfl(sj, base + l);
        }
      }
    }
#pragma unroll
    for (int d = 0; d < D; ++d) { Sd[d] = Yd[d]; Kc[d] = Kd[6][d]; }
  }

  if (valid) {
#pragma unroll
    for (int d = 0; d < D; ++d) { st[d] = Sd[d]; st[D + d] = Kc[d]; }
    st[2 * D] = jtr_acc;
#pragma unroll
    for (int l = 0; l < NPAR; ++l) st[2 * D + 1 + l] = jtj_acc[l];
    if (a.it_begin == 0) {
      if (ta.jtr) ta.jtr[(size_t)traj * NPAR + j] = jtr_acc;
      if (ta.jtj) {
#pragma unroll
        for (int l = 0; l < NPAR; ++l) ta.jtj[((size_t)traj * NPAR + j) * NPAR + l] = jtj_acc[l];
      }
    }
  }
}

}  // namespace ionode
