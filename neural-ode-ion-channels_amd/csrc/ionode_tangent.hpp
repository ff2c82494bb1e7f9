// ionode_tangent.hpp -- gfx950 device code of the TANGENT (forward-mode) sweep through a dopri5 solve of the closed-form models:
// the per-sample sensitivities dI(t_k)/dp_j of the current trace (PINTS ForwardModelS1.simulateS1), and their Gauss-Newton sums
// J^T r and J^T J against the fused objective's reference currents.
//
// What is differentiated: the discretisation the forward launch executed, as in ionode_grad.hpp -- the accepted steps (t0, dt) are
// constants, rejected attempts contribute nothing, FSAL and the 4th-order dense output are differentiated as written.  S = dy/dp is
// D x NPAR, zero at y0; both models are linear in y, f = A(V; p) y + b(V; p), so per parameter column j and stage i
//     Yd_i   = S + dts sum_m beta_im Kd_m
//     Kd_i+1 = A(V_i) Yd_i + (dA/dp_j) Y_i + db/dp_j
// with Y_i rebuilt from the step's checkpoint exactly as the backward sweep rebuilds it, Kd_1 the previous step's Kd_7 (first step:
// df/dp_j at (t_eval[0], y0)) and S <- Yd_6.  A rate is k = p_2q E, E = exp(+-p_2q+1 V): dk/dp_2q = E, dk/dp_2q+1 = +-V k -- no
// division by a parameter; where the fp32-state forward evaluates the rates in fp32 (stage time outside the protocol) the same
// formula is differentiated.  The tangent of the dense output is interp_fit / interp_eval (ionode_interp.hpp) in fp64 on
// (S, S_next, Kd_1, Kd_7) at the forward's x_k; y_k itself is re-evaluated from the checkpoint in the state dtype, as the fused
// backward sweep does.  Tangents are fp64 whatever the state dtype.  Checker: tests/tangent_check.py.
//
// Execution model.  The columns of S are independent: one lane per (trajectory, parameter).  A trajectory owns a group of GROUP
// consecutive lanes (2-state: 8 lanes, 8 trajectories per wavefront; 6-state: a 16-lane row with 12 lanes live, 4 per wavefront), a
// workgroup is one wavefront, and the wavefront walks the steps 0 .. max n_accepted of its trajectories with the finished ones
// predicated off.  The lanes of a group read the same checkpoint record (one broadcast load each) and compute the per-trajectory
// values -- rates, stage inputs, y_k -- redundantly; nothing is shared through LDS.  Per output sample a lane forms s_j = di_k/dp_j
// (tangent_sample: the ONE routine behind the trace and the sums) and either stores it, or adds s_j r_k to J^T r and s_j s_l, l = 0 ..
// NPAR - 1, to row j of J^T J, the s_l fetched from the group's other lanes in registers (__shfl: ds_bpermute, no LDS storage).  No
// atomics; one summation order per trajectory (sample order), whatever the batch around it.
#pragma once

#include "ionode_grad.hpp"   // GArgs, CkptRecord, sse_fit_step; the interpolant and the observation model (ionode_interp.hpp)

namespace ionode {

struct TArgs {
  GArgs g;          // k (protocol lookup, params, prot_v, prot_of_traj, t_eval, B, Nt, P), ckpt, ckpt_cap, nacc, sse_ref, v_tab, obs_*
  double *di_dp;    // [B][Nt][NPAR] or NULL
  double *jtr;      // [B][NPAR] or NULL      (with sse_ref)
  double *jtj;      // [B][NPAR][NPAR] or NULL (with sse_ref)
};

template <int MODEL> struct TangentMap {
  static constexpr int GROUP = (MODEL == IONODE_MODEL_MARKOV6) ? 16 : 8;   // lanes per trajectory
  static constexpr int TPW = 64 / GROUP;                                   // trajectories per wavefront (= per workgroup)
};

// inst_tangent.hip: model IONODE_MODEL_HH2 | IONODE_MODEL_MARKOV6
void launch_tangent(int model, int f32, const TArgs &a, hipStream_t s);

// x[q] for a per-lane q in 0 .. N - 1.  Pure mask arithmetic on the bit patterns: an indexed array lives in scratch, and a chain of
// selects over its elements is folded by hipcc into one load with a selected address, which pins the array there just the same
// (ionode_grad.hpp Signs); and/or on values cannot be.
template <int N> __device__ __forceinline__ double tangent_pick(const double (&x)[N], int q) {
  unsigned long long r = 0ull;
#pragma unroll
  for (int i = 0; i < N; ++i) r |= (unsigned long long)__double_as_longlong(x[i]) & ((q == i) ? ~0ull : 0ull);
  return __longlong_as_double((long long)r);
}

// The rates of one stage voltage with their exponentials: k[q] = p[2q] E[q], E[q] = exp(+-p[2q+1] v), the forms of closed_rates
// (ionode_rhs.hpp) -- fp64, or (fp32 state, stage time outside the protocol) fp32 at (float)v_oob.  vs: the voltage the
// exponent's derivative multiplies, dk/dp[2q+1] = +-vs k.
template <int MODEL, typename S>
__device__ __forceinline__ void tangent_rates(const KArgs &a, const double *p, double v, bool inrange, double (&E)[ModelTraits<MODEL>::NPAR / 2],
                                              double (&k)[ModelTraits<MODEL>::NPAR / 2], double &vs) {
  constexpr int NR = ModelTraits<MODEL>::NPAR / 2;
  if ((sizeof(S) == 4) && !inrange) {
    const float vf = (float)a.v_oob;
#pragma unroll
    for (int i = 0; i < NR; ++i) {
      const float ef = det_expf((float)((i & 1) ? -p[2 * i + 1] : p[2 * i + 1]) * vf);
      E[i] = (double)ef;
      k[i] = (double)((float)p[2 * i] * ef);
    }
    vs = (double)vf;
  } else {
#pragma unroll
    for (int i = 0; i < NR; ++i) {
      E[i] = det_exp_ldexp(((i & 1) ? -p[2 * i + 1] : p[2 * i + 1]) * v);
      k[i] = p[2 * i] * E[i];
    }
    vs = v;
  }
}

// A(rates) x, fp64: closed_rhs's expressions without its additive term
template <int MODEL>
__device__ __forceinline__ void tangent_apply(const double (&r)[ModelTraits<MODEL>::NPAR / 2], const double (&x)[ModelTraits<MODEL>::D],
                                              double (&f)[ModelTraits<MODEL>::D]) {
  if constexpr (MODEL == IONODE_MODEL_MARKOV6) {
    const double a1 = r[0], b1 = r[1], bh = r[2], ah = r[3], a2 = r[4], b2 = r[5];
    const double c1 = x[0], c2 = x[1], i_ = x[2], ic1 = x[3], ic2 = x[4], o = x[5];
    f[0] = a1 * c2 + ah * ic1 + b2 * o - (b1 + bh + a2) * c1;
    f[1] = b1 * c1 + ah * ic2 - (a1 + bh) * c2;
    f[2] = a2 * ic1 + bh * o - (b2 + ah) * i_;
    f[3] = a1 * ic2 + bh * c1 + b2 * i_ - (b1 + ah + a2) * ic1;
    f[4] = b1 * ic1 + bh * c2 - (ah + a1) * ic2;
    f[5] = a2 * c1 + ah * i_ - (b2 + bh) * o;
  } else {
    f[0] = -(r[0] + r[1]) * x[0];   // da/dt = k1 (1 - a) - k2 a
    f[1] = -(r[2] + r[3]) * x[1];   // dr/dt = -k3 r + k4 (1 - r)
  }
}

// df/d(rate q) at the stage input Y (fp64), for the lane's own rate q
template <int MODEL>
__device__ __forceinline__ void tangent_drate(int q, const double (&Y)[ModelTraits<MODEL>::D], double (&g)[ModelTraits<MODEL>::D]) {
  if constexpr (MODEL == IONODE_MODEL_MARKOV6) {
    const double c1 = Y[0], c2 = Y[1], in = Y[2], ic1 = Y[3], ic2 = Y[4], o = Y[5];
    //               a1     b1     bh    ah     a2     b2
    const double g0[6] = {c2, -c1, -c1, ic1, -c1, o};
    const double g1[6] = {-c2, c1, -c2, ic2, 0.0, 0.0};
    const double g2[6] = {0.0, 0.0, o, -in, ic1, -in};
    const double g3[6] = {ic2, -ic1, c1, -ic1, -ic1, in};
    const double g4[6] = {-ic2, ic1, c2, -ic2, 0.0, 0.0};
    const double g5[6] = {0.0, 0.0, -o, in, c1, -o};
    g[0] = tangent_pick(g0, q); g[1] = tangent_pick(g1, q); g[2] = tangent_pick(g2, q);
    g[3] = tangent_pick(g3, q); g[4] = tangent_pick(g4, q); g[5] = tangent_pick(g5, q);
  } else {
    const double av = Y[0], rv = Y[1];
    const double g0[4] = {1.0 - av, -av, 0.0, 0.0};
    const double g1[4] = {0.0, 0.0, -rv, 1.0 - rv};
    g[0] = tangent_pick(g0, q); g[1] = tangent_pick(g1, q);
  }
}

// One output sample: y_k from the step's interpolant at x (state dtype: the forward's bits), its tangent from the tangent
// coefficients at the same x (fp64), the current i_k (obs_current) and s_j = di_k/dp_j = g (V - E) (ad r + a rd), or g (V - E) Od.
// The ONE routine behind the trace and the fused sums: they differ by summation order only.
template <typename S, int D>
__device__ __forceinline__ double tangent_sample(const GArgs &a, const S (&cf)[5][D], const double (&tcf)[5][D], S xs, double v, double &ik) {
  S out[D];
  interp_eval<S, D>(cf, xs, out);
  double yd[D];
  interp_eval<double, D>(tcf, (double)xs, yd);
  ik = obs_current<S, D>(a, out, v);
  const double gdv = a.obs_g * (v - a.obs_e);
  if (a.obs_open) return gdv * yd[D - 1];
  return gdv * (yd[0] * (double)out[1] + (double)out[0] * yd[1]);
}

template <int MODEL, typename S>
__global__ void __launch_bounds__(64) ionode_tangent_sweep_kernel(const TArgs ta) {
  constexpr int D = ModelTraits<MODEL>::D, NPAR = ModelTraits<MODEL>::NPAR, NR = NPAR / 2;
  constexpr int GROUP = TangentMap<MODEL>::GROUP, TPW = TangentMap<MODEL>::TPW;
  static_assert(!ModelTraits<MODEL>::MLP && NPAR <= GROUP, "closed-form models, one lane per parameter");
  using R = Real<S>;
  using CK = CkptRecord<D>;
  constexpr int RECW = CK::WIDTH;
  const GArgs &a = ta.g;

  const int lane = threadIdx.x & 63;
  const int j = lane & (GROUP - 1);
  const int base = lane & ~(GROUP - 1);   // first lane of my group
  const int traj_raw = blockIdx.x * TPW + lane / GROUP;
  const bool valid = traj_raw < a.k.B;
  const int traj = valid ? traj_raw : a.k.B - 1;
  const bool live = valid && j < NPAR;     // (6-state: lanes 12..15 of a row repeat parameter 11 and store nothing)
  const int jp = j < NPAR ? j : NPAR - 1;
  const int q = jp >> 1;                   // my rate; my parameter is its amplitude (even) or its exponent (odd)
  const bool expo = (jp & 1) != 0;
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
  const double *__restrict__ ck = a.ckpt + (size_t)traj * a.ckpt_cap * RECW;
  const bool sums = refb != nullptr && (ta.jtr != nullptr || ta.jtj != nullptr);   // wave-uniform
  double *__restrict__ tr_out = ta.di_dp ? ta.di_dp + (size_t)traj * Nt * NPAR + jp : nullptr;

  // sample 0 is y0: zero sensitivity; a trajectory without steps (failed, empty) has zero rows throughout
  if (tr_out && live) {
    const int rows = nst == 0 ? Nt : 1;
    for (int idx = 0; idx < rows; ++idx) tr_out[(size_t)idx * NPAR] = 0.0;
  }

  // the rate-derivative coefficient of my parameter at a stage: dk_q/dp_j
  auto coef = [&](const double (&E)[NR], const double (&kk)[NR], double vs) {
    const double kq = tangent_pick(kk, q);
    return expo ? ((q & 1) ? -vs : vs) * kq : tangent_pick(E, q);
  };

  double Sd[D], Kc[D];   // S column j at the step's start; Kd_7 of the previous step (FSAL)
#pragma unroll
  for (int d = 0; d < D; ++d) { Sd[d] = 0.0; Kc[d] = 0.0; }
  double jtr_acc = 0.0, jtj_acc[NPAR];
#pragma unroll
  for (int l = 0; l < NPAR; ++l) jtj_acc[l] = 0.0;

  for (int s = 0; __ballot(s < nst) != 0ull; ++s) {
    if (s < nst) {   // (uniform over a group: the cross-lane reads below stay inside it)
      const double *__restrict__ rec = ck + (size_t)s * RECW;
      const double t0 = rec[CK::T0], dt = rec[CK::DT];
      int oi = (int)rec[CK::OI], nout = (int)rec[CK::NOUT];
      double y[D], k[7][D];
#pragma unroll
      for (int d = 0; d < D; ++d) y[d] = rec[CK::Y + d];
#pragma unroll
      for (int jx = 0; jx < 7; ++jx)
#pragma unroll
        for (int d = 0; d < D; ++d) k[jx][d] = rec[CK::K + jx * D + d];
      const double t1 = t0 + dt;
      const S t0s = (S)t0, dts_s = (S)dt, t1s = (S)t1;
      const double dts = (double)dts_s;

      double Kd[7][D];
      double E[NR], kk[NR], vs = 0.0;
      if (s == 0) {   // Kd_1 of the first step: df/dp_j at (t_eval[0], y0); S = 0 there
        double v;
        const bool inr = protocol_v(a.k, pv, (double)(S)a.k.t_eval[0], v);
        tangent_rates<MODEL, S>(a.k, p, v, inr, E, kk, vs);
        double g[D];
        tangent_drate<MODEL>(q, y, g);
        const double c = coef(E, kk, vs);
#pragma unroll
        for (int d = 0; d < D; ++d) Kd[0][d] = c * g[d];
      } else {
#pragma unroll
        for (int d = 0; d < D; ++d) Kd[0][d] = Kc[d];
      }
      double Yd[D];
#pragma unroll
      for (int i = 0; i < 6; ++i) {
        double Yi[D];
#pragma unroll
        for (int d = 0; d < D; ++d) {
          double sacc = 0.0, tacc = 0.0;
#pragma unroll
          for (int jx = 0; jx <= i; ++jx) {
            sacc += k[jx][d] * (kBeta[i][jx] * dts);
            tacc += Kd[jx][d] * (kBeta[i][jx] * dts);
          }
          Yi[d] = y[d] + sacc;
          Yd[d] = Sd[d] + tacc;
        }
        if (i < 5) {   // (the last two stages share their time)
          const S ti = (i >= 4) ? R::prev_(t1s) : t0s + (S)kAlpha[i] * dts_s;
          double v;
          const bool inr = protocol_v(a.k, pv, (double)ti, v);
          tangent_rates<MODEL, S>(a.k, p, v, inr, E, kk, vs);
        }
        double g[D], f[D];
        tangent_drate<MODEL>(q, Yi, g);
        tangent_apply<MODEL>(kk, Yd, f);
        const double c = coef(E, kk, vs);
#pragma unroll
        for (int d = 0; d < D; ++d) Kd[i + 1][d] = f[d] + c * g[d];
      }
      // Yd is now the tangent of y1

      if (oi < 1 || oi >= Nt) nout = 0;
      if (nout > Nt - oi) nout = Nt - oi;
      if (nout > 0) {
        // the step's interpolant as the forward fitted it (state dtype), and its tangent: the same formulas in fp64
        S cf[5][D];
        sse_fit_step<S, D>(dt, y, k, (s + 1 < nst) ? ck + (size_t)(s + 1) * RECW + CK::Y : nullptr, cf);
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
          if (tr_out && live) tr_out[(size_t)idx * NPAR] = sj;
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
  }

  if (live) {
    if (ta.jtr) ta.jtr[(size_t)traj * NPAR + j] = jtr_acc;
    if (ta.jtj) {
#pragma unroll
      for (int l = 0; l < NPAR; ++l) ta.jtj[((size_t)traj * NPAR + j) * NPAR + l] = jtj_acc[l];
    }
  }
}

}  // namespace ionode
