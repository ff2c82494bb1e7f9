// ionode_mala.hpp -- one manifold-MALA iteration (tell, then propose) for many independent chains (include/ionode.h "Manifold MALA
// step"): the per-chain routine ma_chain(), shared WORD FOR WORD by the gfx950 kernel (inst_mala.hip) and the host mirror
// (ionode_mala_step_host).
//
// The "simplified manifold MALA" of Girolami and Calderhead ("Riemann manifold Langevin and Hamiltonian Monte Carlo methods", J. R.
// Statist. Soc. B 73, 2011): a Metropolis-adjusted Langevin step preconditioned by the expected Fisher information, which under the
// Gaussian noise model is the Gauss-Newton matrix J^T J / sigma^2 the tangent sweep already sums.  A chain has n = nf + sample_sigma
// coordinates u: the nf free rate parameters (log x or x) and, when the noise level is sampled, log sigma as the last.  One call, for
// a running chain at iteration t (iters[chain][0] on entry), on the Gauss-Newton evaluation of the point the previous call wrote:
//   reduce   S = sum_p sse, p = 0 .. P - 1 in that order; a non-zero status or a NaN makes S = +inf
//   target   lp_t = -N u_sigma - (S / 2) exp(-2 u_sigma) at the evaluated point (-inf for S = +inf)
//   metric   g_x = sum_p jtr, H_x = sum_p jtj over the free rows and columns (lower triangle); log parameters: g_j x_j, H_jl (x_j x_l);
//            grad_j = -g_j / sigma^2, G_jl = H_jl / sigma^2; sampled sigma: grad_s = -N + S / sigma^2, G_ss = 2 N, no cross terms;
//            G_jj += ridge max(G_jj, 2^-20 max_l G_ll, 2^-256); G = L_t L_t^T packed by rows, ld_t = sum_j log L_jj
//   t = 0    the evaluation is the start's: (lp, grad, L, ld) <- its; NONFINITE, DEGENERATE
//   tell     alpha = 0 for a proposal that was outside the box, a non-finite lp_t or a metric that does not factor; else with
//            y = L_t^-1 grad_t, d = L_t^-T y, mu_t = ut + (eps^2 / 2) d, v = L_t^T (u - mu_t):
//            lq_r = ld_t - n log_eps - (v . v) / (2 eps^2), ratio = ((lp_t + lq_r) - lp) - lq_f, alpha = exp(min(ratio, 0));
//            accepted iff alpha > 0 and log w < ratio, w the first uniform of (chain_base + chain, t, 1, 0)
//   adapt    log_eps <- log_eps + exp(-eta log(t + 1)) (alpha - target_accept): the only thing adapted
//   record   t % thin == 0 and t / thin < sample_cap: samples[chain][t / thin] <- (x, lp)
//   stop     kMala* flags: the start not evaluable, its metric not positive definite, the iteration cap
//   propose  z the deviates of (chain_base + chain, t + 1, 0, pair), eps = exp(log_eps); y = L^-1 grad, w = (eps^2 / 2) y + eps z,
//            ut = u + L^-T w; lq_f = ld - n log_eps - (z . z) / 2; outside the box the slot's rows repeat the current x
//
// Bit-for-bit agreement of the two builds is a property of this file, as it is for ionode_mcmc.hpp: the units are compiled with
// -ffp-contract=off -fno-fast-math (host and device pass), fp64 + - * / and sqrt are correctly rounded on both, every sum has ONE
// written order, the only transcendentals are lm_exp and cm_log, and the generator is ionode_step_math.hpp's, unchanged.  A failed
// factorisation is never stored (a NaN's sign is not the same everywhere).
//
// Execution model: ionode_mcmc.hpp's.  One lane per chain, N (the number of coordinates) a template argument -- every loop unrolls
// with constant indices.  ONE packed triangle (91 words at N = 13) is live at a time: the trial's factor L_t through the tell; then
// each of its words either stays (accepted, and is written to the state) or is replaced BY VALUE with the stored factor's word for
// the proposal.  u, ut, x, xt and the stored gradient are read from and written to the state element by element.  Nothing is in
// scratch or LDS, there are no cross-lane operations and no atomics: a chain's result cannot depend on what shares its wavefront.
#pragma once

#include "ionode_step_math.hpp"

namespace ionode {

constexpr int kMaMaxDim = IONODE_MCMC_MAX_DIM;

// The descriptor's settings as the routine wants them: by value (kernel arguments on the device).  Coordinate j < nf is free parameter j;
// with ss the coordinate nf is log sigma: its box and its parameter bounds sit at index nf of the four bound arrays.
struct MaArgs {
  int32_t K, n_active, P, NPAR, nf, n, log_p, ss, max_iter, thin, sample_cap, chain_base;
  uint32_t seed_lo, seed_hi;
  int32_t free_idx[kLmMaxFree];
  double base[kLmMaxFree];
  double ulo[kMaMaxDim], uhi[kMaMaxDim];   // the box in the search space
  double xlo[kMaMaxDim], xhi[kMaMaxDim];   // ... and in the parameters
  double n_samples, log_sigma, eta, target_accept, ridge;   // log_sigma: of the fixed sigma (without ss)
  const int32_t *active;   // [n_active] or NULL (slot s is chain s)
  const double *sse;       // [n_active * P]
  const double *jtr;       // [n_active * P][NPAR]
  const double *jtj;       // [n_active * P][NPAR][NPAR]
  const int32_t *status;   // [n_active * P]
  double *state;           // [K][ma_state_doubles(n)]
  int32_t *flag;           // [K]
  int32_t *iters;          // [K][2]: tells, accepted
  double *trial;           // [n_active * P][NPAR]
  double *samples;         // [K][sample_cap][n + 1] or NULL
};

// state layout of one chain (IONODE_MALA_STATE_* in the header): 6 scalars, u, ut, x, xt, grad [n], L [n][n]
__host__ __device__ constexpr int ma_state_doubles(int n) { return IONODE_MALA_STATE_U + 5 * n + n * n; }
__host__ __device__ constexpr int ma_off_u(int) { return IONODE_MALA_STATE_U; }
__host__ __device__ constexpr int ma_off_ut(int n) { return IONODE_MALA_STATE_U + n; }
__host__ __device__ constexpr int ma_off_x(int n) { return IONODE_MALA_STATE_U + 2 * n; }
__host__ __device__ constexpr int ma_off_xt(int n) { return IONODE_MALA_STATE_U + 3 * n; }
__host__ __device__ constexpr int ma_off_grad(int n) { return IONODE_MALA_STATE_U + 4 * n; }
__host__ __device__ constexpr int ma_off_l(int n) { return IONODE_MALA_STATE_U + 5 * n; }

// the chain's P rows of the trial tensor: the base parameters with the free columns replaced by xs[0 .. nf) (sigma never enters them)
template <int N>
__host__ __device__ inline void ma_write_trial(const MaArgs &a, int slot, const double *xs) {
  for (int p = 0; p < a.P; ++p) {
    double *row = a.trial + ((size_t)slot * a.P + p) * a.NPAR;
#pragma unroll
    for (int i = 0; i < kLmMaxFree; ++i)   // (constant indices into the by-value arguments)
      if (i < a.NPAR) row[i] = a.base[i];
#pragma unroll
    for (int j = 0; j < (N < kLmMaxFree ? N : kLmMaxFree); ++j)
      if (j < a.nf) row[a.free_idx[j]] = xs[j];
  }
}

// One iteration of the chain in launch slot `slot`.
template <int N>
__host__ __device__ inline void ma_chain(const MaArgs &a, int slot) {
  constexpr int NFM = N < kLmMaxFree ? N : kLmMaxFree;   // the most free parameters N coordinates can hold
  const int c = a.active ? a.active[slot] : slot;
  if (c < 0 || c >= a.K) return;   // (an index list that names no chain: nothing of it is touched)
  double *st = a.state + (size_t)c * ma_state_doubles(N);
  double *su = st + ma_off_u(N), *sut = st + ma_off_ut(N), *sx = st + ma_off_x(N), *sxt = st + ma_off_xt(N), *sg = st + ma_off_grad(N),
         *sL = st + ma_off_l(N);

  if (a.flag[c] != IONODE_MALA_RUNNING) {   // frozen: the slot keeps evaluating the current point until the next compaction
    double xs[N];
#pragma unroll
    for (int j = 0; j < N; ++j) xs[j] = sx[j];
    ma_write_trial<N>(a, slot, xs);
    return;
  }

  // ---- reduce: the evaluated point's sum of squares ----
  double S = 0.0;
  bool failed = false;
  for (int p = 0; p < a.P; ++p) {
    S = S + a.sse[(size_t)slot * a.P + p];
    failed = failed || a.status[(size_t)slot * a.P + p] != 0;
  }
  if (failed || !(S < lm_inf())) S = lm_inf();   // (a NaN counts as a failure)

  const int t = a.iters[2 * c];
  const bool outside = st[IONODE_MALA_STATE_OUTSIDE] != 0.0;
  double lp = st[IONODE_MALA_STATE_LP], log_eps = st[IONODE_MALA_STATE_LOG_EPS], ld = st[IONODE_MALA_STATE_LD];
  const double lqf = st[IONODE_MALA_STATE_LQF];
  int flag = IONODE_MALA_RUNNING;

  // ---- target: the log-posterior of what was evaluated (the start at t = 0, else the proposal) ----
  const double ls_u = su[N - 1], ls_ut = sut[N - 1];   // (both loaded, then chosen by value: a choice of addresses would put log_sigma in scratch)
  double ls = a.log_sigma;
  if (a.ss) ls = t == 0 ? ls_u : ls_ut;
  const double inv_s2 = lm_exp(-2.0 * ls);
  const double lp_t = S < lm_inf() ? -a.n_samples * ls - (0.5 * S) * inv_s2 : -lm_inf();

  // ---- metric: gradient and expected information at the evaluated point, the information's lower triangle packed by rows ----
  double A[N * (N + 1) / 2], gt[N];
  bool ok = lm_finite(inv_s2);
  {
    double xe[N];
#pragma unroll
    for (int j = 0; j < N; ++j) {
      const double x_u = sx[j], x_ut = sxt[j];
      xe[j] = t == 0 ? x_u : x_ut;
    }
#pragma unroll
    for (int j = 0; j < N; ++j) {
      const bool sig = a.ss && j == N - 1;
      if (sig) {
        gt[j] = -a.n_samples + S * inv_s2;
#pragma unroll
        for (int l = 0; l < j; ++l) A[j * (j + 1) / 2 + l] = 0.0;
        A[j * (j + 1) / 2 + j] = 2.0 * a.n_samples;
      } else {
        const int fj = a.free_idx[j < NFM ? j : 0];
        double s = 0.0;
        for (int p = 0; p < a.P; ++p) s = s + a.jtr[((size_t)slot * a.P + p) * a.NPAR + fj];
        if (a.log_p) s = s * xe[j];
        gt[j] = -s * inv_s2;
#pragma unroll
        for (int l = 0; l <= j; ++l) {
          const int fl = a.free_idx[l < NFM ? l : 0];
          double h = 0.0;
          for (int p = 0; p < a.P; ++p) h = h + a.jtj[(((size_t)slot * a.P + p) * a.NPAR + fj) * a.NPAR + fl];
          if (a.log_p) h = h * (xe[j] * xe[l]);
          A[j * (j + 1) / 2 + l] = h * inv_s2;
        }
      }
      ok = ok && lm_finite(gt[j]);
    }
  }
  double ld_t = 0.0;
  {
    double dmax = 0.0;
#pragma unroll
    for (int j = 0; j < N; ++j) dmax = A[j * (j + 1) / 2 + j] > dmax ? A[j * (j + 1) / 2 + j] : dmax;
    const double floor_ = IONODE_LM_FLOOR_REL * dmax > IONODE_LM_FLOOR_ABS ? IONODE_LM_FLOOR_REL * dmax : IONODE_LM_FLOOR_ABS;
#pragma unroll
    for (int j = 0; j < N; ++j) {
      const double gjj = A[j * (j + 1) / 2 + j];
      A[j * (j + 1) / 2 + j] = gjj + a.ridge * (gjj > floor_ ? gjj : floor_);   // (a NaN stays one and fails the pivot)
    }
#pragma unroll
    for (int j = 0; j < N; ++j) {
#pragma unroll
      for (int l = 0; l < j; ++l) {   // L_jl = (A_jl - sum_{m < l} L_jm L_lm) / L_ll
        double s = A[j * (j + 1) / 2 + l];
#pragma unroll
        for (int m = 0; m < l; ++m) s = s - A[j * (j + 1) / 2 + m] * A[l * (l + 1) / 2 + m];
        A[j * (j + 1) / 2 + l] = s / A[l * (l + 1) / 2 + l];
      }
      double piv = A[j * (j + 1) / 2 + j];
#pragma unroll
      for (int m = 0; m < j; ++m) piv = piv - A[j * (j + 1) / 2 + m] * A[j * (j + 1) / 2 + m];
      ok = ok && piv > 0.0 && lm_finite(piv);
      const double ljj = __builtin_sqrt(piv);   // (a failed pivot poisons what follows; `ok` discards it)
      A[j * (j + 1) / 2 + j] = ljj;
      ld_t = ld_t + cm_log(ljj);
    }
    ok = ok && lm_finite(ld_t);
  }

  bool take = false;   // the evaluated point becomes the chain's
  if (t == 0) {
    bool inside = true;
#pragma unroll
    for (int j = 0; j < N; ++j) {
      const double uj = su[j];
      inside = inside && uj >= a.ulo[j] && uj <= a.uhi[j];
    }
    lp = lp_t;
    if (!inside || !lm_finite(lp)) flag = IONODE_MALA_NONFINITE;
    else if (!ok) flag = IONODE_MALA_DEGENERATE;
    else take = true;
  } else {
    // ---- tell: the Metropolis-Hastings decision, with the step size the proposal was drawn with ----
    double alpha = 0.0, ratio = -lm_inf();
    if (!outside && lm_finite(lp_t) && ok) {
      const double eps = lm_exp(log_eps);
      const double h = 0.5 * (eps * eps);
      double y[N], d[N];
#pragma unroll
      for (int j = 0; j < N; ++j) {   // L_t y = grad_t
        double s = gt[j];
#pragma unroll
        for (int m = 0; m < j; ++m) s = s - A[j * (j + 1) / 2 + m] * y[m];
        y[j] = s / A[j * (j + 1) / 2 + j];
      }
#pragma unroll
      for (int j = N - 1; j >= 0; --j) {   // L_t^T d = y
        double s = y[j];
#pragma unroll
        for (int m = N - 1; m > j; --m) s = s - A[m * (m + 1) / 2 + j] * d[m];
        d[j] = s / A[j * (j + 1) / 2 + j];
      }
#pragma unroll
      for (int j = 0; j < N; ++j) d[j] = su[j] - (sut[j] + h * d[j]);   // u - mu_t
      double q = 0.0;
#pragma unroll
      for (int j = 0; j < N; ++j) {   // v = L_t^T (u - mu_t)
        double v = 0.0;
#pragma unroll
        for (int m = j; m < N; ++m) v = v + A[m * (m + 1) / 2 + j] * d[m];
        q = q + v * v;
      }
      const double lqr = (ld_t - (double)N * log_eps) - q / (2.0 * (eps * eps));
      ratio = ((lp_t + lqr) - lp) - lqf;
      if (ratio == ratio) alpha = lm_exp(ratio < 0.0 ? ratio : 0.0);
    }
    uint32_t w[4];
    cm_philox((uint32_t)(a.chain_base + c), (uint32_t)t, 1u, 0u, a.seed_lo, a.seed_hi, w);
    take = alpha > 0.0 && cm_log(cm_uniform(w[0], w[1])) < ratio;
    if (take) {
#pragma unroll
      for (int j = 0; j < N; ++j) {
        su[j] = sut[j];
        sx[j] = sxt[j];
      }
      lp = lp_t;
      a.iters[2 * c + 1] = a.iters[2 * c + 1] + 1;
    }
    st[IONODE_MALA_STATE_ALPHA] = alpha;
    // ---- adapt: the step size alone ----
    log_eps = log_eps + lm_exp(-a.eta * cm_log((double)(t + 1))) * (alpha - a.target_accept);
    if (t >= a.max_iter) flag = IONODE_MALA_MAXITER;
  }
  if (take) {   // (grad, L, ld) <- the evaluated point's
    ld = ld_t;
#pragma unroll
    for (int j = 0; j < N; ++j) {
      sg[j] = gt[j];
#pragma unroll
      for (int l = 0; l < N; ++l) sL[j * N + l] = l <= j ? A[j * (j + 1) / 2 + l] : 0.0;
    }
  }
  st[IONODE_MALA_STATE_LP] = lp;
  st[IONODE_MALA_STATE_LOG_EPS] = log_eps;
  st[IONODE_MALA_STATE_LD] = ld;

  // ---- record: in the parameters ----
  if (a.samples && t % a.thin == 0 && t / a.thin < a.sample_cap) {
    double *row = a.samples + ((size_t)c * a.sample_cap + (size_t)(t / a.thin)) * (N + 1);
#pragma unroll
    for (int j = 0; j < N; ++j) row[j] = sx[j];
    row[N] = lp;
  }

  a.flag[c] = flag;
  if (flag != IONODE_MALA_RUNNING) {   // stopped in this call: the rows repeat the current point, the counter stays at this tell
    double xs[N];
#pragma unroll
    for (int j = 0; j < N; ++j) xs[j] = sx[j];
    ma_write_trial<N>(a, slot, xs);
    return;
  }
  a.iters[2 * c] = t + 1;

  // ---- propose: the chain's own factor and gradient, word by word the trial's (taken) or the stored one ----
#pragma unroll
  for (int j = 0; j < N; ++j) {
    const double g_s = sg[j];
    gt[j] = take ? gt[j] : g_s;
#pragma unroll
    for (int l = 0; l <= j; ++l) {
      const double l_s = sL[j * N + l];
      A[j * (j + 1) / 2 + l] = take ? A[j * (j + 1) / 2 + l] : l_s;
    }
  }
  const double eps = lm_exp(log_eps);
  const double h = 0.5 * (eps * eps);
  double w[N], zz = 0.0;
#pragma unroll
  for (int jp = 0; jp < (N + 1) / 2; ++jp) {
    double z0, z1;
    cm_normal_pair(a.seed_lo, a.seed_hi, a.chain_base + c, t + 1, 0, jp, 0, z0, z1);
    w[2 * jp] = z0;
    zz = zz + z0 * z0;
    if (2 * jp + 1 < N) {
      w[2 * jp + 1] = z1;
      zz = zz + z1 * z1;
    }
  }
  st[IONODE_MALA_STATE_LQF] = (ld - (double)N * log_eps) - 0.5 * zz;
#pragma unroll
  for (int j = 0; j < N; ++j) {   // L y = grad; w = (eps^2 / 2) y + eps z
    double s = gt[j];
#pragma unroll
    for (int m = 0; m < j; ++m) s = s - A[j * (j + 1) / 2 + m] * gt[m];
    gt[j] = s / A[j * (j + 1) / 2 + j];
    w[j] = h * gt[j] + eps * w[j];
  }
#pragma unroll
  for (int j = N - 1; j >= 0; --j) {   // L^T step = w
    double s = w[j];
#pragma unroll
    for (int m = N - 1; m > j; --m) s = s - A[m * (m + 1) / 2 + j] * w[m];
    w[j] = s / A[j * (j + 1) / 2 + j];
  }
  double ut[N];
  bool inside = true;
#pragma unroll
  for (int j = 0; j < N; ++j) {
    ut[j] = su[j] + w[j];
    inside = inside && ut[j] >= a.ulo[j] && ut[j] <= a.uhi[j];   // (a NaN is outside)
  }
  double xt[N];
#pragma unroll
  for (int j = 0; j < N; ++j) {
    double x = sx[j];   // outside: the rows repeat the current point, its evaluation is wasted and its tell rejects
    if (inside) {
      x = (a.log_p || (a.ss && j == N - 1)) ? lm_exp(ut[j]) : ut[j];
      x = x < a.xlo[j] ? a.xlo[j] : x;
      x = x > a.xhi[j] ? a.xhi[j] : x;
    }
    xt[j] = x;
    sut[j] = ut[j];
    sxt[j] = x;
  }
  st[IONODE_MALA_STATE_OUTSIDE] = inside ? 0.0 : 1.0;
  ma_write_trial<N>(a, slot, xt);
}

template <int N>
__global__ void __launch_bounds__(64) ionode_mala_step_kernel(const MaArgs a) {
  const int slot = blockIdx.x * 64 + threadIdx.x;
  if (slot < a.n_active) ma_chain<N>(a, slot);
}

// inst_mala.hip
void launch_mala_step(const MaArgs &a, hipStream_t s);
void mala_step_host(const MaArgs &a);

}  // namespace ionode
