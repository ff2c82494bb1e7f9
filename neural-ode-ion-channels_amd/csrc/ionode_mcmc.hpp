// ionode_mcmc.hpp -- one adaptive-Metropolis iteration (tell, then propose) for many independent chains (include/ionode.h "Adaptive
// Metropolis step"): the per-chain routine mc_chain(), shared WORD FOR WORD by the gfx950 kernel (inst_mcmc.hip) and the host mirror
// (ionode_mcmc_step_host).
//
// Haario, Saksman and Tamminen's adaptive Metropolis ("An adaptive Metropolis algorithm", Bernoulli 7, 2001) with global adaptive
// scaling, in the form of Andrieu and Thoms, "A tutorial on adaptive MCMC" (Statistics and Computing 18, 2008), Algorithm 4.  A chain
// has n = nf + sample_sigma coordinates u: the nf free rate parameters (log x or x) and, when the noise level is sampled, log sigma as
// the last.  One call, for a running chain at iteration t (iters[chain][0] on entry):
//   reduce   S = sum_p value, p = 0 .. P - 1 in that order; a non-zero status or a NaN makes S = +inf
//   target   lp_t = -N u_sigma - (S / 2) exp(-2 u_sigma) at the evaluated point (-inf for S = +inf)
//   t = 0    the evaluation is the start's: lp <- lp_t, nothing is decided, nothing adapts
//   tell     alpha = 0 for a proposal that was outside the box or a non-finite lp_t, else exp(min(lp_t - lp, 0)); accepted iff alpha > 0
//            and log w < lp_t - lp, w the first uniform of (chain_base + chain, t, 1, 0)
//   adapt    from t = adapt_start on: k = t - adapt_start + 2, gamma = exp(-eta log k), mu <- mu + gamma (u - mu),
//            C <- C + gamma ((u - mu)(u - mu)^T - C) with the new mu, log_lambda <- log_lambda + gamma (alpha - target_accept)
//   record   t % thin == 0 and t / thin < sample_cap: samples[chain][t / thin] <- (x, lp)
//   stop     kMc* flags: the start not evaluable, a failed factorisation, the iteration cap
//   propose  L L^T = exp(log_lambda) (C + epsilon I), ut = u + L z, z the deviates of (chain_base + chain, t + 1, 0, pair); outside the box
//            the slot's rows repeat the current x and the next tell rejects, inside they carry xt
//
// Bit-for-bit agreement of the two builds is a property of this file, as it is for ionode_lm.hpp and ionode_cmaes.hpp: the units are
// compiled with -ffp-contract=off -fno-fast-math (host and device pass), fp64 + - * / and sqrt are correctly rounded on both, every sum
// has ONE written order, the only transcendentals are lm_exp and cm_log, and the generator is the CMA-ES step's (ionode_step_math.hpp:
// cm_philox, cm_uniform, cm_ppnd16), unchanged.  A failed factorisation is never stored (a NaN's sign is not the same everywhere).
//
// Execution model: ionode_lm.hpp's.  One lane per chain, N (the number of coordinates) a template argument -- every loop unrolls with
// constant indices; mu and C are updated element by element straight from and to the state, so the packed lower triangle of the factor
// (91 words at N = 13) is the only large thing live in registers.  Nothing is in scratch or LDS, there are no cross-lane operations and
// no atomics: a chain's result cannot depend on what shares its wavefront or its launch.
#pragma once

#include "ionode_step_math.hpp"

namespace ionode {

constexpr int kMcMaxDim = IONODE_MCMC_MAX_DIM;

// The descriptor's settings as the routine wants them: by value (kernel arguments on the device).  Coordinate j < nf is free parameter j;
// with ss the coordinate nf is log sigma: its box and its parameter bounds sit at index nf of the four bound arrays.
struct McArgs {
  int32_t K, n_active, P, NPAR, nf, n, log_p, ss, max_iter, adapt_start, thin, sample_cap, chain_base;
  uint32_t seed_lo, seed_hi;
  int32_t free_idx[kLmMaxFree];
  double base[kLmMaxFree];
  double ulo[kMcMaxDim], uhi[kMcMaxDim];   // the box in the search space
  double xlo[kMcMaxDim], xhi[kMcMaxDim];   // ... and in the parameters
  double n_samples, log_sigma, eta, target_accept, epsilon;   // log_sigma: of the fixed sigma (without ss)
  const int32_t *active;   // [n_active] or NULL (slot s is chain s)
  const double *value;     // [n_active * P]
  const int32_t *status;   // [n_active * P]
  double *state;           // [K][mc_state_doubles(n)]
  int32_t *flag;           // [K]
  int32_t *iters;          // [K][2]: tells, accepted
  double *trial;           // [n_active * P][NPAR]
  double *samples;         // [K][sample_cap][n + 1] or NULL
};

// state layout of one chain (IONODE_MCMC_STATE_* in the header): 4 scalars, u, ut, x, xt, mu [n], C and L [n][n]
__host__ __device__ constexpr int mc_state_doubles(int n) { return IONODE_MCMC_STATE_U + 5 * n + 2 * n * n; }
__host__ __device__ constexpr int mc_off_u(int) { return IONODE_MCMC_STATE_U; }
__host__ __device__ constexpr int mc_off_ut(int n) { return IONODE_MCMC_STATE_U + n; }
__host__ __device__ constexpr int mc_off_x(int n) { return IONODE_MCMC_STATE_U + 2 * n; }
__host__ __device__ constexpr int mc_off_xt(int n) { return IONODE_MCMC_STATE_U + 3 * n; }
__host__ __device__ constexpr int mc_off_mu(int n) { return IONODE_MCMC_STATE_U + 4 * n; }
__host__ __device__ constexpr int mc_off_c(int n) { return IONODE_MCMC_STATE_U + 5 * n; }
__host__ __device__ constexpr int mc_off_l(int n) { return IONODE_MCMC_STATE_U + 5 * n + n * n; }

// the chain's P rows of the trial tensor: the base parameters with the free columns replaced by xs[0 .. nf) (sigma never enters them)
template <int N>
__host__ __device__ inline void mc_write_trial(const McArgs &a, int slot, const double *xs) {
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
__host__ __device__ inline void mc_chain(const McArgs &a, int slot) {
  const int c = a.active ? a.active[slot] : slot;
  if (c < 0 || c >= a.K) return;   // (an index list that names no chain: nothing of it is touched)
  double *st = a.state + (size_t)c * mc_state_doubles(N);
  double *su = st + mc_off_u(N), *sut = st + mc_off_ut(N), *sx = st + mc_off_x(N), *sxt = st + mc_off_xt(N), *smu = st + mc_off_mu(N),
         *sC = st + mc_off_c(N), *sL = st + mc_off_l(N);

  if (a.flag[c] != IONODE_MCMC_RUNNING) {   // frozen: the slot keeps evaluating the current point until the next compaction
    double xs[N];
#pragma unroll
    for (int j = 0; j < N; ++j) xs[j] = sx[j];
    mc_write_trial<N>(a, slot, xs);
    return;
  }

  // ---- reduce: the evaluated point's sum of squares ----
  double S = 0.0;
  bool failed = false;
  for (int p = 0; p < a.P; ++p) {
    S = S + a.value[(size_t)slot * a.P + p];
    failed = failed || a.status[(size_t)slot * a.P + p] != 0;
  }
  if (failed || !(S < lm_inf())) S = lm_inf();   // (a NaN counts as a failure)

  const int t = a.iters[2 * c];
  const bool outside = st[IONODE_MCMC_STATE_OUTSIDE] != 0.0;
  double lp = st[IONODE_MCMC_STATE_LP], log_lambda = st[IONODE_MCMC_STATE_LOG_LAMBDA];
  int flag = IONODE_MCMC_RUNNING;

  // ---- target: the log-posterior of what was evaluated (the start at t = 0, else the proposal) ----
  const double ls_u = su[N - 1], ls_ut = sut[N - 1];   // (both loaded, then chosen by value: a choice of addresses would put log_sigma in scratch)
  double ls = a.log_sigma;
  if (a.ss) ls = t == 0 ? ls_u : ls_ut;
  const double lp_t = S < lm_inf() ? -a.n_samples * ls - (0.5 * S) * lm_exp(-2.0 * ls) : -lm_inf();

  double u[N];
  if (t == 0) {
    bool inside = true;
#pragma unroll
    for (int j = 0; j < N; ++j) {
      u[j] = su[j];
      inside = inside && u[j] >= a.ulo[j] && u[j] <= a.uhi[j];
    }
    lp = lp_t;
    if (!inside || !lm_finite(lp)) flag = IONODE_MCMC_NONFINITE;
  } else {
    // ---- tell: the Metropolis decision ----
    const double diff = lp_t - lp;
    double alpha = 0.0;
    if (!outside && lm_finite(lp_t)) alpha = lm_exp(diff < 0.0 ? diff : 0.0);
    uint32_t w[4];
    cm_philox((uint32_t)(a.chain_base + c), (uint32_t)t, 1u, 0u, a.seed_lo, a.seed_hi, w);
    const bool accept = alpha > 0.0 && cm_log(cm_uniform(w[0], w[1])) < diff;
    if (accept) {
#pragma unroll
      for (int j = 0; j < N; ++j) {
        u[j] = sut[j];
        su[j] = u[j];
        sx[j] = sxt[j];
      }
      lp = lp_t;
      a.iters[2 * c + 1] = a.iters[2 * c + 1] + 1;
    } else {
#pragma unroll
      for (int j = 0; j < N; ++j) u[j] = su[j];
    }
    st[IONODE_MCMC_STATE_ALPHA] = alpha;
    // ---- adapt: mean, covariance (with the new mean) and the global scale ----
    if (t >= a.adapt_start) {
      const double gamma = lm_exp(-a.eta * cm_log((double)(t - a.adapt_start + 2)));
      double d[N];
#pragma unroll
      for (int j = 0; j < N; ++j) {
        const double m = smu[j] + gamma * (u[j] - smu[j]);
        smu[j] = m;
        d[j] = u[j] - m;
      }
#pragma unroll
      for (int j = 0; j < N; ++j) {
#pragma unroll
        for (int l = 0; l <= j; ++l) {
          const double cjl = sC[j * N + l];
          const double v = cjl + gamma * (d[j] * d[l] - cjl);
          sC[j * N + l] = v;
          sC[l * N + j] = v;
        }
      }
      log_lambda = log_lambda + gamma * (alpha - a.target_accept);
    }
  }
  st[IONODE_MCMC_STATE_LP] = lp;
  st[IONODE_MCMC_STATE_LOG_LAMBDA] = log_lambda;

  // ---- record: in the parameters ----
  if (a.samples && t % a.thin == 0 && t / a.thin < a.sample_cap) {
    double *row = a.samples + ((size_t)c * a.sample_cap + (size_t)(t / a.thin)) * (N + 1);
#pragma unroll
    for (int j = 0; j < N; ++j) row[j] = sx[j];
    row[N] = lp;
  }

  // ---- factor: L L^T = exp(log_lambda) (C + epsilon I), lower triangle packed by rows (lm_solve's order of operations) ----
  bool ok = false;
  double A[N * (N + 1) / 2];
  if (flag == IONODE_MCMC_RUNNING) {
    const double lam = lm_exp(log_lambda);
    ok = lm_finite(log_lambda);
#pragma unroll
    for (int j = 0; j < N; ++j) {
#pragma unroll
      for (int l = 0; l <= j; ++l) {
        const double cjl = sC[j * N + l];
        ok = ok && lm_finite(cjl);
        A[j * (j + 1) / 2 + l] = lam * (l == j ? cjl + a.epsilon : cjl);
      }
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
      A[j * (j + 1) / 2 + j] = __builtin_sqrt(piv);   // (a failed pivot poisons what follows; `ok` discards it)
    }
    if (!ok) flag = IONODE_MCMC_DEGENERATE;
    else if (t >= a.max_iter) flag = IONODE_MCMC_MAXITER;
  }
  if (ok) {
#pragma unroll
    for (int j = 0; j < N; ++j)
#pragma unroll
      for (int l = 0; l < N; ++l) sL[j * N + l] = l <= j ? A[j * (j + 1) / 2 + l] : 0.0;
  }

  a.flag[c] = flag;
  if (flag != IONODE_MCMC_RUNNING) {   // stopped in this call: the rows repeat the current point, the counter stays at this tell
    double xs[N];
#pragma unroll
    for (int j = 0; j < N; ++j) xs[j] = sx[j];
    mc_write_trial<N>(a, slot, xs);
    return;
  }
  a.iters[2 * c] = t + 1;

  // ---- propose ----
  double z[N];
#pragma unroll
  for (int jp = 0; jp < (N + 1) / 2; ++jp) {
    double z0, z1;
    cm_normal_pair(a.seed_lo, a.seed_hi, a.chain_base + c, t + 1, 0, jp, 0, z0, z1);
    z[2 * jp] = z0;
    if (2 * jp + 1 < N) z[2 * jp + 1] = z1;
  }
  double ut[N];
  bool inside = true;
#pragma unroll
  for (int j = 0; j < N; ++j) {
    double s = 0.0;
#pragma unroll
    for (int l = 0; l <= j; ++l) s = s + A[j * (j + 1) / 2 + l] * z[l];
    ut[j] = u[j] + s;
    inside = inside && ut[j] >= a.ulo[j] && ut[j] <= a.uhi[j];
  }
  double xt[N];
#pragma unroll
  for (int j = 0; j < N; ++j) {
    double x = sx[j];   // outside: the rows repeat the current point, its solve is wasted and its tell rejects
    if (inside) {
      x = (a.log_p || (a.ss && j == N - 1)) ? lm_exp(ut[j]) : ut[j];
      x = x < a.xlo[j] ? a.xlo[j] : x;
      x = x > a.xhi[j] ? a.xhi[j] : x;
    }
    xt[j] = x;
    sut[j] = ut[j];
    sxt[j] = x;
  }
  st[IONODE_MCMC_STATE_OUTSIDE] = inside ? 0.0 : 1.0;
  mc_write_trial<N>(a, slot, xt);
}

template <int N>
__global__ void __launch_bounds__(64) ionode_mcmc_step_kernel(const McArgs a) {
  const int slot = blockIdx.x * 64 + threadIdx.x;
  if (slot < a.n_active) mc_chain<N>(a, slot);
}

// inst_mcmc.hip
void launch_mcmc_step(const McArgs &a, hipStream_t s);
void mcmc_step_host(const McArgs &a);

}  // namespace ionode
