// ionode_cmaes.hpp -- one CMA-ES generation (tell, then ask) for many independent runs (include/ionode.h "CMA-ES step"): the phase
// functions cm_phase_*(), shared WORD FOR WORD by the gfx950 kernel (inst_cmaes.hip) and the host mirror (ionode_cmaes_step_host).
//
// Hansen's (mu/mu_w, lambda)-CMA-ES, "The CMA Evolution Strategy: A Tutorial" (arXiv 1604.00772), positive weights only.  With
// n search variables, lambda candidates and mu = floor(lambda / 2) (the defaults of the tutorial's table 1; lambda defaults to
// 4 + floor(3 ln n) on the caller's side):
//   w_i     = (ln(mu + 1/2) - ln i) / sum_{l <= mu} (ln(mu + 1/2) - ln l), i = 1 .. mu;   mu_eff = 1 / sum w_i^2
//   c_sigma = (mu_eff + 2) / (n + mu_eff + 5)
//   d_sigma = 1 + 2 max(0, sqrt((mu_eff - 1) / (n + 1)) - 1) + c_sigma
//   c_c     = (4 + mu_eff / n) / (n + 4 + 2 mu_eff / n)
//   c_1     = 2 / ((n + 1.3)^2 + mu_eff)
//   c_mu    = min(1 - c_1, 2 (mu_eff - 2 + 1 / mu_eff) / ((n + 2)^2 + mu_eff))
//   chi_n   = sqrt(n) (1 - 1 / (4 n) + 1 / (21 n^2))
// They are computed once per call on the host (ionode_cmaes_capi.hip, with cm_log below) and arrive by value, as the logarithms of
// the bounds do; a rank's weight is formed where it is used, (ln(mu + 1/2) - cm_log(rank + 1)) / sum.
//
// Execution model: ONE 64-LANE WORKGROUP (one wavefront) PER RUN, the run's state staged in LDS.  At n = 12 a run's C, B, the Jacobi
// work matrix, the paths and up to 64 x 12 evaluated points (17.6 KB) do not fit one lane's registers; they fit LDS many times over.
// The step is a sequence of PHASES.  A phase is a function of (arguments, staged state, run, slot, lane): it reads what earlier
// phases left in the state and writes only elements its lane owns --
//   lane k is candidate k when summing the protocols, ranking and sampling;
//   lane j is coordinate j for the mean and the paths;
//   the lanes stride over the n (n + 1) / 2 elements of C's lower triangle (each with its mirror);
//   in a Jacobi rotation lane k owns row k (the column pass) and then column k (the row pass);
//   lane 0 owns the scalars, the best point, the flag and the counters.
// cm_run() is the order of the phases: the kernel's executor runs a phase on all lanes and puts a workgroup barrier behind it, the
// host's runs it lane after lane.  Control flow between phases reads the staged state only and is uniform over the lanes.  No
// cross-lane instruction, no atomic; every sum is one lane's, in one written order.
//
// Bit-for-bit agreement of the two builds is then a property of this file, as it is for ionode_lm.hpp: the library is compiled with
// -ffp-contract=off -fno-fast-math (host and device pass), fp64 + - * / and sqrt are correctly rounded on both, fma appears only
// inside lm_exp, and the routines below use no libm / ocml call -- the logarithm is cm_log, the normal deviate AS241's rational functions.
#pragma once

#include "ionode_lm.hpp"
#include "ionode_step_math.hpp"

namespace ionode {

constexpr int kCmMaxLambda = IONODE_CMAES_MAX_LAMBDA;
constexpr int kCmResamples = IONODE_CMAES_RESAMPLES;
constexpr int kCmSweeps = IONODE_CMAES_JACOBI_SWEEPS;
constexpr double kCmCondLimit = IONODE_CMAES_CONDITION_LIMIT;

// The descriptor's settings as the phases want them: by value (kernel arguments on the device), bounds already in the search space,
// the strategy constants formed.
struct CmArgs {
  int32_t K, n_active, lam, mu, P, NPAR, n, log_p, max_iter, unchanged_iters, run_base;
  uint32_t seed_lo, seed_hi;
  int32_t free_idx[kLmMaxFree];
  double base[kLmMaxFree];
  double ulo[kLmMaxFree], uhi[kLmMaxFree];   // the box in the search space (log lo, log hi with log_p)
  double xlo[kLmMaxFree], xhi[kLmMaxFree];   // ... and in the parameters
  double unchanged_threshold, tolx;
  double ln_mu_half, sum_w, mu_eff, cs, ds, cc, c1, cmu, chi_n, ln_1mcs;   // ln(mu + 1/2), sum of the raw weights, ..., cm_log(1 - c_sigma)
  const int32_t *active;   // [n_active] or NULL (slot s is run s)
  const double *value;     // [n_active * lam * P]
  const int32_t *status;   // [n_active * lam * P]
  double *state;           // [K][cm_state_doubles(n, lam)]
  int32_t *flag;           // [K]
  int32_t *iters;          // [K][2]: generations sampled, evaluations told
  double *trial;           // [n_active * lam * P][NPAR]
};

// state layout of one run (IONODE_CMAES_STATE_* in the header): scalars, 8 vectors [n], 3 matrices [n][n], f and w [lam], u and x [lam][n]
__host__ __device__ constexpr int cm_state_doubles(int n, int lam) { return IONODE_CMAES_STATE_M + 8 * n + 3 * n * n + 2 * lam + 2 * lam * n; }
__host__ __device__ constexpr int cm_off_m(int) { return IONODE_CMAES_STATE_M; }
__host__ __device__ constexpr int cm_off_mold(int n) { return IONODE_CMAES_STATE_M + n; }
__host__ __device__ constexpr int cm_off_pc(int n) { return IONODE_CMAES_STATE_M + 2 * n; }
__host__ __device__ constexpr int cm_off_ps(int n) { return IONODE_CMAES_STATE_M + 3 * n; }
__host__ __device__ constexpr int cm_off_d(int n) { return IONODE_CMAES_STATE_M + 4 * n; }
__host__ __device__ constexpr int cm_off_bestx(int n) { return IONODE_CMAES_STATE_M + 5 * n; }
__host__ __device__ constexpr int cm_off_yw(int n) { return IONODE_CMAES_STATE_M + 6 * n; }
__host__ __device__ constexpr int cm_off_zw(int n) { return IONODE_CMAES_STATE_M + 7 * n; }
__host__ __device__ constexpr int cm_off_c(int n) { return IONODE_CMAES_STATE_M + 8 * n; }
__host__ __device__ constexpr int cm_off_b(int n) { return cm_off_c(n) + n * n; }
__host__ __device__ constexpr int cm_off_a(int n) { return cm_off_b(n) + n * n; }
__host__ __device__ constexpr int cm_off_f(int n) { return cm_off_a(n) + n * n; }
__host__ __device__ constexpr int cm_off_w(int n, int lam) { return cm_off_f(n) + lam; }
__host__ __device__ constexpr int cm_off_u(int n, int lam) { return cm_off_f(n) + 2 * lam; }
__host__ __device__ constexpr int cm_off_x(int n, int lam) { return cm_off_u(n, lam) + lam * n; }

// ---- the phases ----

// candidate `lane`'s P rows of the trial tensor: the base parameters with the free columns replaced by xs[0 .. N) (lm_write_trial's rule)
template <int N>
__host__ __device__ inline void cm_write_trial(const CmArgs &a, int slot, int lane, const double *xs) {
  for (int p = 0; p < a.P; ++p) {
    double *row = a.trial + (((size_t)slot * a.lam + lane) * a.P + p) * a.NPAR;
#pragma unroll
    for (int i = 0; i < kLmMaxFree; ++i)   // (constant indices into the by-value arguments)
      if (i < a.NPAR) row[i] = a.base[i];
#pragma unroll
    for (int j = 0; j < N; ++j) row[a.free_idx[j]] = xs[j];
  }
}

// frozen, or stopped in this call: every candidate's rows repeat the best point
template <int N>
__host__ __device__ inline void cm_phase_repeat_best(const CmArgs &a, double *st, int slot, int lane) {
  if (lane >= a.lam) return;
  double xs[N];
#pragma unroll
  for (int j = 0; j < N; ++j) xs[j] = st[cm_off_bestx(N) + j];
  cm_write_trial<N>(a, slot, lane, xs);
}

// tell 1, lane k: f_k over the protocols
template <int N>
__host__ __device__ inline void cm_phase_value(const CmArgs &a, double *st, int slot, int lane) {
  if (lane >= a.lam) return;
  double f = 0.0;
  bool failed = false;
  for (int p = 0; p < a.P; ++p) {
    const size_t t = ((size_t)slot * a.lam + lane) * a.P + p;
    f = f + a.value[t];
    failed = failed || a.status[t] != 0;
  }
  if (failed || !(f < lm_inf())) f = lm_inf();   // (a NaN ranks as a failure)
  st[cm_off_f(N) + lane] = f;
}

// tell 2, lane k: its rank among the lambda values by (f, k), and the weight the rank earns; lane 0: the finite values
template <int N>
__host__ __device__ inline void cm_phase_rank(const CmArgs &a, double *st, int lane) {
  if (lane >= a.lam) return;
  const double *f = st + cm_off_f(N);
  const double fk = f[lane];
  int rank = 0, nfin = 0;
  for (int i = 0; i < a.lam; ++i) {
    rank += (f[i] < fk || (f[i] == fk && i < lane)) ? 1 : 0;
    nfin += f[i] < lm_inf() ? 1 : 0;
  }
  st[cm_off_w(N, a.lam) + lane] = rank < a.mu ? (a.ln_mu_half - cm_log((double)(rank + 1))) / a.sum_w : 0.0;
  if (lane == 0) st[IONODE_CMAES_STATE_NFINITE] = (double)nfin;
}

// tell 3, lane j: y_w and the mean
template <int N>
__host__ __device__ inline void cm_phase_mean(const CmArgs &a, double *st, int lane) {
  if (lane >= N) return;
  const double sigma = st[IONODE_CMAES_STATE_SIGMA], mj = st[cm_off_m(N) + lane];
  const double *w = st + cm_off_w(N, a.lam), *u = st + cm_off_u(N, a.lam);
  double s = 0.0;
  for (int k = 0; k < a.lam; ++k)
    if (w[k] != 0.0) s = s + w[k] * ((u[k * N + lane] - mj) / sigma);
  st[cm_off_yw(N) + lane] = s;
  st[cm_off_mold(N) + lane] = mj;
  st[cm_off_m(N) + lane] = mj + sigma * s;
}

// tell 4, lane j: (D^-1 B^T y_w)_j
template <int N>
__host__ __device__ inline void cm_phase_whiten(const CmArgs &, double *st, int lane) {
  if (lane >= N) return;
  const double *B = st + cm_off_b(N), *yw = st + cm_off_yw(N);
  double s = 0.0;
#pragma unroll
  for (int l = 0; l < N; ++l) s = s + B[l * N + lane] * yw[l];
  st[cm_off_zw(N) + lane] = s / st[cm_off_d(N) + lane];
}

// tell 5, lane j: p_sigma
template <int N>
__host__ __device__ inline void cm_phase_psigma(const CmArgs &a, double *st, int lane) {
  if (lane >= N) return;
  const double *B = st + cm_off_b(N), *zw = st + cm_off_zw(N);
  double s = 0.0;
#pragma unroll
  for (int l = 0; l < N; ++l) s = s + B[lane * N + l] * zw[l];
  st[cm_off_ps(N) + lane] = (1.0 - a.cs) * st[cm_off_ps(N) + lane] + __builtin_sqrt(a.cs * (2.0 - a.cs) * a.mu_eff) * s;
}

// tell 6, lane 0: sigma and h_sigma; `tells` counts this one
template <int N>
__host__ __device__ inline void cm_phase_sigma(const CmArgs &a, double *st, int tells, int lane) {
  if (lane != 0) return;
  const double *ps = st + cm_off_ps(N);
  double s = 0.0;
#pragma unroll
  for (int j = 0; j < N; ++j) s = s + ps[j] * ps[j];
  const double norm = __builtin_sqrt(s), sigma = st[IONODE_CMAES_STATE_SIGMA];
  double arg = (a.cs / a.ds) * (norm / a.chi_n - 1.0);
  arg = arg > 1.0 ? 1.0 : arg;
  st[IONODE_CMAES_STATE_SIGMA_OLD] = sigma;
  st[IONODE_CMAES_STATE_SIGMA] = sigma * lm_exp(arg);
  const double decay = 1.0 - lm_exp(2.0 * (double)tells * a.ln_1mcs);   // 1 - (1 - c_sigma)^(2 g)
  st[IONODE_CMAES_STATE_HSIG] = (norm / __builtin_sqrt(decay) / a.chi_n < 1.4 + 2.0 / ((double)N + 1.0)) ? 1.0 : 0.0;
}

// tell 7, lane j: p_c
template <int N>
__host__ __device__ inline void cm_phase_pc(const CmArgs &a, double *st, int lane) {
  if (lane >= N) return;
  st[cm_off_pc(N) + lane] = (1.0 - a.cc) * st[cm_off_pc(N) + lane] +
                            st[IONODE_CMAES_STATE_HSIG] * __builtin_sqrt(a.cc * (2.0 - a.cc) * a.mu_eff) * st[cm_off_yw(N) + lane];
}

// tell 8, lanes stride over the lower triangle: C's rank-one and rank-mu update, symmetrised, written with its mirror; and the Jacobi
// work matrix starts as the new C, B as the identity
template <int N>
__host__ __device__ inline void cm_phase_cov(const CmArgs &a, double *st, int lane) {
  double *C = st + cm_off_c(N), *B = st + cm_off_b(N), *A = st + cm_off_a(N);
  const double *pc = st + cm_off_pc(N), *mold = st + cm_off_mold(N), *w = st + cm_off_w(N, a.lam), *u = st + cm_off_u(N, a.lam);
  const double hs = st[IONODE_CMAES_STATE_HSIG], sig = st[IONODE_CMAES_STATE_SIGMA_OLD];
  const double keep = 1.0 - a.c1 - a.cmu + (1.0 - hs) * a.c1 * a.cc * (2.0 - a.cc);
  for (int e = lane; e < N * (N + 1) / 2; e += 64) {
    int i = 0, rem = e;
    while (rem > i) {   // e = i (i + 1) / 2 + l, l <= i
      rem -= i + 1;
      ++i;
    }
    const int l = rem;
    double r = 0.0;
    for (int k = 0; k < a.lam; ++k)
      if (w[k] != 0.0) r = r + w[k] * (((u[k * N + i] - mold[i]) / sig) * ((u[k * N + l] - mold[l]) / sig));
    const double c = keep * (0.5 * (C[i * N + l] + C[l * N + i])) + a.c1 * (pc[i] * pc[l]) + a.cmu * r;
    C[i * N + l] = c;
    C[l * N + i] = c;
    A[i * N + l] = c;
    A[l * N + i] = c;
    B[i * N + l] = i == l ? 1.0 : 0.0;
    B[l * N + i] = i == l ? 1.0 : 0.0;
  }
}

// Jacobi, lane 0: the rotation that annihilates a_pq -- c and s, or s = 0 where |a_pq| <= 2^-54 sqrt(|a_pp a_qq|) (nothing to do)
template <int N>
__host__ __device__ inline void cm_phase_rot_angle(const CmArgs &, double *st, int p, int q, int lane) {
  if (lane != 0) return;
  const double *A = st + cm_off_a(N);
  const double app = A[p * N + p], aqq = A[q * N + q], apq = A[p * N + q];
  double c = 1.0, s = 0.0;
  if (__builtin_fabs(apq) > 0x1p-54 * __builtin_sqrt(__builtin_fabs(app) * __builtin_fabs(aqq))) {
    const double theta = (aqq - app) / (2.0 * apq);
    const double t = (theta < 0.0 ? -1.0 : 1.0) / (__builtin_fabs(theta) + __builtin_sqrt(theta * theta + 1.0));
    c = 1.0 / __builtin_sqrt(t * t + 1.0);
    s = t * c;
    if (s != 0.0) st[IONODE_CMAES_STATE_NROT] = st[IONODE_CMAES_STATE_NROT] + 1.0;
  }
  st[IONODE_CMAES_STATE_ROT_C] = c;
  st[IONODE_CMAES_STATE_ROT_S] = s;
}

// Jacobi, lane k owns row k: A <- A J and B <- B J touch columns p and q of every row
template <int N>
__host__ __device__ inline void cm_phase_rot_columns(const CmArgs &, double *st, int p, int q, int lane) {
  if (lane >= N) return;
  const double c = st[IONODE_CMAES_STATE_ROT_C], s = st[IONODE_CMAES_STATE_ROT_S];
  double *A = st + cm_off_a(N) + lane * N, *B = st + cm_off_b(N) + lane * N;
  const double ap = A[p], aq = A[q], bp = B[p], bq = B[q];
  A[p] = c * ap - s * aq;
  A[q] = s * ap + c * aq;
  B[p] = c * bp - s * bq;
  B[q] = s * bp + c * bq;
}

// Jacobi, lane k owns column k: A <- J^T A touches rows p and q of every column; the annihilated pair is exactly zero
template <int N>
__host__ __device__ inline void cm_phase_rot_rows(const CmArgs &, double *st, int p, int q, int lane) {
  if (lane >= N) return;
  const double c = st[IONODE_CMAES_STATE_ROT_C], s = st[IONODE_CMAES_STATE_ROT_S];
  double *A = st + cm_off_a(N);
  const double ap = A[p * N + lane], aq = A[q * N + lane];
  A[p * N + lane] = lane == q ? 0.0 : c * ap - s * aq;
  A[q * N + lane] = lane == p ? 0.0 : s * ap + c * aq;
}

template <int N>
__host__ __device__ inline void cm_phase_sweep_begin(const CmArgs &, double *st, int lane) {
  if (lane == 0) st[IONODE_CMAES_STATE_NROT] = 0.0;
}

// Jacobi's end, lane j: D_j from the diagonal
template <int N>
__host__ __device__ inline void cm_phase_eigenvalues(const CmArgs &, double *st, int lane) {
  if (lane >= N) return;
  const double ev = st[cm_off_a(N) + lane * N + lane];
  st[cm_off_d(N) + lane] = __builtin_sqrt(ev > 0.0 ? ev : (ev != ev ? ev : 0.0));
}

// tell's end, lane 0: the best point, the counters, the stop flags.  updated: the state moved (mu finite values were there)
template <int N>
__host__ __device__ inline void cm_phase_stop(const CmArgs &a, double *st, int c, int tells, bool updated, int lane) {
  if (lane != 0) return;
  const double *f = st + cm_off_f(N);
  int kb = 0;
  for (int k = 1; k < a.lam; ++k) kb = f[k] < f[kb] ? k : kb;
  if (f[kb] < st[IONODE_CMAES_STATE_BEST_F]) {
    st[IONODE_CMAES_STATE_BEST_F] = f[kb];
#pragma unroll
    for (int j = 0; j < N; ++j) st[cm_off_bestx(N) + j] = st[cm_off_x(N, a.lam) + kb * N + j];
  }
  a.iters[2 * c + 1] = a.iters[2 * c + 1] + a.lam;
  int flag = IONODE_CMAES_RUNNING;
  const double best = st[IONODE_CMAES_STATE_BEST_F];
  double unchanged = st[IONODE_CMAES_STATE_UNCHANGED];
  if (best < st[IONODE_CMAES_STATE_F_SIG] - a.unchanged_threshold) {   // a significant improvement (PINTS' rule)
    st[IONODE_CMAES_STATE_F_SIG] = best;
    unchanged = 0.0;
  } else {
    unchanged = unchanged + 1.0;
  }
  st[IONODE_CMAES_STATE_UNCHANGED] = unchanged;
  if (!updated) {
    flag = IONODE_CMAES_NONFINITE;
  } else {
    const double sigma = st[IONODE_CMAES_STATE_SIGMA];
    const double *C = st + cm_off_c(N), *pc = st + cm_off_pc(N), *D = st + cm_off_d(N);
    double ext = 0.0, dmax = D[0], dmin = D[0];
    bool fin = lm_finite(sigma) && sigma > 0.0;
#pragma unroll
    for (int j = 0; j < N; ++j) {
      const double sd = __builtin_sqrt(C[j * N + j]), ap = __builtin_fabs(pc[j]);
      const double e = sd > ap ? sd : ap;
      ext = e > ext ? e : ext;
      dmax = D[j] > dmax ? D[j] : dmax;
      dmin = D[j] < dmin ? D[j] : dmin;
      fin = fin && lm_finite(D[j]) && lm_finite(st[cm_off_m(N) + j]);
    }
    const double cond = dmax / dmin;
    st[IONODE_CMAES_STATE_COND] = cond;
    if (!fin) flag = IONODE_CMAES_NONFINITE;
    else if (unchanged >= (double)a.unchanged_iters) flag = IONODE_CMAES_UNCHANGED;
    else if (sigma * ext < a.tolx) flag = IONODE_CMAES_TOLX;
    else if (!(cond <= kCmCondLimit)) flag = IONODE_CMAES_CONDITION;
    else if (tells >= a.max_iter) flag = IONODE_CMAES_MAXITER;
  }
  st[IONODE_CMAES_STATE_FLAG] = (double)flag;
  a.flag[c] = flag;
  if (flag == IONODE_CMAES_RUNNING) a.iters[2 * c] = tells + 1;
}

// the first call's only bookkeeping, lane 0: generation 0 is about to be sampled
template <int N>
__host__ __device__ inline void cm_phase_first(const CmArgs &a, double *, int c, int lane) {
  if (lane == 0) a.iters[2 * c] = 1;
}

// ask, lane k: candidate k of generation `gen`
template <int N>
__host__ __device__ inline void cm_phase_ask(const CmArgs &a, double *st, int c, int slot, int gen, int lane) {
  if (lane >= a.lam) return;
  const double sigma = st[IONODE_CMAES_STATE_SIGMA];
  const double *m = st + cm_off_m(N), *B = st + cm_off_b(N), *D = st + cm_off_d(N);
  double u[N];
  for (int attempt = 0;; ++attempt) {
    double dz[N];
#pragma unroll
    for (int jp = 0; jp < (N + 1) / 2; ++jp) {
      double z0, z1;
      cm_normal_pair(a.seed_lo, a.seed_hi, a.run_base + c, gen, lane, jp, attempt, z0, z1);
      dz[2 * jp] = D[2 * jp] * z0;
      if (2 * jp + 1 < N) dz[2 * jp + 1] = D[2 * jp + 1] * z1;
    }
    bool inside = true;
#pragma unroll
    for (int j = 0; j < N; ++j) {
      double s = 0.0;
#pragma unroll
      for (int l = 0; l < N; ++l) s = s + B[j * N + l] * dz[l];
      u[j] = m[j] + sigma * s;
      inside = inside && u[j] >= a.ulo[j] && u[j] <= a.uhi[j];
    }
    if (inside || attempt == kCmResamples) break;
  }
  double xs[N];
#pragma unroll
  for (int j = 0; j < N; ++j) {
    double t = u[j];
    t = t < a.ulo[j] ? a.ulo[j] : t;
    t = t > a.uhi[j] ? a.uhi[j] : t;
    double x = a.log_p ? lm_exp(t) : t;
    x = x < a.xlo[j] ? a.xlo[j] : x;
    x = x > a.xhi[j] ? a.xhi[j] : x;
    xs[j] = x;
    st[cm_off_u(N, a.lam) + lane * N + j] = t;
    st[cm_off_x(N, a.lam) + lane * N + j] = x;
  }
  cm_write_trial<N>(a, slot, lane, xs);
}

// The order of the phases for the run `c` in launch slot `slot`, on its staged state.  ex(f) runs f(lane) for the 64 lanes and
// makes what they wrote visible to all of them.  flag0 / gen0: the run's flag and generation counter as they were on entry (read
// by the caller before any lane writes them).
template <int N, class Exec>
__host__ __device__ inline void cm_run(const CmArgs &a, double *st, int c, int slot, int flag0, int gen0, const Exec &ex) {
  if (flag0 != IONODE_CMAES_RUNNING) {
    ex([&](int lane) { cm_phase_repeat_best<N>(a, st, slot, lane); });
    return;
  }
  if (gen0 == 0) {
    ex([&](int lane) { cm_phase_first<N>(a, st, c, lane); });
    ex([&](int lane) { cm_phase_ask<N>(a, st, c, slot, 0, lane); });
    return;
  }
  const int tells = gen0;   // generations 0 .. gen0 - 1 have been sampled; this call tells the last of them
  ex([&](int lane) { cm_phase_value<N>(a, st, slot, lane); });
  ex([&](int lane) { cm_phase_rank<N>(a, st, lane); });
  const bool updated = st[IONODE_CMAES_STATE_NFINITE] >= (double)a.mu;
  if (updated) {
    ex([&](int lane) { cm_phase_mean<N>(a, st, lane); });
    ex([&](int lane) { cm_phase_whiten<N>(a, st, lane); });
    ex([&](int lane) { cm_phase_psigma<N>(a, st, lane); });
    ex([&](int lane) { cm_phase_sigma<N>(a, st, tells, lane); });
    ex([&](int lane) { cm_phase_pc<N>(a, st, lane); });
    ex([&](int lane) { cm_phase_cov<N>(a, st, lane); });
    for (int sweep = 0; sweep < kCmSweeps; ++sweep) {
      ex([&](int lane) { cm_phase_sweep_begin<N>(a, st, lane); });
      for (int p = 0; p < N - 1; ++p)
        for (int q = p + 1; q < N; ++q) {
          ex([&](int lane) { cm_phase_rot_angle<N>(a, st, p, q, lane); });
          if (st[IONODE_CMAES_STATE_ROT_S] == 0.0) continue;
          ex([&](int lane) { cm_phase_rot_columns<N>(a, st, p, q, lane); });
          ex([&](int lane) { cm_phase_rot_rows<N>(a, st, p, q, lane); });
        }
      if (st[IONODE_CMAES_STATE_NROT] == 0.0) break;
    }
    ex([&](int lane) { cm_phase_eigenvalues<N>(a, st, lane); });
  }
  ex([&](int lane) { cm_phase_stop<N>(a, st, c, tells, updated, lane); });
  if (st[IONODE_CMAES_STATE_FLAG] == (double)IONODE_CMAES_RUNNING)
    ex([&](int lane) { cm_phase_ask<N>(a, st, c, slot, tells, lane); });
  else
    ex([&](int lane) { cm_phase_repeat_best<N>(a, st, slot, lane); });
}

struct CmDeviceExec {
  template <class F>
  __device__ void operator()(const F &f) const {
    f((int)threadIdx.x);
    __syncthreads();
  }
};

struct CmHostExec {
  template <class F>
  void operator()(const F &f) const {
    for (int lane = 0; lane < 64; ++lane) f(lane);
  }
};

template <int N>
__global__ void __launch_bounds__(64) ionode_cmaes_step_kernel(const CmArgs a) {
  __shared__ double st[cm_state_doubles(N, kCmMaxLambda)];
  const int slot = blockIdx.x, lane = threadIdx.x;
  const int c = a.active ? a.active[slot] : slot;
  if (c < 0 || c >= a.K) return;   // (an index list that names no run: nothing of it is touched; uniform over the workgroup)
  const int words = cm_state_doubles(N, a.lam);
  double *g = a.state + (size_t)c * words;
  const int flag0 = a.flag[c], gen0 = a.iters[2 * c];
  for (int i = lane; i < words; i += 64) st[i] = g[i];
  __syncthreads();   // (also orders every lane's read of flag and iters before lane 0's writes)
  cm_run<N>(a, st, c, slot, flag0, gen0, CmDeviceExec{});
  for (int i = lane; i < words; i += 64) g[i] = st[i];
}

template <int N>
inline void cm_run_host(const CmArgs &a, int slot) {
  const int c = a.active ? a.active[slot] : slot;
  if (c < 0 || c >= a.K) return;
  cm_run<N>(a, a.state + (size_t)c * cm_state_doubles(N, a.lam), c, slot, a.flag[c], a.iters[2 * c], CmHostExec{});
}

// inst_cmaes.hip
void launch_cmaes_step(const CmArgs &a, hipStream_t s);
void cmaes_step_host(const CmArgs &a);

}  // namespace ionode
