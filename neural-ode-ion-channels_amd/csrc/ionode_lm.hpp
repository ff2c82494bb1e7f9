// ionode_lm.hpp -- one Levenberg-Marquardt step for a whole population of candidates (include/ionode.h "Levenberg-Marquardt step"):
// the per-candidate routine lm_candidate(), shared WORD FOR WORD by the gfx950 kernel (inst_lm.hip) and the host mirror
// (ionode_lm_step_host, ionode_lm_capi.hip).
//
// One call consumes the Gauss-Newton evaluation (ionode_tangent_sweep's sse / jtr / jtj and the forward's status) of the TRIAL
// points the previous call wrote, decides about them, and writes the next trial points:
//   reduce   f_t = sum_p sse, g_t = 2 sum_p jtr[free], H_t = 2 sum_p jtj[free][free], p = 0 .. P - 1 in that order; any non-zero
//            status makes f_t = +inf; log parameters: g_j x_j, H_jl (x_j x_l) -- one product of the two x, so H stays exactly symmetric
//            (only the lower triangle of jtj is read, the upper one is its mirror);
//   decide   rho = (f - f_t) / pred; accept when f_t < f and rho > rho_accept: (u, x, f, g, H) <- trial,
//            lam <- lam max(1/3, 1 - (2 rho - 1)^3), nu <- 2; otherwise lam <- lam nu, nu <- 2 nu (Nielsen 1999).  A state with
//            f = +inf (the first call of a fit) accepts any finite evaluation and leaves lam alone;
//   stop     kLm* flags below; a flagged candidate's state is frozen and its trial rows repeat its accepted point;
//   propose  (H + lam D) delta = -g by Cholesky, D_j = max(H_jj, kLmFloorRel max_l H_ll, kLmFloorAbs) (Marquardt's scaling; the floor
//            makes D positive whenever H is finite); a non-positive or non-finite pivot, or a non-finite delta, raises lam by nu
//            (nu <- 2 nu) and retries, kLmRetries times, then flags the candidate as stalled.  A variable that sits at a bound with
//            the gradient pointing out of the box is held (delta_j = 0, its row and column leave the system) and does not count in
//            the gradient test.  Trial point u + delta in the search
//            space (u = log x, or x), projected into the box; d = the projected step as the trial point realises it (ut - u);
//            pred = -(g . d + d . H d / 2).
//
// Bit-for-bit agreement of the two builds is a property of this file: the library is compiled with -ffp-contract=off -fno-fast-math
// (host and device pass), fp64 + - * / and sqrt are correctly rounded on both, every sum has ONE written order, fma appears only
// inside lm_exp (a correctly rounded operation on both sides) and lm_exp is det_exp's operation sequence (ionode_math.hpp), the only
// transcendental.  The logarithms of the bounds are taken on the host by both entry points and arrive by value.
//
// Execution model: one lane per candidate, NF (the number of free parameters) a template argument -- every loop below unrolls with
// constant indices, the arrays are registers (at NF = 12: the 78 words of the factor's lower triangle and five vectors), nothing is in
// scratch or LDS, there are no cross-lane operations and no atomics, so a candidate's result cannot depend on what shares its
// wavefront or its launch.  The lanes of a wavefront read their candidates' rows with a stride (P x NPAR^2 words apart): the step is
// a few hundred bytes per candidate beside a solve of thousands of accepted steps; the 16-lane row mapping of ionode_tangent.hpp
// would coalesce the loads at the price of a second (lock-step) implementation for the host mirror.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ionode.h"
#include "ionode_step_math.hpp"

namespace ionode {

constexpr int kLmRetries = IONODE_LM_RETRIES;
constexpr double kLmFloorRel = IONODE_LM_FLOOR_REL;
constexpr double kLmFloorAbs = IONODE_LM_FLOOR_ABS;

// The descriptor's settings as the routine wants them: by value (kernel arguments on the device), bounds already in the search space.
struct LmArgs {
  int32_t C, n_active, P, NPAR, nf, log_p, max_iter;
  int32_t free_idx[kLmMaxFree];
  double base[kLmMaxFree];
  double ulo[kLmMaxFree], uhi[kLmMaxFree];   // the box in the search space (log lo, log hi with log_p)
  double xlo[kLmMaxFree], xhi[kLmMaxFree];   // ... and in the parameters
  double gtol, xtol, ftol, rho_accept, lam_max;
  const int32_t *active;   // [n_active] or NULL (slot s is candidate s)
  const double *sse;       // [n_active * P]
  const double *jtr;       // [n_active * P][NPAR]
  const double *jtj;       // [n_active * P][NPAR][NPAR]
  const int32_t *status;   // [n_active * P]
  double *state;           // [C][lm_state_doubles(nf)]
  int32_t *flag;           // [C]
  int32_t *iters;          // [C][2]: evaluations, accepted
  double *trial;           // [n_active * P][NPAR]
};

// state layout of one candidate (IONODE_LM_STATE_* in the header)
__host__ __device__ constexpr int lm_state_doubles(int nf) { return IONODE_LM_STATE_U + 6 * nf + nf * nf; }
__host__ __device__ constexpr int lm_off_u(int) { return IONODE_LM_STATE_U; }
__host__ __device__ constexpr int lm_off_x(int nf) { return IONODE_LM_STATE_U + nf; }
__host__ __device__ constexpr int lm_off_g(int nf) { return IONODE_LM_STATE_U + 2 * nf; }
__host__ __device__ constexpr int lm_off_ut(int nf) { return IONODE_LM_STATE_U + 3 * nf; }
__host__ __device__ constexpr int lm_off_xt(int nf) { return IONODE_LM_STATE_U + 4 * nf; }
__host__ __device__ constexpr int lm_off_delta(int nf) { return IONODE_LM_STATE_U + 5 * nf; }
__host__ __device__ constexpr int lm_off_h(int nf) { return IONODE_LM_STATE_U + 6 * nf; }

// the candidate's P rows of the trial tensor: the base parameters with the free columns replaced by xs[0 .. NF)
template <int NF>
__host__ __device__ inline void lm_write_trial(const LmArgs &a, int slot, const double *xs) {
  for (int p = 0; p < a.P; ++p) {
    double *row = a.trial + ((size_t)slot * a.P + p) * a.NPAR;
#pragma unroll
    for (int i = 0; i < kLmMaxFree; ++i)   // (constant indices into the by-value arguments)
      if (i < a.NPAR) row[i] = a.base[i];
#pragma unroll
    for (int j = 0; j < NF; ++j) row[a.free_idx[j]] = xs[j];
  }
}

// Cholesky of A = H + lam diag(D) in place (lower triangle, row-major packed: A[j (j + 1) / 2 + l], l <= j), then delta = -A^-1 g.
// A held variable (fx[j]: at a bound with the gradient pointing out of the box) has its row and column replaced by the identity's
// and a zero right-hand side: its delta is exactly 0 and the others solve the reduced system.
// false: a pivot was not a positive finite number, or delta is not finite.
template <int NF>
__host__ __device__ inline bool lm_solve(const double *H, const double (&D)[NF], double lam, const double (&g)[NF], const bool (&fx)[NF],
                                         double (&delta)[NF]) {
  double A[NF * (NF + 1) / 2];
#pragma unroll
  for (int j = 0; j < NF; ++j) {
#pragma unroll
    for (int l = 0; l < j; ++l) A[j * (j + 1) / 2 + l] = (fx[j] || fx[l]) ? 0.0 : H[j * NF + l];
    A[j * (j + 1) / 2 + j] = fx[j] ? 1.0 : H[j * NF + j] + lam * D[j];
  }
  bool ok = true;
#pragma unroll
  for (int j = 0; j < NF; ++j) {
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
  double y[NF];
#pragma unroll
  for (int j = 0; j < NF; ++j) {   // L y = -g
    double s = fx[j] ? 0.0 : -g[j];
#pragma unroll
    for (int m = 0; m < j; ++m) s = s - A[j * (j + 1) / 2 + m] * y[m];
    y[j] = s / A[j * (j + 1) / 2 + j];
  }
#pragma unroll
  for (int j = NF - 1; j >= 0; --j) {   // L^T delta = y
    double s = y[j];
#pragma unroll
    for (int m = NF - 1; m > j; --m) s = s - A[m * (m + 1) / 2 + j] * delta[m];
    delta[j] = s / A[j * (j + 1) / 2 + j];
    ok = ok && lm_finite(delta[j]);
  }
  return ok;
}

// One Levenberg-Marquardt step of the candidate in launch slot `slot`.
template <int NF>
__host__ __device__ inline void lm_candidate(const LmArgs &a, int slot) {
  const int c = a.active ? a.active[slot] : slot;
  if (c < 0 || c >= a.C) return;   // (an index list that names no candidate: nothing of it is touched)
  double *st = a.state + (size_t)c * lm_state_doubles(NF);
  double *su = st + lm_off_u(NF), *sx = st + lm_off_x(NF), *sg = st + lm_off_g(NF), *sut = st + lm_off_ut(NF), *sxt = st + lm_off_xt(NF),
         *sdl = st + lm_off_delta(NF), *sH = st + lm_off_h(NF);

  if (a.flag[c] != IONODE_LM_RUNNING) {   // frozen: the slot keeps evaluating the accepted point until the next compaction
    double xs[NF];
#pragma unroll
    for (int j = 0; j < NF; ++j) xs[j] = sx[j];
    lm_write_trial<NF>(a, slot, xs);
    return;
  }

  // ---- reduce: the trial's value ----
  double f_t = 0.0;
  bool failed = false;
  for (int p = 0; p < a.P; ++p) {
    f_t = f_t + a.sse[(size_t)slot * a.P + p];
    failed = failed || a.status[(size_t)slot * a.P + p] != 0;
  }
  if (failed) f_t = lm_inf();

  double f = st[IONODE_LM_STATE_F], lam = st[IONODE_LM_STATE_LAM], nu = st[IONODE_LM_STATE_NU];
  const double pred = st[IONODE_LM_STATE_PRED];
  const int n_eval = a.iters[2 * c] + 1;
  a.iters[2 * c] = n_eval;
  const bool first = !(f < lm_inf());
  int flag = IONODE_LM_RUNNING;

  // ---- decide ----
  bool accept;
  if (first) {
    accept = lm_finite(f_t);
    if (!accept) flag = IONODE_LM_NONFINITE;
  } else {
    const double rho = (f - f_t) / pred;
    accept = f_t < f && rho > a.rho_accept;
    if (accept) {
      const double t = 2.0 * rho - 1.0;
      const double shrink = 1.0 - t * t * t;
      lam = lam * (shrink > 1.0 / 3.0 ? shrink : 1.0 / 3.0);
      nu = 2.0;
    } else {
      lam = lam * nu;
      nu = 2.0 * nu;
    }
  }

  double g[NF], u[NF];
  if (accept) {   // (u, x, f, g, H) <- trial: the trial's derivatives are reduced straight into the state
    if (!first && f - f_t <= a.ftol * f) flag = IONODE_LM_FTOL;
    bool fin = true;
    double xs[NF];
#pragma unroll
    for (int j = 0; j < NF; ++j) {
      xs[j] = sxt[j];
      u[j] = sut[j];
      sx[j] = xs[j];
      su[j] = u[j];
    }
#pragma unroll
    for (int j = 0; j < NF; ++j) {
      double s = 0.0;
      for (int p = 0; p < a.P; ++p) s = s + a.jtr[((size_t)slot * a.P + p) * a.NPAR + a.free_idx[j]];
      s = 2.0 * s;
      if (a.log_p) s = s * xs[j];
      g[j] = s;
      sg[j] = s;
      fin = fin && lm_finite(s);
#pragma unroll
      for (int l = 0; l <= j; ++l) {
        double h = 0.0;
        for (int p = 0; p < a.P; ++p) h = h + a.jtj[(((size_t)slot * a.P + p) * a.NPAR + a.free_idx[j]) * a.NPAR + a.free_idx[l]];
        h = 2.0 * h;
        if (a.log_p) h = h * (xs[j] * xs[l]);
        sH[j * NF + l] = h;
        sH[l * NF + j] = h;
        fin = fin && lm_finite(h);
      }
    }
    f = f_t;
    a.iters[2 * c + 1] = a.iters[2 * c + 1] + 1;
    if (!fin) flag = IONODE_LM_NONFINITE;
  } else {
#pragma unroll
    for (int j = 0; j < NF; ++j) {
      g[j] = sg[j];
      u[j] = su[j];
    }
  }

  // held variables: at a bound, with the gradient pointing out of the box (the step may not push them further)
  bool fx[NF];
#pragma unroll
  for (int j = 0; j < NF; ++j) fx[j] = (u[j] <= a.ulo[j] && g[j] > 0.0) || (u[j] >= a.uhi[j] && g[j] < 0.0);

  // ---- stop: gradient, stalled, iteration cap (an earlier flag keeps its place) ----
  if (flag == IONODE_LM_RUNNING && accept) {
    double gmax = 0.0;
#pragma unroll
    for (int j = 0; j < NF; ++j) gmax = (!fx[j] && __builtin_fabs(g[j]) > gmax) ? __builtin_fabs(g[j]) : gmax;
    if (gmax <= a.gtol) flag = IONODE_LM_GTOL;
  }
  if (flag == IONODE_LM_RUNNING && !(lam <= a.lam_max)) flag = IONODE_LM_STALLED;

  // ---- propose ----
  double delta[NF], ut[NF], xt[NF], pred_next = pred;
  if (flag == IONODE_LM_RUNNING) {
    double D[NF], dmax = 0.0;
#pragma unroll
    for (int j = 0; j < NF; ++j) dmax = sH[j * NF + j] > dmax ? sH[j * NF + j] : dmax;
    const double floor_ = kLmFloorRel * dmax > kLmFloorAbs ? kLmFloorRel * dmax : kLmFloorAbs;
#pragma unroll
    for (int j = 0; j < NF; ++j) D[j] = sH[j * NF + j] > floor_ ? sH[j * NF + j] : floor_;
    bool ok;
    for (int r = 0;; ++r) {
      ok = lm_solve<NF>(sH, D, lam, g, fx, delta);
      if (ok || r == kLmRetries) break;
      lam = lam * nu;
      nu = 2.0 * nu;
    }
    if (!ok || !(lam <= a.lam_max)) {
      flag = IONODE_LM_STALLED;
    } else {
      double d[NF], dd = 0.0, uu = 0.0;
#pragma unroll
      for (int j = 0; j < NF; ++j) {
        double t = u[j] + delta[j];
        t = t < a.ulo[j] ? a.ulo[j] : t;
        t = t > a.uhi[j] ? a.uhi[j] : t;
        ut[j] = t;
        d[j] = t - u[j];
        double x = a.log_p ? lm_exp(t) : t;
        x = x < a.xlo[j] ? a.xlo[j] : x;
        x = x > a.xhi[j] ? a.xhi[j] : x;
        xt[j] = x;
        dd = dd + d[j] * d[j];
        uu = uu + u[j] * u[j];
      }
      double gd = 0.0, dHd = 0.0;
#pragma unroll
      for (int j = 0; j < NF; ++j) {
        gd = gd + g[j] * d[j];
        double hd = 0.0;
#pragma unroll
        for (int l = 0; l < NF; ++l) hd = hd + sH[j * NF + l] * d[l];
        dHd = dHd + d[j] * hd;
      }
      pred_next = -(gd + 0.5 * dHd);
      if (__builtin_sqrt(dd) <= a.xtol * (__builtin_sqrt(uu) + a.xtol)) flag = IONODE_LM_XTOL;
    }
  }
  if (flag == IONODE_LM_RUNNING && n_eval >= a.max_iter) flag = IONODE_LM_MAXITER;

  st[IONODE_LM_STATE_F] = f;
  st[IONODE_LM_STATE_LAM] = lam;
  st[IONODE_LM_STATE_NU] = nu;
  a.flag[c] = flag;
  if (flag == IONODE_LM_RUNNING) {
    st[IONODE_LM_STATE_PRED] = pred_next;
#pragma unroll
    for (int j = 0; j < NF; ++j) {
      sut[j] = ut[j];
      sxt[j] = xt[j];
      sdl[j] = delta[j];
    }
    lm_write_trial<NF>(a, slot, xt);
  } else {
    double xs[NF];
#pragma unroll
    for (int j = 0; j < NF; ++j) xs[j] = sx[j];
    lm_write_trial<NF>(a, slot, xs);
  }
}

template <int NF>
__global__ void __launch_bounds__(64) ionode_lm_step_kernel(const LmArgs a) {
  const int slot = blockIdx.x * 64 + threadIdx.x;
  if (slot < a.n_active) lm_candidate<NF>(a, slot);
}

// inst_lm.hip
void launch_lm_step(const LmArgs &a, hipStream_t s);
void lm_step_host(const LmArgs &a);

}  // namespace ionode
