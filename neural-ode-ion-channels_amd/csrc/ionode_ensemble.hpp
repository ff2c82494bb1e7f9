// ionode_ensemble.hpp -- one half-iteration (tell, then ask) of many affine-invariant ensembles (include/ionode.h "Affine-invariant
// ensemble step"): the per-ensemble routine en_ensemble(), shared WORD FOR WORD by the gfx950 kernel (inst_ensemble.hip) and the host
// mirror (ionode_ensemble_step_host).
//
// Goodman and Weare's stretch move ("Ensemble samplers with affine invariance", Comm. App. Math. Comp. Sci. 5, 2010) in the parallel
// form of Foreman-Mackey et al. ("emcee: the MCMC hammer", PASP 125, 2013), and ter Braak's differential-evolution move ("A Markov
// chain Monte Carlo version of the genetic algorithm Differential Evolution", Stat. Comput. 16, 2006) in the same form: the W walkers
// of an ensemble are two halves, and a half moves at once with its partners drawn from the other half, which stands still until the
// movers have been told.  An ensemble has n = nf + sample_sigma coordinates per walker; one call at the ensemble's counter t
// (iters[e][0] on entry):
//   t = 0    reduce and target for all W walkers: lp <- the start's; row 0 recorded; a start outside the box or a non-finite lp flags
//            the ensemble; else ask half 0
//   tell     half (t - 1) % 2: S = sum_p value in order (a status or a NaN: +inf), lp_t at ut, alpha = 0 for OUTSIDE or a non-finite
//            lp_t, accepted iff alpha > 0 and log w3 < (lp_t + lq) - lp
//   record   t even: full iteration i = t / 2, i % thin == 0 and i / thin < sample_cap: samples[e][walker][i / thin] <- (x, lp), all W
//   stop     t = 2 max_iter: kEnMaxIter, nothing asked
//   barrier  the tell's u are the ask's partners
//   ask      half t % 2: stretch ut = u_j + z (u_k - u_j), lq = (n - 1) log z; DE ut = (u_k + gamma (u_a - u_b)) + jitter xi, lq = 0
//
// Bit-for-bit agreement of the two builds is a property of this file, as it is for ionode_mcmc.hpp: the units are compiled with
// -ffp-contract=off -fno-fast-math (host and device pass), fp64 + - * / are correctly rounded on both, every sum has ONE written
// order, the only transcendentals are lm_exp and cm_log, and the generator is the CMA-ES step's (ionode_step_math.hpp), unchanged.
//
// Execution model: one workgroup of kEnLanes lanes per ensemble; lane l serves walkers l, l + kEnLanes, ... of the half in turn; N
// (the coordinates) is a template argument, so every per-walker array has constant indices and lives in registers.  A walker is told
// and asked by the same lane, which alone writes its state words; what a lane reads of OTHER walkers is their u, written before the
// barrier by the tell and by nobody after it (the ask writes ut, xt, lq and the OUTSIDE word).  flag and iters are read by every lane
// on entry and written by lane 0 behind the barrier.  The host mirror is the same routine run as lane 0 of 1, en_barrier() a no-op.
// No atomics, no scratch.
#pragma once

#include "ionode_step_math.hpp"

namespace ionode {

constexpr int kEnMaxDim = IONODE_MCMC_MAX_DIM;
constexpr int kEnLanes = 256;

// The descriptor's settings as the routine wants them: by value (kernel arguments on the device).  Coordinate j < nf is free parameter j;
// with ss the coordinate nf is log sigma: its box and its parameter bounds sit at index nf of the four bound arrays.
struct EnArgs {
  int32_t E, W, H, P, NPAR, nf, n, log_p, ss, max_iter, thin, sample_cap, ensemble_base, move;
  uint32_t seed_lo, seed_hi;
  int32_t free_idx[kLmMaxFree];
  double base[kLmMaxFree];
  double ulo[kEnMaxDim], uhi[kEnMaxDim];   // the box in the search space
  double xlo[kEnMaxDim], xhi[kEnMaxDim];   // ... and in the parameters
  double n_samples, log_sigma, a, gamma, jitter;   // log_sigma: of the fixed sigma (without ss)
  const double *value;     // [E * W * P] at t = 0, [E * H * P] after
  const int32_t *status;   // as value
  double *state;           // [E][W][en_state_doubles(n)]
  int32_t *flag;           // [E]
  int32_t *iters;          // [E][2]: calls, full iterations told
  int32_t *accepted;       // [E][W]
  double *trial;           // [E * W * P][NPAR]; the asks fill the first E * H * P rows
  double *samples;         // [E][W][sample_cap][n + 1] or NULL
};

// state layout of one walker (IONODE_ENSEMBLE_STATE_* in the header): 3 scalars, then u, ut, x, xt [n]
__host__ __device__ constexpr int en_state_doubles(int n) { return IONODE_ENSEMBLE_STATE_U + 4 * n; }

__host__ __device__ inline void en_barrier() {
#if defined(__HIP_DEVICE_COMPILE__)
  __syncthreads();
#endif
}

// the P trial rows of launch slot `slot`: the base parameters with the free columns replaced by xs[0 .. nf) (sigma never enters them)
template <int N>
__host__ __device__ inline void en_write_trial(const EnArgs &a, int slot, const double *xs) {
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

// the H slots of a stopped ensemble: the current x of half 0's walkers
template <int N>
__host__ __device__ inline void en_write_current(const EnArgs &a, int e, int lane, int lanes) {
  for (int k = lane; k < a.H; k += lanes) {
    const double *sx = a.state + ((size_t)e * a.W + k) * en_state_doubles(N) + IONODE_ENSEMBLE_STATE_U + 2 * N;
    double xs[N];
#pragma unroll
    for (int j = 0; j < N; ++j) xs[j] = sx[j];
    en_write_trial<N>(a, e * a.H + k, xs);
  }
}

// the log-posterior of walker state `st` at its u (at_ut false) or ut, from the P rows of launch slot `slot`
template <int N>
__host__ __device__ inline double en_target(const EnArgs &a, const double *st, int slot, bool at_ut) {
  double S = 0.0;
  bool failed = false;
  for (int p = 0; p < a.P; ++p) {
    S = S + a.value[(size_t)slot * a.P + p];
    failed = failed || a.status[(size_t)slot * a.P + p] != 0;
  }
  if (failed || !(S < lm_inf())) S = lm_inf();   // (a NaN counts as a failure)
  const double ls_u = st[IONODE_ENSEMBLE_STATE_U + N - 1], ls_ut = st[IONODE_ENSEMBLE_STATE_U + 2 * N - 1];   // (both loaded, then chosen by value)
  double ls = a.log_sigma;
  if (a.ss) ls = at_ut ? ls_ut : ls_u;
  return S < lm_inf() ? -a.n_samples * ls - (0.5 * S) * lm_exp(-2.0 * ls) : -lm_inf();
}

template <int N>
__host__ __device__ inline void en_record(const EnArgs &a, int e, int w, const double *st, int row_index) {
  double *row = a.samples + (((size_t)e * a.W + w) * a.sample_cap + (size_t)row_index) * (N + 1);
#pragma unroll
  for (int j = 0; j < N; ++j) row[j] = st[IONODE_ENSEMBLE_STATE_U + 2 * N + j];
  row[N] = st[IONODE_ENSEMBLE_STATE_LP];
}

// One call of ensemble e, as lane `lane` of `lanes`; *bad is a word all lanes of the ensemble share.
template <int N>
__host__ __device__ inline void en_ensemble(const EnArgs &a, int e, int lane, int lanes, int *bad) {
  constexpr int SD = en_state_doubles(N), OU = IONODE_ENSEMBLE_STATE_U, OUT = OU + N, OX = OU + 2 * N, OXT = OU + 3 * N;
  double *ens = a.state + (size_t)e * a.W * SD;
  const int H = a.H;
  const int t = a.iters[2 * e];
  if (a.flag[e] != IONODE_ENSEMBLE_RUNNING) {   // frozen (uniform over the workgroup: no lane has written the flag yet)
    en_write_current<N>(a, e, lane, lanes);
    return;
  }
  const uint32_t run = (uint32_t)(a.ensemble_base + e);
  int flag = IONODE_ENSEMBLE_RUNNING;

  if (t == 0) {
    // ---- the starts' evaluation: all W walkers ----
    if (lane == 0) *bad = 0;
    en_barrier();
    for (int w = lane; w < a.W; w += lanes) {
      double *st = ens + (size_t)w * SD;
      const double lp = en_target<N>(a, st, e * a.W + w, false);
      bool inside = true;
#pragma unroll
      for (int j = 0; j < N; ++j) inside = inside && st[OU + j] >= a.ulo[j] && st[OU + j] <= a.uhi[j];
      st[IONODE_ENSEMBLE_STATE_LP] = lp;
      if (!inside || !lm_finite(lp)) *bad = 1;   // (every finder stores the same word)
      if (a.samples && a.sample_cap > 0) en_record<N>(a, e, w, st, 0);
    }
    en_barrier();
    if (*bad != 0) flag = IONODE_ENSEMBLE_NONFINITE;
  } else {
    // ---- tell: the Metropolis-Hastings decision of half (t - 1) % 2, walker by walker ----
    const int hp = (t - 1) & 1;
    for (int k = lane; k < H; k += lanes) {
      const int w = hp * H + k;
      double *st = ens + (size_t)w * SD;
      const double lp_t = en_target<N>(a, st, e * H + k, true);
      const double lp = st[IONODE_ENSEMBLE_STATE_LP];
      const double ratio = (lp_t + st[IONODE_ENSEMBLE_STATE_LQ]) - lp;
      const bool live = st[IONODE_ENSEMBLE_STATE_OUTSIDE] == 0.0 && lm_finite(lp_t);   // alpha > 0
      uint32_t r[4];
      cm_philox(run, (uint32_t)t, (uint32_t)w, 65536u * 1u, a.seed_lo, a.seed_hi, r);
      if (live && cm_log(cm_uniform(r[0], r[1])) < ratio) {
#pragma unroll
        for (int j = 0; j < N; ++j) {
          st[OU + j] = st[OUT + j];
          st[OX + j] = st[OXT + j];
        }
        st[IONODE_ENSEMBLE_STATE_LP] = lp_t;
        a.accepted[(size_t)e * a.W + w] = a.accepted[(size_t)e * a.W + w] + 1;
      }
      // ---- record: a full iteration ends with half 1's tell; this lane's walker of half 0 has not moved since its own ----
      if (hp == 1 && a.samples) {
        const int i = t / 2;
        if (i % a.thin == 0 && i / a.thin < a.sample_cap) {
          en_record<N>(a, e, k, ens + (size_t)k * SD, i / a.thin);
          en_record<N>(a, e, w, st, i / a.thin);
        }
      }
    }
    if (t >= 2 * a.max_iter) flag = IONODE_ENSEMBLE_MAXITER;
    en_barrier();   // the movers' u stand: they are the partners now
  }

  if (lane == 0) {
    a.flag[e] = flag;
    if (flag == IONODE_ENSEMBLE_RUNNING) a.iters[2 * e] = t + 1;
    if (t >= 2 && (t & 1) == 0) a.iters[2 * e + 1] = t / 2;
  }
  if (flag != IONODE_ENSEMBLE_RUNNING) {   // stopped in this call: the counter stays, the rows repeat the current points
    en_write_current<N>(a, e, lane, lanes);
    return;
  }

  // ---- ask: half t % 2 moves against the other half as it stands ----
  const int h = t & 1;
  const double *partners = ens + (size_t)((1 - h) * H) * SD;
  for (int k = lane; k < H; k += lanes) {
    const int w = h * H + k;
    double *st = ens + (size_t)w * SD;
    uint32_t r[4];
    cm_philox(run, (uint32_t)t, (uint32_t)w, 0u, a.seed_lo, a.seed_hi, r);
    const double w1 = cm_uniform(r[0], r[1]), w2 = cm_uniform(r[2], r[3]);
    int ia = (int)(w1 * (double)H);
    ia = ia > H - 1 ? H - 1 : ia;
    double ut[N];
    double lq = 0.0;
    if (a.move == IONODE_ENSEMBLE_STRETCH) {
      const double *pj = partners + (size_t)ia * SD + OU;
      const double s = (a.a - 1.0) * w2 + 1.0;
      const double z = (s * s) / a.a;
#pragma unroll
      for (int j = 0; j < N; ++j) {
        const double uj = pj[j];
        ut[j] = uj + z * (st[OU + j] - uj);
      }
      lq = (double)(N - 1) * cm_log(z);
    } else {
      int off = (int)(w2 * (double)(H - 1));
      off = off > H - 2 ? H - 2 : off;
      int ib = ia + 1 + off;
      ib = ib >= H ? ib - H : ib;
      const double *pa = partners + (size_t)ia * SD + OU, *pb = partners + (size_t)ib * SD + OU;
#pragma unroll
      for (int jp = 0; jp < (N + 1) / 2; ++jp) {
        double z0, z1;
        cm_normal_pair(a.seed_lo, a.seed_hi, (int)run, t, w, jp, 2, z0, z1);
        ut[2 * jp] = (st[OU + 2 * jp] + a.gamma * (pa[2 * jp] - pb[2 * jp])) + a.jitter * z0;
        if (2 * jp + 1 < N) ut[2 * jp + 1] = (st[OU + 2 * jp + 1] + a.gamma * (pa[2 * jp + 1] - pb[2 * jp + 1])) + a.jitter * z1;
      }
    }
    bool inside = true;
#pragma unroll
    for (int j = 0; j < N; ++j) inside = inside && ut[j] >= a.ulo[j] && ut[j] <= a.uhi[j];
    double xt[N];
#pragma unroll
    for (int j = 0; j < N; ++j) {
      double x = st[OX + j];   // outside: the rows repeat the current point, its solve is wasted and its tell rejects
      if (inside) {
        x = (a.log_p || (a.ss && j == N - 1)) ? lm_exp(ut[j]) : ut[j];
        x = x < a.xlo[j] ? a.xlo[j] : x;
        x = x > a.xhi[j] ? a.xhi[j] : x;
      }
      xt[j] = x;
      st[OUT + j] = ut[j];
      st[OXT + j] = x;
    }
    st[IONODE_ENSEMBLE_STATE_LQ] = lq;
    st[IONODE_ENSEMBLE_STATE_OUTSIDE] = inside ? 0.0 : 1.0;
    en_write_trial<N>(a, e * H + k, xt);
  }
}

template <int N>
__global__ void __launch_bounds__(kEnLanes) ionode_ensemble_step_kernel(const EnArgs a) {
  __shared__ int bad;
  en_ensemble<N>(a, (int)blockIdx.x, (int)threadIdx.x, kEnLanes, &bad);
}

// inst_ensemble.hip
void launch_ensemble_step(const EnArgs &a, hipStream_t s);
void ensemble_step_host(const EnArgs &a);

}  // namespace ionode
