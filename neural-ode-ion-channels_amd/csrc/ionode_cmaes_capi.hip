// ionode_cmaes_capi.hip -- C ABI of the CMA-ES step (include/ionode.h "CMA-ES step"): the checks, the descriptor turned into the
// phases' by-value arguments (the box's logarithms and the strategy constants are formed here, on the host, for the kernel and the
// mirror alike), the launch and the host mirror.  A unit of its own: the other units compile to what they did.
#include <cmath>

#include "ionode_cmaes.hpp"
#include "ionode_step_capi.hpp"

namespace {

using ionode::refuse;

int cmaes_args(const char *who, const ionode_cmaes_desc *d, const int32_t *active, const double *value, const int32_t *status, double *state,
               int32_t *flag, int32_t *iters, double *trial, ionode::CmArgs &a) {
  using ionode::cm_log;
  const int rc = ionode::step_box(
      who, d, value && status && state && flag && iters && trial, "value, status, state, flag, iters, trial", a,
      [&] {
        if (d->lambda < 2 || d->lambda > IONODE_CMAES_MAX_LAMBDA)
          return refuse(IONODE_ERR_ARG, "%s: lambda = %d outside 2 .. %d", who, (int)d->lambda, IONODE_CMAES_MAX_LAMBDA);
        if (const int r = ionode::step_n_params(who, d->n_params)) return r;
        if (d->n_run < 1 || d->n_active < 1 || d->n_active > d->n_run || d->n_prot < 1 || d->max_iter < 1 || d->unchanged_iters < 1)
          return refuse(IONODE_ERR_ARG, "%s: n_run, n_active <= n_run, n_prot, max_iter and unchanged_iters must be positive", who);
        return IONODE_OK;
      },
      ionode::no_bound_rule);
  if (rc != IONODE_OK) return rc;
  const bool lg = d->log_parameters != 0;
  a.K = d->n_run; a.n_active = d->n_active; a.lam = d->lambda; a.mu = d->lambda / 2; a.P = d->n_prot; a.NPAR = d->n_params;
  a.n = d->n_free; a.log_p = lg ? 1 : 0; a.max_iter = d->max_iter; a.unchanged_iters = d->unchanged_iters; a.run_base = d->run_base;
  a.unchanged_threshold = d->unchanged_threshold; a.tolx = d->tolx;
  ionode::step_seed(d->seed, a.seed_lo, a.seed_hi);
  // the strategy constants (ionode_cmaes.hpp's head), sums in index order
  const double n = (double)a.n;
  a.ln_mu_half = cm_log((double)a.mu + 0.5);
  double sw = 0.0;
  for (int i = 1; i <= a.mu; ++i) sw = sw + (a.ln_mu_half - cm_log((double)i));
  a.sum_w = sw;
  double s2 = 0.0;
  for (int i = 1; i <= a.mu; ++i) {
    const double w = (a.ln_mu_half - cm_log((double)i)) / sw;
    s2 = s2 + w * w;
  }
  a.mu_eff = 1.0 / s2;
  a.cs = (a.mu_eff + 2.0) / (n + a.mu_eff + 5.0);
  const double root = std::sqrt((a.mu_eff - 1.0) / (n + 1.0)) - 1.0;
  a.ds = 1.0 + 2.0 * (root > 0.0 ? root : 0.0) + a.cs;
  a.cc = (4.0 + a.mu_eff / n) / (n + 4.0 + 2.0 * a.mu_eff / n);
  a.c1 = 2.0 / ((n + 1.3) * (n + 1.3) + a.mu_eff);
  const double cmu = 2.0 * (a.mu_eff - 2.0 + 1.0 / a.mu_eff) / ((n + 2.0) * (n + 2.0) + a.mu_eff);
  a.cmu = cmu < 1.0 - a.c1 ? cmu : 1.0 - a.c1;
  a.chi_n = std::sqrt(n) * (1.0 - 1.0 / (4.0 * n) + 1.0 / (21.0 * n * n));
  a.ln_1mcs = cm_log(1.0 - a.cs);
  a.active = active; a.value = value; a.status = status;
  a.state = state; a.flag = flag; a.iters = iters; a.trial = trial;
  return IONODE_OK;
}

}  // namespace

extern "C" {

int ionode_cmaes_step(const ionode_cmaes_desc *d, const int32_t *active, const double *value, const int32_t *status, double *state,
                      int32_t *flag, int32_t *iters, double *trial, void *stream) {
  ionode::CmArgs a;
  const int rc = cmaes_args("ionode_cmaes_step", d, active, value, status, state, flag, iters, trial, a);
  if (rc != IONODE_OK) return rc;
  ionode::launch_cmaes_step(a, reinterpret_cast<hipStream_t>(stream));
  return ionode::step_launched("ionode_cmaes_step");
}

int ionode_cmaes_step_host(const ionode_cmaes_desc *d, const int32_t *active, const double *value, const int32_t *status, double *state,
                           int32_t *flag, int32_t *iters, double *trial) {
  ionode::CmArgs a;
  const int rc = cmaes_args("ionode_cmaes_step_host", d, active, value, status, state, flag, iters, trial, a);
  if (rc != IONODE_OK) return rc;
  ionode::cmaes_step_host(a);
  return IONODE_OK;
}

void ionode_cmaes_draw_host(int64_t seed, int32_t run, int32_t generation, int32_t candidate, int32_t pair, int32_t attempt,
                            uint32_t words[4], double z[2]) {
  uint32_t lo, hi;
  ionode::step_seed(seed, lo, hi);
  uint32_t w[4];
  ionode::cm_philox((uint32_t)run, (uint32_t)generation, (uint32_t)candidate, (uint32_t)pair + 65536u * (uint32_t)attempt, lo, hi, w);
  for (int i = 0; i < 4; ++i) words[i] = w[i];
  ionode::cm_normal_pair(lo, hi, run, generation, candidate, pair, attempt, z[0], z[1]);
}

double ionode_cmaes_log_host(double x) { return ionode::cm_log(x); }

}  // extern "C"
