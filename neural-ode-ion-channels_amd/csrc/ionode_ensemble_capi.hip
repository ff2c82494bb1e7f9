// ionode_ensemble_capi.hip -- C ABI of the affine-invariant ensemble step (include/ionode.h "Affine-invariant ensemble step"): the
// checks, the descriptor turned into the routine's by-value arguments (the box's logarithms are formed here, on the host, for the
// kernel and the mirror alike), the launch and the host mirror.  A unit of its own: the other units compile to what they did.
#include <cmath>

#include "ionode_ensemble.hpp"
#include "ionode_step_capi.hpp"

namespace {

using ionode::refuse;

int ensemble_args(const char *who, const ionode_ensemble_desc *d, const double *value, const int32_t *status, double *state, int32_t *flag,
                  int32_t *iters, int32_t *accepted, double *trial, double *samples, ionode::EnArgs &a) {
  const double inf = __builtin_inf();
  const int rc = ionode::step_box(
      who, d, value && status && state && flag && iters && accepted && trial, "value, status, state, flag, iters, accepted, trial", a,
      [&] {
        if (const int r = ionode::step_n_params(who, d->n_params)) return r;
        if (d->n_ens < 1 || d->n_prot < 1 || d->max_iter < 1) return refuse(IONODE_ERR_ARG, "%s: n_ens, n_prot and max_iter must be positive", who);
        if (d->max_iter > (1 << 30) - 1) return refuse(IONODE_ERR_ARG, "%s: max_iter = %d above 2^30 - 1 (the counter counts half-iterations)", who, (int)d->max_iter);
        if (d->thin < 1) return refuse(IONODE_ERR_ARG, "%s: thin = %d < 1", who, (int)d->thin);
        if (d->sample_cap < 0) return refuse(IONODE_ERR_ARG, "%s: sample_cap = %d < 0", who, (int)d->sample_cap);
        if (d->move != IONODE_ENSEMBLE_STRETCH && d->move != IONODE_ENSEMBLE_DE) return refuse(IONODE_ERR_ARG, "%s: unknown move %d", who, (int)d->move);
        const int n = d->n_free + (d->sample_sigma != 0 ? 1 : 0), W = d->n_walkers;
        if (W < 0 || W % 2 != 0) return refuse(IONODE_ERR_ARG, "%s: n_walkers = %d is odd (or negative): the walkers move as two halves", who, W);
        if (W > IONODE_ENSEMBLE_MAX_WALKERS) return refuse(IONODE_ERR_ARG, "%s: n_walkers = %d above %d", who, W, IONODE_ENSEMBLE_MAX_WALKERS);
        if (d->move == IONODE_ENSEMBLE_DE && W / 2 < 2) return refuse(IONODE_ERR_ARG, "%s: the DE move needs two partners: n_walkers >= 4", who);
        if (W < 2 * (n + 1))
          return refuse(IONODE_ERR_ARG, "%s: n_walkers = %d < 2 (n + 1) = %d: a half must affinely span the %d coordinates", who, W, 2 * (n + 1), n);
        if ((int64_t)d->n_ens * W * d->n_prot > 2147483647ll) return refuse(IONODE_ERR_ARG, "%s: n_ens n_walkers n_prot beyond 2^31 - 1 rows", who);
        if (!(d->a > 1.0) || d->a == inf) return refuse(IONODE_ERR_ARG, "%s: a = %g: the stretch scale must be above 1 and finite", who, d->a);
        if (!std::isfinite(d->gamma)) return refuse(IONODE_ERR_ARG, "%s: gamma = %g is not finite", who, d->gamma);
        if (!(d->jitter >= 0.0) || d->jitter == inf) return refuse(IONODE_ERR_ARG, "%s: jitter = %g must be finite and not negative", who, d->jitter);
        if (!(d->n_samples > 0.0) || d->n_samples == inf) return refuse(IONODE_ERR_ARG, "%s: n_samples = %g must be positive and finite", who, d->n_samples);
        return IONODE_OK;
      },
      [&](int j) {
        if (d->lo[j] == -inf || d->hi[j] == inf)
          return refuse(IONODE_ERR_ARG, "%s: infinite bound of free parameter %d (the box is the prior: it must be finite)", who, j);
        return IONODE_OK;
      });
  if (rc != IONODE_OK) return rc;
  const bool lg = d->log_parameters != 0, ss = d->sample_sigma != 0;
  if (ss) {
    if (!(d->sigma_lo > 0.0) || !(d->sigma_lo <= d->sigma_hi) || d->sigma_hi == inf)
      return refuse(IONODE_ERR_ARG, "%s: sample_sigma needs 0 < sigma_lo <= sigma_hi < inf", who);
    a.xlo[d->n_free] = d->sigma_lo;
    a.xhi[d->n_free] = d->sigma_hi;
    a.ulo[d->n_free] = std::log(d->sigma_lo);
    a.uhi[d->n_free] = std::log(d->sigma_hi);
  } else {
    if (!(d->sigma > 0.0) || d->sigma == inf) return refuse(IONODE_ERR_ARG, "%s: a fixed sigma must be positive and finite", who);
    a.log_sigma = std::log(d->sigma);
  }
  a.E = d->n_ens; a.W = d->n_walkers; a.H = d->n_walkers / 2; a.P = d->n_prot; a.NPAR = d->n_params; a.nf = d->n_free;
  a.n = d->n_free + (ss ? 1 : 0); a.log_p = lg ? 1 : 0; a.ss = ss ? 1 : 0; a.max_iter = d->max_iter; a.thin = d->thin;
  a.sample_cap = d->sample_cap; a.ensemble_base = d->ensemble_base; a.move = d->move;
  ionode::step_seed(d->seed, a.seed_lo, a.seed_hi);
  a.n_samples = d->n_samples; a.a = d->a; a.gamma = d->gamma; a.jitter = d->jitter;
  a.value = value; a.status = status; a.state = state; a.flag = flag; a.iters = iters; a.accepted = accepted; a.trial = trial; a.samples = samples;
  return IONODE_OK;
}

}  // namespace

extern "C" {

int ionode_ensemble_step(const ionode_ensemble_desc *d, const double *value, const int32_t *status, double *state, int32_t *flag,
                         int32_t *iters, int32_t *accepted, double *trial, double *samples, void *stream) {
  ionode::EnArgs a;
  const int rc = ensemble_args("ionode_ensemble_step", d, value, status, state, flag, iters, accepted, trial, samples, a);
  if (rc != IONODE_OK) return rc;
  ionode::launch_ensemble_step(a, reinterpret_cast<hipStream_t>(stream));
  return ionode::step_launched("ionode_ensemble_step");
}

int ionode_ensemble_step_host(const ionode_ensemble_desc *d, const double *value, const int32_t *status, double *state, int32_t *flag,
                              int32_t *iters, int32_t *accepted, double *trial, double *samples) {
  ionode::EnArgs a;
  const int rc = ensemble_args("ionode_ensemble_step_host", d, value, status, state, flag, iters, accepted, trial, samples, a);
  if (rc != IONODE_OK) return rc;
  ionode::ensemble_step_host(a);
  return IONODE_OK;
}

}  // extern "C"
