// ionode_mala_capi.hip -- C ABI of the manifold-MALA step (include/ionode.h "Manifold MALA step"): the checks, the descriptor turned
// into the routine's by-value arguments (the box's logarithms are formed here, on the host, for the kernel and the mirror alike), the
// launch and the host mirror.  A unit of its own: the other units compile to what they did.
#include <cmath>

#include "ionode_mala.hpp"
#include "ionode_step_capi.hpp"

namespace {

using ionode::refuse;

int mala_args(const char *who, const ionode_mala_desc *d, const int32_t *active, const double *sse, const double *jtr, const double *jtj,
              const int32_t *status, double *state, int32_t *flag, int32_t *iters, double *trial, double *samples, ionode::MaArgs &a) {
  const double inf = __builtin_inf();
  const int rc = ionode::step_box(
      who, d, sse && jtr && jtj && status && state && flag && iters && trial, "sse, jtr, jtj, status, state, flag, iters, trial", a,
      [&] {
        if (const int r = ionode::step_n_params(who, d->n_params)) return r;
        if (d->n_chain < 1 || d->n_active < 1 || d->n_active > d->n_chain || d->n_prot < 1 || d->max_iter < 1)
          return refuse(IONODE_ERR_ARG, "%s: n_chain, n_active <= n_chain, n_prot and max_iter must be positive", who);
        if (d->thin < 1) return refuse(IONODE_ERR_ARG, "%s: thin = %d < 1", who, (int)d->thin);
        if (!(d->eta > 0.5 && d->eta <= 1.0)) return refuse(IONODE_ERR_ARG, "%s: eta = %g outside (0.5, 1]", who, d->eta);
        if (!(d->target_accept > 0.0 && d->target_accept < 1.0)) return refuse(IONODE_ERR_ARG, "%s: target_accept = %g outside (0, 1)", who, d->target_accept);
        if (!(d->ridge >= 0.0) || d->ridge == inf) return refuse(IONODE_ERR_ARG, "%s: ridge = %g must be a finite number >= 0", who, d->ridge);
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
  a.K = d->n_chain; a.n_active = d->n_active; a.P = d->n_prot; a.NPAR = d->n_params; a.nf = d->n_free; a.n = d->n_free + (ss ? 1 : 0);
  a.log_p = lg ? 1 : 0; a.ss = ss ? 1 : 0; a.max_iter = d->max_iter; a.thin = d->thin;
  a.sample_cap = d->sample_cap; a.chain_base = d->chain_base;
  ionode::step_seed(d->seed, a.seed_lo, a.seed_hi);
  a.n_samples = d->n_samples; a.eta = d->eta; a.target_accept = d->target_accept; a.ridge = d->ridge;
  a.active = active; a.sse = sse; a.jtr = jtr; a.jtj = jtj; a.status = status;
  a.state = state; a.flag = flag; a.iters = iters; a.trial = trial; a.samples = samples;
  return IONODE_OK;
}

}  // namespace

extern "C" {

int ionode_mala_step(const ionode_mala_desc *d, const int32_t *active, const double *sse, const double *jtr, const double *jtj,
                     const int32_t *status, double *state, int32_t *flag, int32_t *iters, double *trial, double *samples, void *stream) {
  ionode::MaArgs a;
  const int rc = mala_args("ionode_mala_step", d, active, sse, jtr, jtj, status, state, flag, iters, trial, samples, a);
  if (rc != IONODE_OK) return rc;
  ionode::launch_mala_step(a, reinterpret_cast<hipStream_t>(stream));
  return ionode::step_launched("ionode_mala_step");
}

int ionode_mala_step_host(const ionode_mala_desc *d, const int32_t *active, const double *sse, const double *jtr, const double *jtj,
                          const int32_t *status, double *state, int32_t *flag, int32_t *iters, double *trial, double *samples) {
  ionode::MaArgs a;
  const int rc = mala_args("ionode_mala_step_host", d, active, sse, jtr, jtj, status, state, flag, iters, trial, samples, a);
  if (rc != IONODE_OK) return rc;
  ionode::mala_step_host(a);
  return IONODE_OK;
}

}  // extern "C"
