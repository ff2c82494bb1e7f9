// ionode_mcmc_capi.hip -- C ABI of the adaptive-Metropolis step (include/ionode.h "Adaptive Metropolis step"): the checks, the
// descriptor turned into the routine's by-value arguments (the box's logarithms are formed here, on the host, for the kernel and the
// mirror alike), the launch and the host mirror.  A unit of its own: the other units compile to what they did.
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>

#include "ionode_mcmc.hpp"

namespace {

// The message goes where the gradient path's and the other steps' go (ionode_lm_capi.hip refuse()).
constexpr size_t kGradErrBytes = 256;
__attribute__((format(printf, 2, 3))) int refuse(int rc, const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(const_cast<char *>(ionode_grad_last_error()), kGradErrBytes, fmt, ap);
  va_end(ap);
  return rc;
}

int mcmc_args(const char *who, const ionode_mcmc_desc *d, const int32_t *active, const double *value, const int32_t *status, double *state,
              int32_t *flag, int32_t *iters, double *trial, double *samples, ionode::McArgs &a) {
  if (!d) return refuse(IONODE_ERR_ARG, "%s: null descriptor", who);
  if (!value || !status || !state || !flag || !iters || !trial)
    return refuse(IONODE_ERR_ARG, "%s: required buffer is NULL (value, status, state, flag, iters, trial)", who);
  if (d->n_free < 1 || d->n_free > IONODE_LM_MAX_FREE) return refuse(IONODE_ERR_ARG, "%s: n_free = %d outside 1 .. %d", who, (int)d->n_free, IONODE_LM_MAX_FREE);
  if (d->n_params < 1 || d->n_params > IONODE_LM_MAX_FREE)
    return refuse(IONODE_ERR_ARG, "%s: n_params = %d outside 1 .. %d", who, (int)d->n_params, IONODE_LM_MAX_FREE);
  if (d->n_chain < 1 || d->n_active < 1 || d->n_active > d->n_chain || d->n_prot < 1 || d->max_iter < 1)
    return refuse(IONODE_ERR_ARG, "%s: n_chain, n_active <= n_chain, n_prot and max_iter must be positive", who);
  if (d->thin < 1) return refuse(IONODE_ERR_ARG, "%s: thin = %d < 1", who, (int)d->thin);
  if (!(d->eta > 0.5 && d->eta <= 1.0)) return refuse(IONODE_ERR_ARG, "%s: eta = %g outside (0.5, 1]", who, d->eta);
  if (!(d->target_accept > 0.0 && d->target_accept < 1.0)) return refuse(IONODE_ERR_ARG, "%s: target_accept = %g outside (0, 1)", who, d->target_accept);
  const bool lg = d->log_parameters != 0, ss = d->sample_sigma != 0;
  const double inf = __builtin_inf();
  memset(&a, 0, sizeof a);
  for (int j = 0; j < d->n_free; ++j) {
    if (d->free_idx[j] < 0 || d->free_idx[j] >= d->n_params)
      return refuse(IONODE_ERR_ARG, "%s: free index %d outside the model's %d parameters", who, (int)d->free_idx[j], (int)d->n_params);
    if (!(d->lo[j] <= d->hi[j])) return refuse(IONODE_ERR_ARG, "%s: bounds of free parameter %d: lo > hi (or NaN)", who, j);
    if (d->lo[j] == -inf || d->hi[j] == inf)
      return refuse(IONODE_ERR_ARG, "%s: infinite bound of free parameter %d (the box is the prior: it must be finite)", who, j);
    if (lg && !(d->lo[j] > 0.0)) return refuse(IONODE_ERR_ARG, "%s: log_parameters needs positive bounds (free parameter %d)", who, j);
    a.free_idx[j] = d->free_idx[j];
    a.xlo[j] = d->lo[j];
    a.xhi[j] = d->hi[j];
    a.ulo[j] = lg ? std::log(d->lo[j]) : d->lo[j];
    a.uhi[j] = lg ? std::log(d->hi[j]) : d->hi[j];
  }
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
  for (int i = 0; i < d->n_params; ++i) a.base[i] = d->base[i];
  a.K = d->n_chain; a.n_active = d->n_active; a.P = d->n_prot; a.NPAR = d->n_params; a.nf = d->n_free; a.n = d->n_free + (ss ? 1 : 0);
  a.log_p = lg ? 1 : 0; a.ss = ss ? 1 : 0; a.max_iter = d->max_iter; a.adapt_start = d->adapt_start; a.thin = d->thin;
  a.sample_cap = d->sample_cap; a.chain_base = d->chain_base;
  a.seed_lo = (uint32_t)((uint64_t)d->seed & 0xFFFFFFFFull); a.seed_hi = (uint32_t)((uint64_t)d->seed >> 32);
  a.n_samples = d->n_samples; a.eta = d->eta; a.target_accept = d->target_accept; a.epsilon = d->epsilon;
  a.active = active; a.value = value; a.status = status;
  a.state = state; a.flag = flag; a.iters = iters; a.trial = trial; a.samples = samples;
  return IONODE_OK;
}

}  // namespace

extern "C" {

int ionode_mcmc_step(const ionode_mcmc_desc *d, const int32_t *active, const double *value, const int32_t *status, double *state,
                     int32_t *flag, int32_t *iters, double *trial, double *samples, void *stream) {
  ionode::McArgs a;
  const int rc = mcmc_args("ionode_mcmc_step", d, active, value, status, state, flag, iters, trial, samples, a);
  if (rc != IONODE_OK) return rc;
  ionode::launch_mcmc_step(a, reinterpret_cast<hipStream_t>(stream));
  const hipError_t err = hipGetLastError();
  if (err != hipSuccess) return refuse(IONODE_ERR_LAUNCH, "ionode_mcmc_step: %s", hipGetErrorString(err));
  return IONODE_OK;
}

int ionode_mcmc_step_host(const ionode_mcmc_desc *d, const int32_t *active, const double *value, const int32_t *status, double *state,
                          int32_t *flag, int32_t *iters, double *trial, double *samples) {
  ionode::McArgs a;
  const int rc = mcmc_args("ionode_mcmc_step_host", d, active, value, status, state, flag, iters, trial, samples, a);
  if (rc != IONODE_OK) return rc;
  ionode::mcmc_step_host(a);
  return IONODE_OK;
}

}  // extern "C"
