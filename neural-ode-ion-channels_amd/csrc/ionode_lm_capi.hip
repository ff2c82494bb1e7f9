// ionode_lm_capi.hip -- C ABI of the Levenberg-Marquardt step (include/ionode.h "Levenberg-Marquardt step"): the checks, the
// descriptor turned into the routine's by-value arguments, the launch and the host mirror.  A unit of its own: the gradient path's
// unit compiles to what it did.
#include <cmath>

#include "ionode_lm.hpp"
#include "ionode_step_capi.hpp"

namespace {

using ionode::refuse;

// Every refusal of both entry points, and the arguments of the routine (the shared checks and the box: ionode_step_capi.hpp).
int lm_args(const char *who, const ionode_lm_desc *d, const int32_t *active, const double *sse, const double *jtr, const double *jtj,
            const int32_t *status, double *state, int32_t *flag, int32_t *iters, double *trial, ionode::LmArgs &a) {
  const int rc = ionode::step_box(
      who, d, sse && jtr && jtj && status && state && flag && iters && trial, "sse, jtr, jtj, status, state, flag, iters, trial", a,
      [&] {
        if (d->n_params != 8 && d->n_params != 12) return refuse(IONODE_ERR_ARG, "%s: n_params must be 8 (HH 2-state) or 12 (6-state)", who);
        if (d->n_cand < 1 || d->n_active < 1 || d->n_active > d->n_cand || d->n_prot < 1 || d->max_iter < 1)
          return refuse(IONODE_ERR_ARG, "%s: n_cand, n_active <= n_cand, n_prot and max_iter must be positive", who);
        return IONODE_OK;
      },
      ionode::no_bound_rule);
  if (rc != IONODE_OK) return rc;
  const bool lg = d->log_parameters != 0;
  a.C = d->n_cand; a.n_active = d->n_active; a.P = d->n_prot; a.NPAR = d->n_params; a.nf = d->n_free; a.log_p = lg ? 1 : 0;
  a.max_iter = d->max_iter;
  a.gtol = d->gtol; a.xtol = d->xtol; a.ftol = d->ftol; a.rho_accept = d->rho_accept; a.lam_max = d->lam_max;
  a.active = active; a.sse = sse; a.jtr = jtr; a.jtj = jtj; a.status = status;
  a.state = state; a.flag = flag; a.iters = iters; a.trial = trial;
  return IONODE_OK;
}

}  // namespace

extern "C" {

int ionode_lm_step(const ionode_lm_desc *d, const int32_t *active, const double *sse, const double *jtr, const double *jtj,
                   const int32_t *status, double *state, int32_t *flag, int32_t *iters, double *trial, void *stream) {
  ionode::LmArgs a;
  const int rc = lm_args("ionode_lm_step", d, active, sse, jtr, jtj, status, state, flag, iters, trial, a);
  if (rc != IONODE_OK) return rc;
  ionode::launch_lm_step(a, reinterpret_cast<hipStream_t>(stream));
  return ionode::step_launched("ionode_lm_step");
}

int ionode_lm_step_host(const ionode_lm_desc *d, const int32_t *active, const double *sse, const double *jtr, const double *jtj,
                        const int32_t *status, double *state, int32_t *flag, int32_t *iters, double *trial) {
  ionode::LmArgs a;
  const int rc = lm_args("ionode_lm_step_host", d, active, sse, jtr, jtj, status, state, flag, iters, trial, a);
  if (rc != IONODE_OK) return rc;
  ionode::lm_step_host(a);
  return IONODE_OK;
}

}  // extern "C"
