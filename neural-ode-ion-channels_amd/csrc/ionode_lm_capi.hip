// ionode_lm_capi.hip -- C ABI of the Levenberg-Marquardt step (include/ionode.h "Levenberg-Marquardt step"): the checks, the
// descriptor turned into the routine's by-value arguments, the launch and the host mirror.  A unit of its own: the gradient path's
// unit compiles to what it did.
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>

#include "ionode_lm.hpp"

namespace {

// The message goes where the gradient path's go: ionode_grad_last_error() hands out that unit's thread-local buffer (256 bytes,
// ionode_grad_capi.hip g_gerr), which is an ordinary writable array.
constexpr size_t kGradErrBytes = 256;
__attribute__((format(printf, 2, 3))) int refuse(int rc, const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(const_cast<char *>(ionode_grad_last_error()), kGradErrBytes, fmt, ap);
  va_end(ap);
  return rc;
}

// Every refusal of both entry points, and the arguments of the routine.  The bounds' logarithms are taken here, on the host, for
// the kernel and the mirror alike.
int lm_args(const char *who, const ionode_lm_desc *d, const int32_t *active, const double *sse, const double *jtr, const double *jtj,
            const int32_t *status, double *state, int32_t *flag, int32_t *iters, double *trial, ionode::LmArgs &a) {
  if (!d) return refuse(IONODE_ERR_ARG, "%s: null descriptor", who);
  if (!sse || !jtr || !jtj || !status || !state || !flag || !iters || !trial)
    return refuse(IONODE_ERR_ARG, "%s: required buffer is NULL (sse, jtr, jtj, status, state, flag, iters, trial)", who);
  if (d->n_free < 1 || d->n_free > IONODE_LM_MAX_FREE) return refuse(IONODE_ERR_ARG, "%s: n_free = %d outside 1 .. %d", who, (int)d->n_free, IONODE_LM_MAX_FREE);
  if (d->n_params != 8 && d->n_params != 12) return refuse(IONODE_ERR_ARG, "%s: n_params must be 8 (HH 2-state) or 12 (6-state)", who);
  if (d->n_cand < 1 || d->n_active < 1 || d->n_active > d->n_cand || d->n_prot < 1 || d->max_iter < 1)
    return refuse(IONODE_ERR_ARG, "%s: n_cand, n_active <= n_cand, n_prot and max_iter must be positive", who);
  const bool lg = d->log_parameters != 0;
  memset(&a, 0, sizeof a);
  for (int j = 0; j < d->n_free; ++j) {
    if (d->free_idx[j] < 0 || d->free_idx[j] >= d->n_params)
      return refuse(IONODE_ERR_ARG, "%s: free index %d outside the model's %d parameters", who, (int)d->free_idx[j], (int)d->n_params);
    if (!(d->lo[j] <= d->hi[j])) return refuse(IONODE_ERR_ARG, "%s: bounds of free parameter %d: lo > hi (or NaN)", who, j);
    if (lg && !(d->lo[j] > 0.0)) return refuse(IONODE_ERR_ARG, "%s: log_parameters needs positive bounds (free parameter %d)", who, j);
    a.free_idx[j] = d->free_idx[j];
    a.xlo[j] = d->lo[j];
    a.xhi[j] = d->hi[j];
    a.ulo[j] = lg ? std::log(d->lo[j]) : d->lo[j];
    a.uhi[j] = lg ? std::log(d->hi[j]) : d->hi[j];
  }
  for (int i = 0; i < d->n_params; ++i) a.base[i] = d->base[i];
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
  const hipError_t err = hipGetLastError();
  if (err != hipSuccess) return refuse(IONODE_ERR_LAUNCH, "ionode_lm_step: %s", hipGetErrorString(err));
  return IONODE_OK;
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
