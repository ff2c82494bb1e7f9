// ionode_step_capi.hpp -- host only: what the entry points of the optimiser steps (ionode_lm_capi.hip, ionode_cmaes_capi.hip,
// ionode_mcmc_capi.hip, ionode_mala_capi.hip, ionode_ensemble_capi.hip) share.  The refusal that sets ionode_grad_last_error(), the checks and the box every step descriptor carries
// (n_free, n_params, free_idx, lo, hi, base, log_parameters), the seed split and the launch's tail.
#pragma once

#include <cmath>
#include <cstring>

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ionode.h"

namespace ionode {

// ionode_grad_capi.hip, next to the thread-local buffer it writes: sets ionode_grad_last_error(), returns rc
__attribute__((format(printf, 2, 3))) int refuse(int rc, const char *fmt, ...);

// The shared part of a step's checks, in the order every step refuses in: the descriptor, the buffers (`buffers`: all there; `names`
// lists them in the message), n_free; then the step's own rules (`rules()`: IONODE_OK or its refusal); then, free parameter by free
// parameter, the index, lo <= hi, the step's own rule about a bound (`bound_rule(j)`) and positive bounds under log_parameters.  `a` is
// zeroed and its free_idx / xlo / xhi / ulo / uhi / base are filled: the bounds' logarithms are taken here, on the host, for the kernel
// and the mirror alike.
template <class Desc, class Args, class Rules, class BoundRule>
int step_box(const char *who, const Desc *d, bool buffers, const char *names, Args &a, Rules rules, BoundRule bound_rule) {
  if (!d) return refuse(IONODE_ERR_ARG, "%s: null descriptor", who);
  if (!buffers) return refuse(IONODE_ERR_ARG, "%s: required buffer is NULL (%s)", who, names);
  if (d->n_free < 1 || d->n_free > IONODE_LM_MAX_FREE) return refuse(IONODE_ERR_ARG, "%s: n_free = %d outside 1 .. %d", who, (int)d->n_free, IONODE_LM_MAX_FREE);
  if (const int rc = rules()) return rc;
  const bool lg = d->log_parameters != 0;
  memset(&a, 0, sizeof a);
  for (int j = 0; j < d->n_free; ++j) {
    if (d->free_idx[j] < 0 || d->free_idx[j] >= d->n_params)
      return refuse(IONODE_ERR_ARG, "%s: free index %d outside the model's %d parameters", who, (int)d->free_idx[j], (int)d->n_params);
    if (!(d->lo[j] <= d->hi[j])) return refuse(IONODE_ERR_ARG, "%s: bounds of free parameter %d: lo > hi (or NaN)", who, j);
    if (const int rc = bound_rule(j)) return rc;
    if (lg && !(d->lo[j] > 0.0)) return refuse(IONODE_ERR_ARG, "%s: log_parameters needs positive bounds (free parameter %d)", who, j);
    a.free_idx[j] = d->free_idx[j];
    a.xlo[j] = d->lo[j];
    a.xhi[j] = d->hi[j];
    a.ulo[j] = lg ? std::log(d->lo[j]) : d->lo[j];
    a.uhi[j] = lg ? std::log(d->hi[j]) : d->hi[j];
  }
  for (int i = 0; i < d->n_params; ++i) a.base[i] = d->base[i];
  return IONODE_OK;
}
inline int no_bound_rule(int) { return IONODE_OK; }

// the n_params rule of the steps that serve every model
inline int step_n_params(const char *who, int n_params) {
  if (n_params < 1 || n_params > IONODE_LM_MAX_FREE)
    return refuse(IONODE_ERR_ARG, "%s: n_params = %d outside 1 .. %d", who, n_params, IONODE_LM_MAX_FREE);
  return IONODE_OK;
}

// the generator's key: the two halves of the descriptor's seed
inline void step_seed(int64_t seed, uint32_t &lo, uint32_t &hi) {
  lo = (uint32_t)((uint64_t)seed & 0xFFFFFFFFull);
  hi = (uint32_t)((uint64_t)seed >> 32);
}

// after a launch: HIP's pending error, refused under the entry's name
inline int step_launched(const char *who) {
  const hipError_t err = hipGetLastError();
  if (err != hipSuccess) return refuse(IONODE_ERR_LAUNCH, "%s: %s", who, hipGetErrorString(err));
  return IONODE_OK;
}

}  // namespace ionode
