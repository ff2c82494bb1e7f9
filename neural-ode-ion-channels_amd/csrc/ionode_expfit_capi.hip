// ionode_expfit_capi.hip -- C ABI of the multi-exponential fit objective and evaluation (include/ionode.h "Multi-exponential fits"):
// the checks, the launches and the host mirrors.  A unit of its own: the other units compile to what they did.
#include "ionode_expfit.hpp"
#include "ionode_step_capi.hpp"

namespace {

using ionode::refuse;

int n_params_rule(const char *who, int n_params) {
  if (n_params != 5 && n_params != 7)
    return refuse(IONODE_ERR_ARG, "%s: n_params = %d: 5 (bi-exponential) or 7 (tri-exponential)", who, n_params);
  return IONODE_OK;
}

int objective_args(const char *who, int32_t n_run, int32_t n_active, int32_t lambda, int32_t n_params, const int32_t *active,
                   const int32_t *seg_of_run, const int64_t *seg_off, const double *t_rel, const double *a, const double *trial, double *value,
                   int32_t *status, ionode::EfArgs &g) {
  if (!(seg_of_run && seg_off && t_rel && a && trial && value && status))
    return refuse(IONODE_ERR_ARG, "%s: required buffer is NULL (seg_of_run, seg_off, t_rel, a, trial, value, status)", who);
  if (const int rc = n_params_rule(who, n_params)) return rc;
  if (lambda < 2 || lambda > IONODE_CMAES_MAX_LAMBDA)
    return refuse(IONODE_ERR_ARG, "%s: lambda = %d outside 2 .. %d", who, (int)lambda, IONODE_CMAES_MAX_LAMBDA);
  if (n_run < 1 || n_active < 1 || n_active > n_run) return refuse(IONODE_ERR_ARG, "%s: n_run and n_active <= n_run must be positive", who);
  if ((int64_t)n_active * lambda > INT32_MAX)
    return refuse(IONODE_ERR_ARG, "%s: n_active * lambda = %lld rows exceed one launch's %d", who, (long long)n_active * lambda, INT32_MAX);
  g = ionode::EfArgs{n_run, n_active, lambda, n_params, active, seg_of_run, seg_off, t_rel, a, trial, value, status};
  return IONODE_OK;
}

int eval_args(const char *who, int32_t n_seg, int32_t n_params, const double *x, const int64_t *full_off, const double *t_full, double *a_fit,
              double *dadt, double *d2adt2, ionode::EfEvalArgs &g) {
  if (!(x && full_off && t_full && a_fit && dadt && d2adt2))
    return refuse(IONODE_ERR_ARG, "%s: required buffer is NULL (x, full_off, t_full, a_fit, dadt, d2adt2)", who);
  if (const int rc = n_params_rule(who, n_params)) return rc;
  if (n_seg < 1) return refuse(IONODE_ERR_ARG, "%s: n_seg must be positive", who);
  g = ionode::EfEvalArgs{n_seg, n_params, x, full_off, t_full, a_fit, dadt, d2adt2};
  return IONODE_OK;
}

}  // namespace

extern "C" {

int ionode_multi_exp_objective(int32_t n_run, int32_t n_active, int32_t lambda, int32_t n_params, const int32_t *active,
                               const int32_t *seg_of_run, const int64_t *seg_off, const double *t_rel, const double *a, const double *trial,
                               double *value, int32_t *status, void *stream) {
  ionode::EfArgs g;
  const int rc = objective_args("ionode_multi_exp_objective", n_run, n_active, lambda, n_params, active, seg_of_run, seg_off, t_rel, a, trial,
                                value, status, g);
  if (rc != IONODE_OK) return rc;
  ionode::launch_multi_exp_objective(g, reinterpret_cast<hipStream_t>(stream));
  return ionode::step_launched("ionode_multi_exp_objective");
}

int ionode_multi_exp_objective_host(int32_t n_run, int32_t n_active, int32_t lambda, int32_t n_params, const int32_t *active,
                                    const int32_t *seg_of_run, const int64_t *seg_off, const double *t_rel, const double *a,
                                    const double *trial, double *value, int32_t *status) {
  ionode::EfArgs g;
  const int rc = objective_args("ionode_multi_exp_objective_host", n_run, n_active, lambda, n_params, active, seg_of_run, seg_off, t_rel, a,
                                trial, value, status, g);
  if (rc != IONODE_OK) return rc;
  ionode::multi_exp_objective_host(g);
  return IONODE_OK;
}

int ionode_multi_exp_eval(int32_t n_seg, int32_t n_params, const double *x, const int64_t *full_off, const double *t_full, double *a_fit,
                          double *dadt, double *d2adt2, void *stream) {
  ionode::EfEvalArgs g;
  const int rc = eval_args("ionode_multi_exp_eval", n_seg, n_params, x, full_off, t_full, a_fit, dadt, d2adt2, g);
  if (rc != IONODE_OK) return rc;
  ionode::launch_multi_exp_eval(g, reinterpret_cast<hipStream_t>(stream));
  return ionode::step_launched("ionode_multi_exp_eval");
}

int ionode_multi_exp_eval_host(int32_t n_seg, int32_t n_params, const double *x, const int64_t *full_off, const double *t_full, double *a_fit,
                               double *dadt, double *d2adt2) {
  ionode::EfEvalArgs g;
  const int rc = eval_args("ionode_multi_exp_eval_host", n_seg, n_params, x, full_off, t_full, a_fit, dadt, d2adt2, g);
  if (rc != IONODE_OK) return rc;
  ionode::multi_exp_eval_host(g);
  return IONODE_OK;
}

}  // extern "C"
