// ionode_predictive_capi.hip -- C ABI of the posterior predictive bands (include/ionode.h "Posterior predictive bands"): the checks,
// the plan, the launches and the host mirrors.  A unit of its own: the other units compile to what they did.
#include "ionode_predictive.hpp"
#include "ionode_step_capi.hpp"

namespace {

using ionode::refuse;

// what the column store's shape must satisfy, for the plan and the quantiles alike
int store_rule(const char *who, int32_t n_prot, int32_t n_out, int32_t s_cap) {
  if (n_prot < 1 || n_out < 1 || s_cap < 1) return refuse(IONODE_ERR_ARG, "%s: n_prot, n_out and s_cap must be positive", who);
  if ((int64_t)n_prot * n_out > INT32_MAX)
    return refuse(IONODE_ERR_ARG, "%s: n_prot * n_out = %lld columns exceed one launch's %d", who, (long long)n_prot * n_out, INT32_MAX);
  if (s_cap > IONODE_PREDICTIVE_MAX_DRAWS)
    return refuse(IONODE_ERR_UNSUPPORTED,
                  "%s: s_cap = %d draws per column exceed %d, what one workgroup sorts in LDS (128 KiB of the compute unit's 160): thin the "
                  "pool with max_draws (predictive.draws), or ask for no quantiles",
                  who, (int)s_cap, IONODE_PREDICTIVE_MAX_DRAWS);
  return IONODE_OK;
}

int accumulate_args(const char *who, const ionode_predictive_desc *d, const double *trace, const int32_t *status, const double *sigma,
                    double *mean, double *m2, double *mn, double *mx, int64_t *count, double *cols, ionode::PrArgs &a) {
  if (!d) return refuse(IONODE_ERR_ARG, "%s: null descriptor", who);
  if (!(trace && status && mean && m2 && mn && mx && count))
    return refuse(IONODE_ERR_ARG, "%s: required buffer is NULL (trace, status, mean, m2, min, max, count)", who);
  if (d->n_prot < 1 || d->n_prot > 65535 || d->n_out < 1 || d->n_draw < 1)
    return refuse(IONODE_ERR_ARG, "%s: n_prot (at most 65535), n_out and n_draw must be positive", who);
  if ((int64_t)d->n_draw * d->n_prot > INT32_MAX)
    return refuse(IONODE_ERR_ARG, "%s: n_draw * n_prot = %lld rows exceed one launch's %d", who, (long long)d->n_draw * d->n_prot, INT32_MAX);
  if (d->draw_base < 0 || d->draw_offset < 0 || (int64_t)d->draw_offset + d->draw_base + d->n_draw > INT32_MAX)
    return refuse(IONODE_ERR_ARG, "%s: draw_base = %d, draw_offset = %d: the draw indices must lie in 0 .. 2^31 - 1", who, (int)d->draw_base,
                  (int)d->draw_offset);
  if (d->noise && !sigma && !(d->sigma >= 0.0 && d->sigma < __builtin_inf()))
    return refuse(IONODE_ERR_ARG, "%s: noise without sigma: give the sigma array or a finite sigma >= 0", who);
  if (cols) {
    if (const int rc = store_rule(who, d->n_prot, d->n_out, d->s_cap)) return rc;
    if ((int64_t)d->draw_base + d->n_draw > d->s_cap)
      return refuse(IONODE_ERR_ARG, "%s: draws %d .. %lld do not fit the column store's s_cap = %d", who, (int)d->draw_base,
                    (long long)d->draw_base + d->n_draw - 1, (int)d->s_cap);
  }
  a = ionode::PrArgs{};
  a.P = d->n_prot; a.Nt = d->n_out; a.n_draw = d->n_draw; a.S_cap = d->s_cap; a.draw_base = d->draw_base; a.draw_offset = d->draw_offset; a.noise = d->noise ? 1 : 0;
  ionode::step_seed(d->seed, a.seed_lo, a.seed_hi);
  a.sigma0 = d->sigma;
  a.trace = trace; a.status = status; a.sigma = sigma;
  a.mean = mean; a.m2 = m2; a.mn = mn; a.mx = mx; a.count = count; a.cols = cols;
  return IONODE_OK;
}

int quantile_args(const char *who, int32_t n_prot, int32_t n_out, int32_t s_cap, int32_t n_q, const double *q, const int64_t *count,
                  const double *cols, double *quant, ionode::PrQuantArgs &a) {
  if (!(q && count && cols && quant)) return refuse(IONODE_ERR_ARG, "%s: required buffer is NULL (q, count, cols, quant)", who);
  if (const int rc = store_rule(who, n_prot, n_out, s_cap)) return rc;
  if (n_q < 1 || n_q > IONODE_PREDICTIVE_MAX_Q) return refuse(IONODE_ERR_ARG, "%s: n_q = %d outside 1 .. %d", who, (int)n_q, IONODE_PREDICTIVE_MAX_Q);
  a = ionode::PrQuantArgs{};
  for (int i = 0; i < n_q; ++i) {
    if (!(q[i] >= 0.0 && q[i] <= 1.0)) return refuse(IONODE_ERR_ARG, "%s: q[%d] = %g outside [0, 1]", who, i, q[i]);
    a.q[i] = q[i];
  }
  a.P = n_prot; a.Nt = n_out; a.S_cap = s_cap; a.Q = n_q;
  a.count = count; a.cols = cols; a.quant = quant;
  return IONODE_OK;
}

}  // namespace

extern "C" {

int ionode_predictive_plan(int32_t n_prot, int32_t n_out, int32_t s_cap, int64_t budget_bytes, int64_t out[3]) {
  const char *who = "ionode_predictive_plan";
  if (!out) return refuse(IONODE_ERR_ARG, "%s: out is NULL", who);
  if (const int rc = store_rule(who, n_prot, n_out, s_cap)) return rc;
  const int L = ionode::pr_sort_log2(s_cap);
  const int64_t bytes = (int64_t)sizeof(double) * n_prot * n_out * s_cap;
  if (budget_bytes > 0 && bytes > budget_bytes)
    return refuse(IONODE_ERR_UNSUPPORTED,
                  "%s: the column store [%d][%d][%d] takes %lld bytes, above budget_bytes = %lld: thin the pool with max_draws "
                  "(predictive.draws), raise the budget, or ask for no quantiles",
                  who, (int)n_prot, (int)n_out, (int)s_cap, (long long)bytes, (long long)budget_bytes);
  out[0] = (int64_t)sizeof(uint64_t) << L;
  out[1] = bytes;
  out[2] = L;
  return IONODE_OK;
}

int ionode_predictive_accumulate(const ionode_predictive_desc *d, const double *trace, const int32_t *status, const double *sigma,
                                 double *mean, double *m2, double *min, double *max, int64_t *count, double *cols, void *stream) {
  ionode::PrArgs a;
  const int rc = accumulate_args("ionode_predictive_accumulate", d, trace, status, sigma, mean, m2, min, max, count, cols, a);
  if (rc != IONODE_OK) return rc;
  ionode::launch_predictive_accumulate(a, reinterpret_cast<hipStream_t>(stream));
  return ionode::step_launched("ionode_predictive_accumulate");
}

int ionode_predictive_accumulate_host(const ionode_predictive_desc *d, const double *trace, const int32_t *status, const double *sigma,
                                      double *mean, double *m2, double *min, double *max, int64_t *count, double *cols) {
  ionode::PrArgs a;
  const int rc = accumulate_args("ionode_predictive_accumulate_host", d, trace, status, sigma, mean, m2, min, max, count, cols, a);
  if (rc != IONODE_OK) return rc;
  ionode::predictive_accumulate_host(a);
  return IONODE_OK;
}

int ionode_predictive_quantiles(int32_t n_prot, int32_t n_out, int32_t s_cap, int32_t n_q, const double *q, const int64_t *count,
                                const double *cols, double *quant, void *stream) {
  ionode::PrQuantArgs a;
  const int rc = quantile_args("ionode_predictive_quantiles", n_prot, n_out, s_cap, n_q, q, count, cols, quant, a);
  if (rc != IONODE_OK) return rc;
  ionode::launch_predictive_quantiles(a, reinterpret_cast<hipStream_t>(stream));
  return ionode::step_launched("ionode_predictive_quantiles");
}

int ionode_predictive_quantiles_host(int32_t n_prot, int32_t n_out, int32_t s_cap, int32_t n_q, const double *q, const int64_t *count,
                                     const double *cols, double *quant) {
  ionode::PrQuantArgs a;
  const int rc = quantile_args("ionode_predictive_quantiles_host", n_prot, n_out, s_cap, n_q, q, count, cols, quant, a);
  if (rc != IONODE_OK) return rc;
  ionode::predictive_quantiles_host(a);
  return IONODE_OK;
}

}  // extern "C"
