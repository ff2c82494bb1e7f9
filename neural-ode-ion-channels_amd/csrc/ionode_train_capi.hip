// ionode_train_capi.hip -- C ABI of the update of training through the solve (include/ionode.h "Training through the solve"): the
// checks, the launches and the host mirrors.  A unit of its own: the other units compile to what they did.
#include "ionode_train.hpp"
#include "ionode_step_capi.hpp"

namespace {

using ionode::refuse;

// n is the state-dict size of (L, N): W0[N][2], b0[N], L x (W[N][N], b[N]), wl[N], bl
int shape_rule(const char *who, int32_t n, int32_t L, int32_t N) {
  if (L < 0 || N < 1 || N > 512) return refuse(IONODE_ERR_ARG, "%s: (mlp_layers, mlp_width) = (%d, %d) is no net", who, (int)L, (int)N);
  const int64_t expect = 3 * (int64_t)N + (int64_t)L * ((int64_t)N * N + N) + N + 1;
  if (n != expect) return refuse(IONODE_ERR_ARG, "%s: n = %d floats, the state dict of (L=%d, N=%d) has %lld", who, (int)n, (int)L, (int)N, (long long)expect);
  return IONODE_OK;
}

int norm_args(const char *who, int32_t n, int32_t L, int32_t N, const double *acc, const int32_t *padmap, float *grad, double *norm_part,
              ionode::TrNormArgs &g) {
  if (!(acc && padmap && grad && norm_part)) return refuse(IONODE_ERR_ARG, "%s: required buffer is NULL (acc, padmap, grad, norm_partials)", who);
  if (const int rc = shape_rule(who, n, L, N)) return rc;
  const size_t n_acc = ionode_grad_partial_floats(L, N);
  if (n_acc == 0) return refuse(IONODE_ERR_ARG, "%s: the gradient path needs at least one hidden layer", who);
  g = ionode::TrNormArgs{n, (int64_t)n_acc, acc, padmap, grad, norm_part};
  return IONODE_OK;
}

int apply_args(const char *who, int32_t n, int32_t L, int32_t N, const float *grad, const double *norm_part, const double *loss,
               const double *state_in, double *state_out, float *w, float *m, float *v, float lr, double beta1, double beta2, float eps,
               double max_norm, ionode::TrApplyArgs &g) {
  if (!(grad && norm_part && loss && state_in && state_out && w && m && v))
    return refuse(IONODE_ERR_ARG, "%s: required buffer is NULL (grad, norm_partials, loss, state_in, state_out, weights, exp_avg, exp_avg_sq)", who);
  if (const int rc = shape_rule(who, n, L, N)) return rc;
  if (state_in == state_out) return refuse(IONODE_ERR_ARG, "%s: state_in and state_out must be two blocks", who);
  if (!(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0))
    return refuse(IONODE_ERR_ARG, "%s: betas = (%g, %g) outside [0, 1)", who, beta1, beta2);
  if (!(eps > 0.0f)) return refuse(IONODE_ERR_ARG, "%s: eps = %g must be positive", who, (double)eps);
  if (!std::isfinite(lr)) return refuse(IONODE_ERR_ARG, "%s: lr is not finite", who);
  if (!std::isfinite(max_norm)) return refuse(IONODE_ERR_ARG, "%s: max_norm is not finite", who);
  g = ionode::TrApplyArgs{n, ionode_train_norm_partials(n), grad, norm_part, loss, state_in, state_out, w, m, v, lr, eps, beta1, beta2, max_norm};
  return IONODE_OK;
}

int refresh_args(const char *who, int32_t n, int32_t L, int32_t N, const int32_t *fwd_map, const int32_t *grad_map, const float *w,
                 float *fwd_image, float *grad_image, ionode::TrRefreshArgs &g) {
  if (!(fwd_map && w && fwd_image) || (grad_map == nullptr) != (grad_image == nullptr))
    return refuse(IONODE_ERR_ARG, "%s: required buffer is NULL (forward_map, weights, forward_image; grad_map and grad_image come together)", who);
  if (const int rc = shape_rule(who, n, L, N)) return rc;
  const size_t n_fwd = ionode_mlp_packed_floats(L, N);
  if (n_fwd == 0) return refuse(IONODE_ERR_UNSUPPORTED, "%s: no forward kernel serves (L=%d, N=%d)", who, (int)L, (int)N);
  const size_t n_grad = grad_map ? ionode_grad_image_floats(L, N) : 0;
  if (grad_map && n_grad == 0) return refuse(IONODE_ERR_UNSUPPORTED, "%s: no grad image for (L=%d, N=%d)", who, (int)L, (int)N);
  g = ionode::TrRefreshArgs{n, (int64_t)n_fwd, (int64_t)n_grad, fwd_map, grad_map, w, fwd_image, grad_image};
  return IONODE_OK;
}

}  // namespace

extern "C" {

int32_t ionode_train_norm_partials(int32_t n) { return n < 1 ? 0 : (n + ionode::kTrChunk - 1) / ionode::kTrChunk; }

int ionode_train_grad_norm(int32_t n, int32_t L, int32_t N, const double *acc, const int32_t *padmap, float *grad, double *norm_part,
                           void *stream) {
  ionode::TrNormArgs g;
  if (const int rc = norm_args("ionode_train_grad_norm", n, L, N, acc, padmap, grad, norm_part, g)) return rc;
  ionode::launch_train_grad_norm(g, reinterpret_cast<hipStream_t>(stream));
  return ionode::step_launched("ionode_train_grad_norm");
}

int ionode_train_grad_norm_host(int32_t n, int32_t L, int32_t N, const double *acc, const int32_t *padmap, float *grad, double *norm_part) {
  ionode::TrNormArgs g;
  if (const int rc = norm_args("ionode_train_grad_norm_host", n, L, N, acc, padmap, grad, norm_part, g)) return rc;
  ionode::train_grad_norm_host(g);
  return IONODE_OK;
}

int ionode_train_apply(int32_t n, int32_t L, int32_t N, const float *grad, const double *norm_part, const double *loss,
                       const double *state_in, double *state_out, float *w, float *m, float *v, float lr, double beta1, double beta2,
                       float eps, double max_norm, void *stream) {
  ionode::TrApplyArgs g;
  if (const int rc = apply_args("ionode_train_apply", n, L, N, grad, norm_part, loss, state_in, state_out, w, m, v, lr, beta1, beta2, eps,
                                max_norm, g))
    return rc;
  ionode::launch_train_apply(g, reinterpret_cast<hipStream_t>(stream));
  return ionode::step_launched("ionode_train_apply");
}

int ionode_train_apply_host(int32_t n, int32_t L, int32_t N, const float *grad, const double *norm_part, const double *loss,
                            const double *state_in, double *state_out, float *w, float *m, float *v, float lr, double beta1, double beta2,
                            float eps, double max_norm) {
  ionode::TrApplyArgs g;
  if (const int rc = apply_args("ionode_train_apply_host", n, L, N, grad, norm_part, loss, state_in, state_out, w, m, v, lr, beta1, beta2,
                                eps, max_norm, g))
    return rc;
  ionode::train_apply_host(g);
  return IONODE_OK;
}

int ionode_train_refresh(int32_t n, int32_t L, int32_t N, const int32_t *fwd_map, const int32_t *grad_map, const float *w, float *fwd_image,
                         float *grad_image, void *stream) {
  ionode::TrRefreshArgs g;
  if (const int rc = refresh_args("ionode_train_refresh", n, L, N, fwd_map, grad_map, w, fwd_image, grad_image, g)) return rc;
  ionode::launch_train_refresh(g, reinterpret_cast<hipStream_t>(stream));
  return ionode::step_launched("ionode_train_refresh");
}

int ionode_train_refresh_host(int32_t n, int32_t L, int32_t N, const int32_t *fwd_map, const int32_t *grad_map, const float *w,
                              float *fwd_image, float *grad_image) {
  ionode::TrRefreshArgs g;
  if (const int rc = refresh_args("ionode_train_refresh_host", n, L, N, fwd_map, grad_map, w, fwd_image, grad_image, g)) return rc;
  ionode::train_refresh_host(g);
  return IONODE_OK;
}

}  // extern "C"
