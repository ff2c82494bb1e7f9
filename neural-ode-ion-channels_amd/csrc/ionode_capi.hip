// ionode_capi.hip -- the C ABI of libionode.so (include/ionode.h): the extern "C" surface, the three small kernels this unit owns or
// launches (protocol at outputs, compose order, dense expand) and the forward solve's one checked launch path, checked_solve.
// What to launch is decided in ionode_plan.hpp (plan_launch); the packed weight image is made in ionode_pack.hpp.
#include <vector>

#include "ionode_pack.hpp"

namespace {

thread_local const char *g_last_kernel = "";  // variant name of this thread's last successful ionode_dopri5 launch

int launch_failed(hipError_t e) {
  set_err("kernel launch failed: %s", hipGetErrorString(e));
  return IONODE_ERR_LAUNCH;
}

bool cost_source_ok(int cost_source) {
  if (cost_source >= 0 && cost_source <= 2) return true;
  set_err("cost_source: 0 (not composed), 1 (pilot) or 2 (counts)");
  return false;
}

// The plan queries: the LaunchPlan of `d` for a caller that will (want_current) or will not pass an i_out buffer
int query_plan(const ionode_desc *d, int32_t want_current, LaunchPlan *lp, int cost_source = 0) {
  return plan_launch(d, request_of(d, want_current != 0, false, true, true, cost_source), lp);
}

}  // namespace

namespace ionode {
// Pre-pass of the current / objective epilogue: V(t_k) for every protocol at every requested output time, evaluated ONCE per
// protocol with the same protocol_v() the integrator uses (so the epilogue's values do not change), instead of once per
// trajectory per sample (~35 fp64 vector instructions each: as much as the dense-output polynomial itself).
__global__ void __launch_bounds__(256) ionode_protocol_at_outputs_kernel(const KArgs a, double *__restrict__ v_out) {
  const long long n = (long long)a.P * a.Nt;
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long long)gridDim.x * 256) {
    const int p = (int)(e / a.Nt), k = (int)(e - (long long)p * a.Nt);
    double v;
    protocol_v(a, a.prot_v + (size_t)p * a.Np, a.t_eval[k], v);
    v_out[e] = v;
  }
}
}  // namespace ionode

extern "C" {

int32_t ionode_abi_version(void) { return IONODE_ABI_VERSION; }

const char *ionode_last_error(void) { return g_err; }

size_t ionode_mlp_packed_floats(int32_t L, int32_t N) { return image_layout(L, N).total; }

int ionode_mlp_pack(const float *w, int32_t L, int32_t N, float *out) { return pack_image(w, L, N, out); }

int ionode_launch_geometry(const ionode_desc *d, int32_t out[4]) {
  LaunchPlan lp;
  const int rc = plan_launch(d, Request{}, &lp);   // the states alone: not even a fused objective in `d` implies the epilogue here
  if (rc != IONODE_OK) return rc;
  out[0] = (int32_t)lp.kernel.grid;
  out[1] = (int32_t)lp.kernel.block;
  out[2] = (int32_t)lp.kernel.lds;
  out[3] = lp.kernel.v->G;
  return IONODE_OK;
}

const char *ionode_kernel_name(const ionode_desc *d) {
  LaunchPlan lp;
  // the descriptor does not say whether i_out will be passed: a table (or a fused objective) implies the epilogue
  if (query_plan(d, d && d->v_at_outputs != nullptr, &lp) != IONODE_OK) return "";
  return lp.kernel.v->name;
}

const char *ionode_last_kernel_name(void) { return g_last_kernel; }

int32_t ionode_lane_wise_from(int32_t model, int32_t mlp_width) { return lane_wise_from(model, mlp_width); }

int ionode_dense_defer_plan(const ionode_desc *d, int32_t want_current, int64_t out[2]) {
  LaunchPlan lp;
  const int rc = query_plan(d, want_current, &lp);
  if (rc != IONODE_OK) return rc;
  out[0] = lp.defer.cap;
  out[1] = lp.defer.bytes;
  return IONODE_OK;
}

int ionode_dense_tail_plan(const ionode_desc *d, int32_t want_current, int64_t out[2]) { return ionode_compose_tail_plan(d, want_current, 0, out); }

int ionode_compose_tail_plan(const ionode_desc *d, int32_t want_current, int32_t cost_source, int64_t out[2]) {
  LaunchPlan lp;
  const int rc = query_plan(d, want_current, &lp, cost_source);
  if (rc != IONODE_OK) return rc;
  if (!cost_source_ok(cost_source)) return IONODE_ERR_ARG;
  out[0] = lp.tail.rank;
  out[1] = lp.tail.fill;
  return IONODE_OK;
}

int ionode_compose_plan(const ionode_desc *d, int32_t want_current, int32_t out[2]) {
  LaunchPlan lp;
  const int rc = query_plan(d, want_current, &lp);
  if (rc != IONODE_OK) return rc;
  out[0] = lp.compose ? 1 : 0;
  out[1] = (int32_t)lp.source;
  return IONODE_OK;
}

int ionode_compose_order_host(const double *cost, int32_t n_traj, int32_t *order) {
  if (!cost || !order || n_traj < 1) { set_err("ionode_compose_order_host: bad argument"); return IONODE_ERR_ARG; }
  std::vector<int32_t> idx((size_t)n_traj);
  std::vector<double> c((size_t)n_traj);
  for (int32_t i = 0; i < n_traj; ++i) { idx[i] = i; c[i] = ionode::compose_cost(cost[i]); }
  std::sort(idx.begin(), idx.end(), [&](int32_t x, int32_t y) { return ionode::compose_before(c[x], x, c[y], y); });
  const bool flat = c[idx[0]] == c[idx[n_traj - 1]];
  for (int32_t p = 0; p < n_traj; ++p) order[flat ? p : ionode::compose_slot(p, n_traj)] = idx[p];
  return IONODE_OK;
}

int ionode_compose_order(const void *cost, int32_t cost_is_int64, int64_t cost_stride, int32_t n_traj, int32_t *order, void *stream) {
  if (!cost || !order || n_traj < 1 || cost_stride < 1) { set_err("ionode_compose_order: bad argument"); return IONODE_ERR_ARG; }
  if (n_traj > ionode::kComposeMaxB) { set_err("ionode_compose_order: more trajectories than the one-workgroup sort holds (8192)"); return IONODE_ERR_UNSUPPORTED; }
  const size_t lds = ionode::compose_lds_bytes(n_traj);
  auto kern = cost_is_int64 ? ionode::ionode_compose_kernel<1> : ionode::ionode_compose_kernel<0>;
  if (lds > 64 * 1024) {
    const hipError_t ea = hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (ea != hipSuccess) return launch_failed(ea);
  }
  hipLaunchKernelGGL(kern, dim3(1), dim3(ionode::kComposeThreads), lds, reinterpret_cast<hipStream_t>(stream), cost, (long long)cost_stride,
                     (int)n_traj, order);
  const hipError_t e = hipGetLastError();
  return e != hipSuccess ? launch_failed(e) : IONODE_OK;
}

}  // extern "C"

namespace {

// What a solve entry point received, by the names of include/ionode.h; what it does not have keeps its default.
struct Received {
  const float *mlp_packed;
  const double *params, *prot_v, *prot_t, *t_eval;
  const int32_t *prot_of_traj;
  const void *y0;
  void *y_out, *stream, *workspace;
  double *i_out;
  int32_t *status;
  int64_t *stats;
  int64_t workspace_bytes;
  int32_t cost_source, objective;   // 0: not composed, IONODE_OBJECTIVE_SSE
};

inline bool is_mlp(const ionode_desc *d) { return d->model == IONODE_MODEL_NNF || d->model == IONODE_MODEL_NND; }

// The kernel arguments of a call that passed checked_solve's checks
ionode::KArgs fill_kargs(const ionode_desc *d, const Received &r, const LaunchPlan &lp) {
  const bool mlp = is_mlp(d);
  ionode::KArgs a;
  memset(&a, 0, sizeof a);
  a.mlp = r.mlp_packed; a.params = r.params; a.prot_v = r.prot_v; a.prot_t = r.prot_t; a.prot_of_traj = r.prot_of_traj;
  a.y0 = r.y0; a.t_eval = r.t_eval; a.y_out = r.y_out; a.i_out = r.i_out; a.status = r.status; a.stats = r.stats;
  a.B = d->n_traj; a.Nt = d->n_out; a.P = d->n_prot; a.Np = d->prot_n; a.n_params = d->n_params;
  if (mlp) { a.L = d->mlp_layers; a.N = d->mlp_width; a.NP = np_of(d->mlp_width); a.NT = a.NP / 16; }
  a.max_steps = d->max_steps > 0 ? d->max_steps : (int64_t)2147483647;  // torchdiffeq max_num_steps default 2**31 - 1
  a.max_total = d->max_total_steps > 0 ? d->max_total_steps
                                       : (d->max_total_steps == 0 ? (int64_t)IONODE_DEFAULT_MAX_TOTAL_STEPS : INT64_MAX);
  a.ckpt = d->ckpt; a.ckpt_cap = d->ckpt ? d->ckpt_cap : 0;
  a.prot_rdt = 1.0 / d->prot_dt;  // correctly rounded: the kernels divide by prot_dt through div_by()
  a.dt_max = d->max_step > 0.0 ? d->max_step : __builtin_inf();
  a.prot_t0 = d->prot_t0; a.prot_dt = d->prot_dt; a.v_oob = d->v_oob; a.rtol = d->rtol; a.atol = d->atol;
  a.obs_g = d->obs_g; a.obs_e = d->obs_e; a.obs_open = d->obs_open_state_only;
  a.step_log = d->step_log; a.step_log_cap = d->step_log ? d->step_log_cap : 0;
  a.sse_ref = d->sse_ref; a.sse_out = d->sse_out; a.v_tab = d->v_at_outputs;
  a.obj_abs = r.objective == IONODE_OBJECTIVE_SAE ? 1 : 0;
  if (mlp && d->traj_per_image > 0) { a.mlp_stride = d->mlp_image_stride; a.traj_per_img = d->traj_per_image; }  // checked in make_plan
  a.order = d->launch_order;
  a.lw_bytes = (int32_t)lp.kernel.lw_bytes;
  a.te_t0 = d->t_eval_t0_hint; a.te_dt = (d->t_eval_dt_hint > 0.0 && d->n_out > 1) ? d->t_eval_dt_hint : 0.0;
  a.te_rdt = a.te_dt > 0.0 ? 1.0 / a.te_dt : 0.0;
  a.te_exact = (a.te_dt > 0.0 && d->t_eval_exact) ? 1 : 0;
  a.tile_shrink = lp.kernel.tile_shrink ? 1 : 0;
  if (lp.defer.cap > 0) {
    using Rec = ionode::DenseRecord<2>;
    a.defer_count = static_cast<int32_t *>(r.workspace);
    a.defer_rec = reinterpret_cast<double *>(static_cast<unsigned char *>(r.workspace) + Rec::records_offset(d->n_traj));
    a.defer_cap = (int32_t)lp.defer.cap;
    a.defer_fill = (int32_t)lp.tail.fill;
    a.defer_tail_rank = (int32_t)lp.tail.rank;
    // the tail block: the last record slot (no trajectory fills it)
    if (lp.tail.rank > 0) a.defer_tail = reinterpret_cast<int32_t *>(a.defer_rec + ((size_t)d->n_traj * (size_t)lp.defer.cap - 1) * Rec::ROW);
  }
  return a;
}

// The four solve entry points' one path: the checks, then the solve and, when the plan defers the dense output into the workspace, its
// expansion.  The order of the checks is pinned by tests/golden/forward_entry_checks.json: the objective's kind first (whatever else is
// wrong with the call, an unknown kind or absolute values without a fused objective is what it reports), cost_source, the plan's
// refusals (NULL descriptor, inconsistent descriptor, MLP shape, traj_per_image), NULL buffers, the fused objective's prerequisites,
// ckpt_cap, launch_order with traj_per_image, the workspace's size and alignment.  Nothing on the device is touched before the last.
int checked_solve(const ionode_desc *d, const Received &r) {
  if (r.objective != IONODE_OBJECTIVE_SSE && r.objective != IONODE_OBJECTIVE_SAE) {
    set_err("ionode_dopri5_objective: objective must be IONODE_OBJECTIVE_SSE (0) or IONODE_OBJECTIVE_SAE (1)");
    return IONODE_ERR_ARG;
  }
  if (r.objective == IONODE_OBJECTIVE_SAE && (d == nullptr || d->sse_out == nullptr)) {
    set_err("ionode_dopri5_objective: IONODE_OBJECTIVE_SAE needs the fused objective's output, d->sse_out");
    return IONODE_ERR_ARG;
  }
  if (!cost_source_ok(r.cost_source)) return IONODE_ERR_ARG;
  LaunchPlan lp;
  const int rc = plan_launch(d, request_of(d, r.i_out != nullptr, r.prot_t != nullptr, r.workspace != nullptr, r.y_out != nullptr, r.cost_source, r.objective), &lp);
  if (rc != IONODE_OK) return rc;
  if (!r.params || !r.prot_v || !r.y0 || !r.t_eval || (!r.y_out && !d->sse_out) || !r.status || (is_mlp(d) && !r.mlp_packed)) {
    set_err("ionode_dopri5: required buffer is NULL");
    return IONODE_ERR_ARG;
  }
  if (d->sse_out && (!d->sse_ref || !(d->t_eval_dt_hint > 0.0) || d->n_out < 2)) {
    set_err("fused objective: sse_out needs sse_ref and the output-grid hint (t_eval_dt_hint > 0)");
    return IONODE_ERR_ARG;
  }
  if (d->ckpt && d->ckpt_cap < 1) { set_err("ckpt given with ckpt_cap < 1"); return IONODE_ERR_ARG; }
  if (d->launch_order && is_mlp(d) && d->traj_per_image > 0) {
    set_err("launch_order cannot be combined with traj_per_image (tiles of an image must stay together)");
    return IONODE_ERR_ARG;
  }
  if (lp.defer.cap > 0 && (r.workspace_bytes < lp.defer.bytes || (reinterpret_cast<uintptr_t>(r.workspace) & 15) != 0)) {
    set_err("ionode_dopri5_deferred: workspace smaller than ionode_dense_defer_plan() asks for, or not 16-byte aligned");
    return IONODE_ERR_ARG;
  }
  const ionode::KArgs a = fill_kargs(d, r, lp);
  const hipStream_t stream = reinterpret_cast<hipStream_t>(r.stream);
  if (a.defer_tail) {   // the tail's finish counter, zeroed in stream order ahead of the solve
    const hipError_t em = hipMemsetAsync(a.defer_tail, 0, ionode::DenseRecord<2>::BYTES, stream);
    if (em != hipSuccess) { set_err("hipMemsetAsync failed: %s", hipGetErrorString(em)); return IONODE_ERR_LAUNCH; }
  }
  hipError_t e = lp.kernel.v->fn(a, lp.kernel.grid, lp.kernel.lds, stream);
  if (e != hipSuccess) return launch_failed(e);
  if (lp.defer.cap > 0) {
    const int64_t blocks = std::min<int64_t>((lp.defer.cap + ionode::kExpandRecordsPerWg - 1) / ionode::kExpandRecordsPerWg, ionode::kExpandMaxBlocks);
    const dim3 grid((unsigned)std::min<int64_t>((int64_t)d->n_traj * blocks, ionode::kExpandGrid));
    if (d->state_f32) hipLaunchKernelGGL((ionode::ionode_dense_expand_kernel<float, 2>), grid, dim3(256), 0, stream, a);
    else hipLaunchKernelGGL((ionode::ionode_dense_expand_kernel<double, 2>), grid, dim3(256), 0, stream, a);
    e = hipGetLastError();
    if (e != hipSuccess) return launch_failed(e);
  }
  g_last_kernel = lp.kernel.v->name;
  return IONODE_OK;
}

}  // namespace

extern "C" {

// The solve entry points (include/ionode.h): each names what it received and hands it to checked_solve.
int ionode_dopri5(const ionode_desc *d, const float *mlp_packed, const double *params, const double *prot_v,
                  const double *prot_t, const int32_t *prot_of_traj, const void *y0, const double *t_eval,
                  void *y_out, double *i_out, int32_t *status, int64_t *stats, void *stream) {
  Received r = {};
  r.mlp_packed = mlp_packed; r.params = params; r.prot_v = prot_v; r.prot_t = prot_t; r.prot_of_traj = prot_of_traj; r.y0 = y0;
  r.t_eval = t_eval; r.y_out = y_out; r.i_out = i_out; r.status = status; r.stats = stats; r.stream = stream;
  return checked_solve(d, r);
}

int ionode_dopri5_deferred(const ionode_desc *d, const float *mlp_packed, const double *params, const double *prot_v,
                           const double *prot_t, const int32_t *prot_of_traj, const void *y0, const double *t_eval,
                           void *y_out, double *i_out, int32_t *status, int64_t *stats, void *stream, void *workspace,
                           int64_t workspace_bytes) {
  Received r = {};
  r.mlp_packed = mlp_packed; r.params = params; r.prot_v = prot_v; r.prot_t = prot_t; r.prot_of_traj = prot_of_traj; r.y0 = y0;
  r.t_eval = t_eval; r.y_out = y_out; r.i_out = i_out; r.status = status; r.stats = stats; r.stream = stream;
  r.workspace = workspace; r.workspace_bytes = workspace_bytes;
  return checked_solve(d, r);
}

int ionode_dopri5_composed(const ionode_desc *d, const float *mlp_packed, const double *params, const double *prot_v,
                           const double *prot_t, const int32_t *prot_of_traj, const void *y0, const double *t_eval,
                           void *y_out, double *i_out, int32_t *status, int64_t *stats, void *stream, void *workspace,
                           int64_t workspace_bytes, int32_t cost_source) {
  Received r = {};
  r.mlp_packed = mlp_packed; r.params = params; r.prot_v = prot_v; r.prot_t = prot_t; r.prot_of_traj = prot_of_traj; r.y0 = y0;
  r.t_eval = t_eval; r.y_out = y_out; r.i_out = i_out; r.status = status; r.stats = stats; r.stream = stream;
  r.workspace = workspace; r.workspace_bytes = workspace_bytes; r.cost_source = cost_source;
  return checked_solve(d, r);
}

int ionode_dopri5_objective(const ionode_desc *d, const float *mlp_packed, const double *params, const double *prot_v,
                            const double *prot_t, const int32_t *prot_of_traj, const void *y0, const double *t_eval,
                            void *y_out, double *i_out, int32_t *status, int64_t *stats, void *stream, void *workspace,
                            int64_t workspace_bytes, int32_t cost_source, int32_t objective) {
  Received r = {};
  r.mlp_packed = mlp_packed; r.params = params; r.prot_v = prot_v; r.prot_t = prot_t; r.prot_of_traj = prot_of_traj; r.y0 = y0;
  r.t_eval = t_eval; r.y_out = y_out; r.i_out = i_out; r.status = status; r.stats = stats; r.stream = stream;
  r.workspace = workspace; r.workspace_bytes = workspace_bytes; r.cost_source = cost_source; r.objective = objective;
  return checked_solve(d, r);
}

int ionode_protocol_at_outputs(const ionode_desc *d, const double *prot_v, const double *prot_t, const double *t_eval,
                               double *v_out, void *stream) {
  if (!d || !prot_v || !t_eval || !v_out) { set_err("ionode_protocol_at_outputs: required buffer is NULL"); return IONODE_ERR_ARG; }
  if (d->n_out < 1 || d->n_prot < 1 || d->prot_n < 2 || !(d->prot_dt > 0)) { set_err("ionode_protocol_at_outputs: empty grid / protocol"); return IONODE_ERR_ARG; }
  ionode::KArgs a;
  memset(&a, 0, sizeof a);
  a.prot_v = prot_v; a.prot_t = prot_t; a.t_eval = t_eval; a.Nt = d->n_out; a.P = d->n_prot; a.Np = d->prot_n;
  a.prot_t0 = d->prot_t0; a.prot_dt = d->prot_dt; a.prot_rdt = 1.0 / d->prot_dt; a.v_oob = d->v_oob;
  const long long n = (long long)a.P * a.Nt;
  const unsigned grid = (unsigned)((n + 255) / 256 > 65536 ? 65536 : (n + 255) / 256);
  hipLaunchKernelGGL(ionode::ionode_protocol_at_outputs_kernel, dim3(grid), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), a, v_out);
  const hipError_t e = hipGetLastError();
  return e != hipSuccess ? launch_failed(e) : IONODE_OK;
}

}  // extern "C"
