// ionode_grad_capi.hip -- C ABI of the gradient path (include/ionode.h, "gradients through the solve"): the grad image
// packer, the backward-sweep launcher and the weight-gradient reduction launcher.
#include <cstdio>
#include <cstring>

#include "ionode_grad_launch.hpp"
#include "ionode_grad_reduce.hpp"

namespace {

thread_local char g_gerr[256] = "";
void gerr(const char *m) { snprintf(g_gerr, sizeof g_gerr, "%s", m); }

inline int np_of(int N) { return 16 * ((N + 15) / 16); }

using ionode::GArgs;
using ionode::Sweep;
using ionode::SweepFn;

// launchers that have no width: the closed-form models' sweeps (NT = 1, unused) and the NN models' walk
template <int MODEL> SweepFn closed_sweep(int f32) { return f32 ? &ionode::launch_sweep<MODEL, float, 1> : &ionode::launch_sweep<MODEL, double, 1>; }
template <int MODEL> SweepFn closed_sweep_sse(int f32) { return f32 ? &ionode::launch_sweep_sse<MODEL, float> : &ionode::launch_sweep_sse<MODEL, double>; }
inline SweepFn sse_gc(int f32) { return f32 ? &ionode::launch_sse_gc<float> : &ionode::launch_sse_gc<double>; }
template <int MODEL> SweepFn walk(int f32) { return f32 ? &ionode::launch_walk<MODEL, float> : &ionode::launch_walk<MODEL, double>; }

// nullptr: no variant of that width (a width without a sweep has no walk either, though the walk kernel itself has no width)
SweepFn find_sweep(Sweep which, int model, int f32, int NT) {
  if (which == Sweep::Walk) {
    if (!ionode::for_width(NT, [](auto) {}, [] {})) return nullptr;
    return model == IONODE_MODEL_NNF ? walk<IONODE_MODEL_NNF>(f32) : walk<IONODE_MODEL_NND>(f32);
  }
  const bool recompute = which == Sweep::Recompute;
  SweepFn fn = nullptr;
  ionode::for_width(NT, [&](auto nt) { fn = ionode::pick_sweep<decltype(nt)::value>(recompute, model, f32); },
                    [&] { fn = ionode::pick_sweep32(recompute, model, f32); });   // inst_grad32.hip
  return fn;
}

// ---- what every sweep entry point shares: the descriptor's consistency, and the argument block filled from it ----
inline bool is_m6(const ionode_desc *d) { return d->model == IONODE_MODEL_MARKOV6; }
inline bool desc_consistent(const ionode_desc *d) {
  const bool m6 = is_m6(d);
  return !(d->n_state != (m6 ? 6 : 2) || d->n_traj < 1 || d->n_out < 1 || d->n_prot < 1 || d->prot_n < 2 || d->n_params < (m6 ? 12 : 8) || !(d->prot_dt > 0));
}
inline bool bad_range(int32_t it_begin, int32_t it_end, int32_t n_iter) { return it_begin < 0 || it_end <= it_begin || it_end > n_iter; }

// (L, NP): the net; closed-form models: (0, 16)
GArgs fill_args(const ionode_desc *d, int L, int NP, int32_t it_begin, int32_t it_end, int32_t n_iter, const double *params,
                const double *prot_v, const double *prot_t, const int32_t *prot_of_traj, const double *t_eval, const int32_t *n_accepted,
                double *state, double *grad_params, double *grad_y0) {
  GArgs a;
  memset(&a, 0, sizeof a);
  a.k.params = params; a.k.prot_v = prot_v; a.k.prot_t = prot_t; a.k.prot_of_traj = prot_of_traj; a.k.t_eval = t_eval;
  a.k.B = d->n_traj; a.k.Nt = d->n_out; a.k.P = d->n_prot; a.k.Np = d->prot_n; a.k.n_params = d->n_params;
  a.k.L = L; a.k.NP = NP; a.k.NT = NP / 16;
  a.k.prot_t0 = d->prot_t0; a.k.prot_dt = d->prot_dt; a.k.prot_rdt = 1.0 / d->prot_dt; a.k.v_oob = d->v_oob;
  a.ckpt = d->ckpt; a.ckpt_cap = d->ckpt_cap; a.nacc = n_accepted; a.state = state; a.grad_params = grad_params; a.grad_y0 = grad_y0;
  a.it_begin = it_begin; a.it_end = it_end; a.n_iter = n_iter;
  return a;
}

int launch(SweepFn fn, const GArgs &a, size_t lds, void *stream) {
  fn(a, (unsigned)((a.k.B + 15) / 16), lds, reinterpret_cast<hipStream_t>(stream));
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) { gerr(hipGetErrorString(e)); return IONODE_ERR_LAUNCH; }
  return IONODE_OK;
}

}  // namespace

extern "C" {

const char *ionode_grad_last_error(void) { return g_gerr; }

size_t ionode_grad_image_floats(int32_t L, int32_t N) {
  if (L < 1 || N < 1) return 0;
  return ionode::grad_img_floats(L, np_of(N) / 16);
}

size_t ionode_grad_record_floats(int32_t L, int32_t N) {
  if (L < 1 || N < 1) return 0;
  return (size_t)ionode::grad_record_floats(L, np_of(N) / 16);
}

int ionode_grad_pack(const float *w, int32_t L, int32_t N, float *out) {
  if (!w || !out || L < 1 || N < 1) { gerr("ionode_grad_pack: bad argument"); return IONODE_ERR_ARG; }
  const int NP = np_of(N), NT = NP / 16;
  memset(out, 0, ionode::grad_img_floats(L, NT) * sizeof(float));
  const float *W0 = w, *b0 = w + (size_t)N * 2;
  for (int r = 0; r < N; ++r) {
    out[4 * r + 0] = b0[r];
    out[4 * r + 1] = W0[2 * r + 0];
    out[4 * r + 2] = W0[2 * r + 1];
  }
  const float *src = b0 + N;
  float *bias = out + ionode::grad_img_bias(NT);
  float *fw = out + ionode::grad_img_fwd(L, NT), *bw = out + ionode::grad_img_bwd(L, NT);
  for (int l = 0; l < L; ++l) {
    const float *W = src, *b = src + (size_t)N * N;
    for (int r = 0; r < N; ++r) bias[(size_t)l * NP + r] = b[r];
    // A operand of v_mfma_f32_16x16x4_f32, k-step r: lane = 16*kq + m supplies A[m][kq]; with the forward kernel's
    // k-permutation that is row 16*rt + m, contraction index 16*kt + 4*kq + r.  Transposed section: W^T.
    for (int rt = 0; rt < NT; ++rt)
      for (int kt = 0; kt < NT; ++kt)
        for (int lane = 0; lane < 64; ++lane) {
          const int m = lane & 15, kq = lane >> 4;
          const size_t f = ((((size_t)l * NT + rt) * NT + kt) * 64 + lane) * 4;
          for (int r = 0; r < 4; ++r) {
            const int row = 16 * rt + m, k = 16 * kt + 4 * kq + r;
            const bool in = row < N && k < N;
            fw[f + r] = in ? W[(size_t)row * N + k] : 0.0f;
            bw[f + r] = in ? W[(size_t)k * N + row] : 0.0f;
          }
        }
    src += (size_t)N * N + N;
  }
  float *wl = out + ionode::grad_img_wl(L, NT);
  for (int k = 0; k < N; ++k) wl[k] = src[k];
  wl[NP] = src[N];
  return IONODE_OK;
}

// One-phase sweep, or phase A (Recompute: the unit-seed products and packets of every (tile, step)) / phase B (Walk) of the two-phase
// sweep.  Phase A carries no adjoint state: it requires neither `state` nor the gradient outputs.
static int backward_impl(Sweep which, const ionode_desc *d, int32_t it_begin, int32_t it_end, int32_t n_iter, const float *grad_image,
                         const double *params, const double *prot_v, const double *prot_t, const int32_t *prot_of_traj,
                         const double *t_eval, const int32_t *n_accepted, const void *grad_y, double *state,
                         float *records, double *packets, double *grad_params, double *grad_y0, void *stream,
                         bool fused = false, const double *sse_y0 = nullptr) {
  // fused (two-phase only): the sum-of-squares objective -- no grad_y; the walk reads the sample-0 term of dL/dy0 from sse_y0
  if (!d) { gerr("null descriptor"); return IONODE_ERR_ARG; }
  const bool two_phase = which != Sweep::OnePhase;
  if (two_phase && (!packets || (d->model != IONODE_MODEL_NNF && d->model != IONODE_MODEL_NND))) {
    gerr("two-phase sweep: NN-f / NN-d only, `packets` required"); return IONODE_ERR_ARG;
  }
  const bool m6 = is_m6(d);
  const bool closed = d->model == IONODE_MODEL_HH2 || m6;  // closed-form models: no MLP image, no records
  if (d->model < 0 || d->model > 3) { gerr("backward sweep: unknown model"); return IONODE_ERR_UNSUPPORTED; }
  if (!desc_consistent(d)) { gerr("inconsistent descriptor"); return IONODE_ERR_ARG; }
  const bool adjoint = which != Sweep::Recompute;   // the launch reads and writes the adjoint state
  if ((!grad_image && !closed) || !params || !prot_v || !t_eval || !n_accepted || (fused ? (which == Sweep::Walk && !sse_y0) : !grad_y) || (adjoint && (!state || !grad_params || !grad_y0)) || !d->ckpt || d->ckpt_cap < 1) {
    gerr("ionode_dopri5_backward: required buffer is NULL (ckpt / ckpt_cap come from the descriptor)"); return IONODE_ERR_ARG;
  }
  if (bad_range(it_begin, it_end, n_iter)) { gerr("bad iteration range"); return IONODE_ERR_ARG; }
  if (which == Sweep::Recompute && (int64_t)it_end - it_begin > (int64_t)65535 * ionode::GRAD_RECOMPUTE_IB) {
    gerr("ionode_dopri5_backward_recompute: at most 65535 x 4 iterations per launch (HIP's grid.y limit): split the range");
    return IONODE_ERR_ARG;
  }
  if (d->traj_per_image > 0) { gerr("backward sweep: one weight set per launch (traj_per_image must be 0)"); return IONODE_ERR_UNSUPPORTED; }
  if (!closed && (d->mlp_layers < 1 || d->mlp_width < 1)) { gerr("bad MLP shape"); return IONODE_ERR_ARG; }
  const int NP = closed ? 16 : np_of(d->mlp_width), NT = NP / 16, L = closed ? 0 : d->mlp_layers;
  SweepFn fn = m6 ? closed_sweep<IONODE_MODEL_MARKOV6>(d->state_f32) : closed ? closed_sweep<IONODE_MODEL_HH2>(d->state_f32)
                                                                            : find_sweep(which, d->model, d->state_f32 ? 1 : 0, NT);
  const size_t lds = closed ? ionode::grad_closed_lds_bytes(d->n_state) : ionode::grad_lds_bytes(L, NT);
  if (!fn || lds > 160 * 1024 || L > 15) {
    gerr("backward sweep: (L, N) outside the compiled variants (N pads to 16, 112, 208 or 512; at most 15 hidden layers)");
    return IONODE_ERR_UNSUPPORTED;
  }
  GArgs a = fill_args(d, L, NP, it_begin, it_end, n_iter, params, prot_v, prot_t, prot_of_traj, t_eval, n_accepted, state, grad_params, grad_y0);
  a.k.N = d->mlp_width; a.img = grad_image; a.grad_y = fused ? nullptr : grad_y; a.sse_y0 = const_cast<double *>(sse_y0);
  a.records = closed ? nullptr : records;
  a.record_floats = ionode::grad_record_floats(L, NT);
  a.packets = two_phase ? packets : nullptr;
  if (two_phase && ionode::grad_lds_bytes(L, NT) + 16 + ionode::grad_walk_lds_bytes() > 160 * 1024) { gerr("two-phase sweep: LDS"); return IONODE_ERR_UNSUPPORTED; }
  return launch(fn, a, lds, stream);
}

int ionode_dopri5_backward(const ionode_desc *d, int32_t it_begin, int32_t it_end, int32_t n_iter, const float *grad_image,
                           const double *params, const double *prot_v, const double *prot_t, const int32_t *prot_of_traj,
                           const double *t_eval, const int32_t *n_accepted, const void *grad_y, double *state,
                           float *records, double *grad_params, double *grad_y0, void *stream) {
  return backward_impl(Sweep::OnePhase, d, it_begin, it_end, n_iter, grad_image, params, prot_v, prot_t, prot_of_traj, t_eval, n_accepted, grad_y,
                       state, records, nullptr, grad_params, grad_y0, stream);
}

int ionode_dopri5_backward_sse(const ionode_desc *d, int32_t it_begin, int32_t it_end, int32_t n_iter, const double *params,
                               const double *prot_v, const double *prot_t, const int32_t *prot_of_traj, const double *t_eval,
                               const int32_t *n_accepted, const double *grad_sse, double *state, double *grad_params,
                               double *grad_y0, void *stream) {
  if (!d) { gerr("null descriptor"); return IONODE_ERR_ARG; }
  if (d->model != IONODE_MODEL_HH2 && d->model != IONODE_MODEL_MARKOV6) {
    gerr("ionode_dopri5_backward_sse: closed-form models only (HH 2-state, 6-state)"); return IONODE_ERR_UNSUPPORTED;
  }
  if (d->traj_per_image > 0) { gerr("ionode_dopri5_backward_sse: traj_per_image must be 0"); return IONODE_ERR_UNSUPPORTED; }
  if (!desc_consistent(d)) { gerr("inconsistent descriptor"); return IONODE_ERR_ARG; }
  if (!d->sse_ref || !grad_sse || !d->ckpt || d->ckpt_cap < 1 || !params || !prot_v || !t_eval || !n_accepted || !state || !grad_params || !grad_y0) {
    gerr("ionode_dopri5_backward_sse: required buffer is NULL (sse_ref / ckpt / ckpt_cap come from the descriptor)"); return IONODE_ERR_ARG;
  }
  if (bad_range(it_begin, it_end, n_iter)) { gerr("bad iteration range"); return IONODE_ERR_ARG; }
  GArgs a = fill_args(d, 0, 16, it_begin, it_end, n_iter, params, prot_v, prot_t, prot_of_traj, t_eval, n_accepted, state, grad_params, grad_y0);
  a.grad_sse = grad_sse; a.sse_ref = d->sse_ref; a.v_tab = d->v_at_outputs;
  a.obs_g = d->obs_g; a.obs_e = d->obs_e; a.obs_open = d->obs_open_state_only ? 1 : 0;
  SweepFn fn = is_m6(d) ? closed_sweep_sse<IONODE_MODEL_MARKOV6>(d->state_f32) : closed_sweep_sse<IONODE_MODEL_HH2>(d->state_f32);
  return launch(fn, a, ionode::grad_closed_lds_bytes(d->n_state), stream);
}

size_t ionode_grad_packet_doubles(void) { return (size_t)16 * ionode::GRAD_PACKET; }

int ionode_dopri5_backward_recompute(const ionode_desc *d, int32_t it_begin, int32_t it_end, int32_t n_iter, const float *grad_image,
                                     const double *params, const double *prot_v, const double *prot_t, const int32_t *prot_of_traj,
                                     const double *t_eval, const int32_t *n_accepted, const void *grad_y, float *records,
                                     double *packets, void *stream) {
  return backward_impl(Sweep::Recompute, d, it_begin, it_end, n_iter, grad_image, params, prot_v, prot_t, prot_of_traj, t_eval, n_accepted, grad_y,
                       nullptr, records, packets, nullptr, nullptr, stream);
}

int ionode_dopri5_backward_sweep(const ionode_desc *d, int32_t it_begin, int32_t it_end, int32_t n_iter, const float *grad_image,
                                 const double *params, const double *prot_v, const double *prot_t, const int32_t *prot_of_traj,
                                 const double *t_eval, const int32_t *n_accepted, const void *grad_y, double *state,
                                 float *records, const double *packets, double *grad_params, double *grad_y0,
                                 void *stream) {
  return backward_impl(Sweep::Walk, d, it_begin, it_end, n_iter, grad_image, params, prot_v, prot_t, prot_of_traj, t_eval, n_accepted, grad_y,
                       state, records, const_cast<double *>(packets), grad_params, grad_y0, stream);
}

// ---- the fused sum-of-squares objective on the two-phase sweep (NN-f / NN-d) ----
// what the three entry points check first, in ionode_dopri5_backward_sse's order; nothing is launched before it passes
static int sse_nn_check(const char *who, const ionode_desc *d, int32_t it_begin, int32_t it_end, int32_t n_iter) {
  char m[200];
  if (!d) { gerr("null descriptor"); return IONODE_ERR_ARG; }
  if (d->model != IONODE_MODEL_NNF && d->model != IONODE_MODEL_NND) {
    snprintf(m, sizeof m, "%s: NN-f / NN-d only (closed-form models: ionode_dopri5_backward_sse)", who); gerr(m); return IONODE_ERR_UNSUPPORTED;
  }
  if (d->traj_per_image > 0) { snprintf(m, sizeof m, "%s: traj_per_image must be 0", who); gerr(m); return IONODE_ERR_UNSUPPORTED; }
  if (!desc_consistent(d)) { gerr("inconsistent descriptor"); return IONODE_ERR_ARG; }
  if (!d->sse_ref || !d->ckpt || d->ckpt_cap < 1) {
    snprintf(m, sizeof m, "%s: required buffer is NULL (sse_ref / ckpt / ckpt_cap come from the descriptor)", who); gerr(m); return IONODE_ERR_ARG;
  }
  if (bad_range(it_begin, it_end, n_iter)) { gerr("bad iteration range"); return IONODE_ERR_ARG; }
  if (d->mlp_layers < 1 || d->mlp_width < 1) { gerr("bad MLP shape"); return IONODE_ERR_ARG; }
  const int NT = np_of(d->mlp_width) / 16;
  if (!find_sweep(Sweep::Walk, d->model, d->state_f32 ? 1 : 0, NT) || d->mlp_layers > 15 ||
      ionode::grad_lds_bytes(d->mlp_layers, NT) + 16 + ionode::grad_walk_lds_bytes() > 160 * 1024) {
    gerr("backward sweep: (L, N) outside the compiled variants (N pads to 16, 112, 208 or 512; at most 15 hidden layers)");
    return IONODE_ERR_UNSUPPORTED;
  }
  return IONODE_OK;
}

int ionode_dopri5_backward_sse_gc(const ionode_desc *d, int32_t it_begin, int32_t it_end, int32_t n_iter, const double *prot_v,
                                  const double *prot_t, const int32_t *prot_of_traj, const double *t_eval, const int32_t *n_accepted,
                                  const double *grad_sse, double *packets, double *sse_grad_y0, void *stream) {
  const int rc = sse_nn_check("ionode_dopri5_backward_sse_gc", d, it_begin, it_end, n_iter);
  if (rc != IONODE_OK) return rc;
  if (!grad_sse || !prot_v || !t_eval || !n_accepted || !packets || !sse_grad_y0) {
    gerr("ionode_dopri5_backward_sse_gc: required buffer is NULL"); return IONODE_ERR_ARG;
  }
  if ((int64_t)it_end - it_begin > (int64_t)65535 * ionode::GRAD_GC_WAVES) {
    gerr("ionode_dopri5_backward_sse_gc: at most 65535 x 4 iterations per launch (HIP's grid.y limit): split the range"); return IONODE_ERR_ARG;
  }
  GArgs a = fill_args(d, d->mlp_layers, np_of(d->mlp_width), it_begin, it_end, n_iter, nullptr, prot_v, prot_t, prot_of_traj, t_eval, n_accepted,
                      nullptr, nullptr, nullptr);
  a.packets = packets; a.sse_y0 = sse_grad_y0;
  a.grad_sse = grad_sse; a.sse_ref = d->sse_ref; a.v_tab = d->v_at_outputs;
  a.obs_g = d->obs_g; a.obs_e = d->obs_e; a.obs_open = d->obs_open_state_only ? 1 : 0;
  return launch(sse_gc(d->state_f32), a, 0, stream);
}

int ionode_dopri5_backward_recompute_sse(const ionode_desc *d, int32_t it_begin, int32_t it_end, int32_t n_iter, const float *grad_image,
                                         const double *params, const double *prot_v, const double *prot_t, const int32_t *prot_of_traj,
                                         const double *t_eval, const int32_t *n_accepted, float *records, double *packets, void *stream) {
  const int rc = sse_nn_check("ionode_dopri5_backward_recompute_sse", d, it_begin, it_end, n_iter);
  if (rc != IONODE_OK) return rc;
  return backward_impl(Sweep::Recompute, d, it_begin, it_end, n_iter, grad_image, params, prot_v, prot_t, prot_of_traj, t_eval, n_accepted, nullptr,
                       nullptr, records, packets, nullptr, nullptr, stream, true, nullptr);
}

int ionode_dopri5_backward_sweep_sse(const ionode_desc *d, int32_t it_begin, int32_t it_end, int32_t n_iter, const float *grad_image,
                                     const double *params, const double *prot_v, const double *prot_t, const int32_t *prot_of_traj,
                                     const double *t_eval, const int32_t *n_accepted, const double *sse_grad_y0, double *state,
                                     float *records, const double *packets, double *grad_params, double *grad_y0, void *stream) {
  const int rc = sse_nn_check("ionode_dopri5_backward_sweep_sse", d, it_begin, it_end, n_iter);
  if (rc != IONODE_OK) return rc;
  return backward_impl(Sweep::Walk, d, it_begin, it_end, n_iter, grad_image, params, prot_v, prot_t, prot_of_traj, t_eval, n_accepted, nullptr,
                       state, records, const_cast<double *>(packets), grad_params, grad_y0, stream, true, sse_grad_y0);
}

static int reduce_impl(int32_t L, int32_t N, const float *records, int64_t n_records, int32_t n_slabs, float *partials, void *stream,
                       int unit_seed) {
  if (!records || !partials || n_records < 1 || n_slabs < 1 || L < 1 || N < 1) { gerr("ionode_grad_reduce: bad argument"); return IONODE_ERR_ARG; }
  const int NT = np_of(N) / 16;
  const hipError_t e = ionode::launch_grad_reduce(L, NT, records, n_records, n_slabs, partials, reinterpret_cast<hipStream_t>(stream), unit_seed);
  if (e == hipErrorInvalidValue) { gerr("ionode_grad_reduce: width outside the compiled variants"); return IONODE_ERR_UNSUPPORTED; }
  if (e != hipSuccess) { gerr(hipGetErrorString(e)); return IONODE_ERR_LAUNCH; }
  return IONODE_OK;
}

int32_t ionode_grad_reduce_slabs(int32_t L, int32_t N, int64_t n_records) {
  if (L < 1 || N < 1 || n_records < 1) return 1;
  int dev = 0, cus = 0;
  if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 1) {
    (void)hipGetLastError();
    cus = 256;   // (no device: the plan of an unpartitioned MI355X)
  }
  return ionode::grad_reduce_slabs(L, np_of(N) / 16, cus, n_records);
}

int ionode_grad_reduce(int32_t L, int32_t N, const float *records, int64_t n_records, int32_t n_slabs, float *partials,
                       void *stream) {
  return reduce_impl(L, N, records, n_records, n_slabs, partials, stream, 0);
}

int ionode_grad_reduce_unit(int32_t L, int32_t N, const float *records, int64_t n_records, int32_t n_slabs, float *partials,
                            void *stream) {
  return reduce_impl(L, N, records, n_records, n_slabs, partials, stream, 1);
}

int ionode_regress_step(int32_t L, int32_t N, const float *grad_image, const float *x, const float *offset, const float *y,
                        int32_t n_rows, float netscale, float *records, double *loss_partials, int32_t n_workgroups,
                        void *stream) {
  if (!grad_image || !x || !y || !records || !loss_partials || n_rows < 1 || n_workgroups < 1 || L < 1 || N < 1) {
    gerr("ionode_regress_step: bad argument"); return IONODE_ERR_ARG;
  }
  const int NT = np_of(N) / 16;
  if (ionode::grad_lds_bytes(L, NT) > 160 * 1024 || L > 15) { gerr("ionode_regress_step: (L, N) outside the compiled variants (at most 15 hidden layers)"); return IONODE_ERR_UNSUPPORTED; }
  ionode::RArgs a;
  memset(&a, 0, sizeof a);
  a.img = grad_image; a.x = x; a.y = y; a.offset = offset; a.records = records; a.loss_part = loss_partials;
  a.M = n_rows; a.L = L; a.N = N; a.NT = NT; a.record_floats = ionode::grad_record_floats(L, NT); a.netscale = netscale;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (!ionode::for_width(NT, [&](auto nt) { ionode::launch_regress<decltype(nt)::value>(a, (unsigned)n_workgroups, s); },
                         [&] { ionode::launch_regress32(a, (unsigned)n_workgroups, s); })) {
    gerr("ionode_regress_step: width outside the compiled variants (N pads to 16, 112, 208 or 512)"); return IONODE_ERR_UNSUPPORTED;
  }
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) { gerr(hipGetErrorString(e)); return IONODE_ERR_LAUNCH; }
  return IONODE_OK;
}

int ionode_adam_step(int32_t n_params, int32_t n_slabs, int32_t L, int32_t N, const float *partials, const int32_t *padmap,
                     float *weights, float *exp_avg, float *exp_avg_sq, float lr, float beta1, float beta2, float eps,
                     int32_t step, float *grad_out, int32_t apply, void *stream) {
  if (!partials || !padmap || n_params < 1 || n_slabs < 1 || step < 1 || (apply && (!weights || !exp_avg || !exp_avg_sq))) {
    gerr("ionode_adam_step: bad argument"); return IONODE_ERR_ARG;
  }
  const float bc1 = 1.0f - powf(beta1, (float)step);
  const float bc2_sqrt = sqrtf(1.0f - powf(beta2, (float)step));
  const size_t partf = ionode::grad_partial_floats(L, np_of(N) / 16);
  hipLaunchKernelGGL(ionode::ionode_adam_kernel, dim3((n_params + 255) / 256), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                     n_params, n_slabs, partf, partials, padmap, weights, exp_avg, exp_avg_sq, lr, beta1, beta2, eps, bc1, bc2_sqrt,
                     grad_out, apply);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) { gerr(hipGetErrorString(e)); return IONODE_ERR_LAUNCH; }
  return IONODE_OK;
}

int ionode_image_refresh(int32_t L, int32_t N, const int32_t *image_map, const float *weights, float *grad_image, void *stream) {
  if (!image_map || !weights || !grad_image || L < 1 || N < 1) { gerr("ionode_image_refresh: bad argument"); return IONODE_ERR_ARG; }
  const size_t n = ionode::grad_img_floats(L, np_of(N) / 16);
  hipLaunchKernelGGL(ionode::ionode_image_refresh_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), n, image_map, weights, grad_image);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) { gerr(hipGetErrorString(e)); return IONODE_ERR_LAUNCH; }
  return IONODE_OK;
}

size_t ionode_grad_partial_floats(int32_t L, int32_t N) {
  if (L < 1 || N < 1) return 0;
  return ionode::grad_partial_floats(L, np_of(N) / 16);
}

}  // extern "C"
