// ionode_grad_capi.hip -- C ABI of the gradient path (include/ionode.h, "gradients through the solve"): the grad image
// packer, the backward-sweep launcher and the weight-gradient reduction launcher.
#include <cstdarg>
#include <cstdio>
#include <cstring>

#include "ionode_grad_launch.hpp"
#include "ionode_grad_reduce.hpp"
#include "ionode_grad_gen_plan.hpp"
#include "ionode_host.hpp"
#include "ionode_tangent.hpp"
#include "ionode_tangent_nn.hpp"

#include "ionode_step_capi.hpp"

namespace {
thread_local char g_gerr[256] = "";
}  // namespace

// sets ionode_grad_last_error(), returns rc (declared in ionode_step_capi.hpp: the optimiser steps' units refuse through it too)
int ionode::refuse(int rc, const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_gerr, sizeof g_gerr, fmt, ap);
  va_end(ap);
  return rc;
}

namespace {

using ionode::refuse;
void gerr(const char *m) { refuse(0, "%s", m); }

inline int np_of(int N) { return 16 * ((N + 15) / 16); }

using ionode::GArgs;
using ionode::Sweep;
using ionode::SweepFn;

// launchers that have no width: the closed-form models' sweeps (NT = 1, unused), the NN models' walk and their G_c kernel
template <int MODEL> SweepFn closed_sweep(int f32) { return f32 ? &ionode::launch_sweep<MODEL, float, 1> : &ionode::launch_sweep<MODEL, double, 1>; }
template <int MODEL> SweepFn closed_sweep_sse(int f32) { return f32 ? &ionode::launch_sweep_sse<MODEL, float> : &ionode::launch_sweep_sse<MODEL, double>; }
inline SweepFn sse_gc(int f32) { return f32 ? &ionode::launch_sse_gc<float> : &ionode::launch_sse_gc<double>; }
template <int MODEL> SweepFn walk(int f32) { return f32 ? &ionode::launch_walk<MODEL, float> : &ionode::launch_walk<MODEL, double>; }

inline bool is_m6(const ionode_desc *d) { return d->model == IONODE_MODEL_MARKOV6; }
inline bool is_nn(const ionode_desc *d) { return d->model == IONODE_MODEL_NNF || d->model == IONODE_MODEL_NND; }
inline bool desc_consistent(const ionode_desc *d) {
  const bool m6 = is_m6(d);
  return !(d->n_state != (m6 ? 6 : 2) || d->n_traj < 1 || d->n_out < 1 || d->n_prot < 1 || d->prot_n < 2 || d->n_params < (m6 ? 12 : 8) || !(d->prot_dt > 0));
}

// nullptr: no variant of that width (a width without a sweep has no walk and no G_c launch either, though those kernels have no width)
// (Not a correctness rule: the branches may come in any order.  This one -- walk, sweep / recompute, closed-form, G_c -- is the order
// the launchers were first used in before, so the kernels are emitted where they were and the code objects compare equal byte for byte.)
SweepFn find_sweep(Sweep which, const ionode_desc *d, int NT) {
  const int f32 = d->state_f32 ? 1 : 0;
  const bool nn = is_nn(d), m6 = is_m6(d);
  if (nn && which == Sweep::Walk) {
    if (!ionode::for_width(NT, [](auto) {}, [] {})) return nullptr;
    return d->model == IONODE_MODEL_NNF ? walk<IONODE_MODEL_NNF>(f32) : walk<IONODE_MODEL_NND>(f32);
  }
  if (nn && which != Sweep::SseGc) {
    const bool recompute = which == Sweep::Recompute;
    SweepFn fn = nullptr;
    ionode::for_width(NT, [&](auto nt) { fn = ionode::pick_sweep<decltype(nt)::value>(recompute, d->model, f32); },
                      [&] { fn = ionode::pick_sweep32(recompute, d->model, f32); });   // inst_grad32.hip
    return fn;
  }
  if (!nn && which != Sweep::ClosedSse) return m6 ? closed_sweep<IONODE_MODEL_MARKOV6>(f32) : closed_sweep<IONODE_MODEL_HH2>(f32);
  if (!nn) return m6 ? closed_sweep_sse<IONODE_MODEL_MARKOV6>(f32) : closed_sweep_sse<IONODE_MODEL_HH2>(f32);
  return ionode::for_width(NT, [](auto) {}, [] {}) ? sse_gc(f32) : nullptr;
}

// ---- the seven sweep entry points: one block of named arguments, one Entry row each, one checked launch ----
// What an entry point received, by the names of include/ionode.h; what it does not have stays NULL.
struct Buffers {
  int32_t it_begin, it_end, n_iter;
  const float *grad_image;
  const double *params, *prot_v, *prot_t;
  const int32_t *prot_of_traj;
  const double *t_eval;
  const int32_t *n_accepted;
  const void *grad_y;
  const double *grad_sse;
  double *sse_grad_y0, *state;
  float *records;
  double *packets, *grad_params, *grad_y0;
  void *stream;
};

enum class Family { Any, Closed, NN };
// Where the checks that move sit (checked_launch writes the order down); tests/golden/grad_entry_checks.json pins all three.
//   Oldest     packets, then the family; buffers before the range, grid.y behind it; traj_per_image behind those
//   SseClosed  family, traj_per_image; buffers before the range
//   SseNN      family, traj_per_image; packets, buffers and grid.y last, behind the MLP shape
enum class Order { Oldest, SseClosed, SseNN };

constexpr const char *OLDEST_NULL = "ionode_dopri5_backward: required buffer is NULL (ckpt / ckpt_cap come from the descriptor)";
constexpr const char *SSE_NULL = "%s: required buffer is NULL (sse_ref / ckpt / ckpt_cap come from the descriptor)";
constexpr const char *RECOMPUTE = "ionode_dopri5_backward_recompute";

struct Entry {
  const char *name;          // in messages
  Family family;             // the models it serves
  Order order;
  Sweep launch;              // how find_sweep picks the launcher; the LDS bytes follow the model (closed-form: G_c scratch, NN: the net's; SseGc: none)
  bool sse_ref;              // reads d->sse_ref: the sum-of-squares fields of GArgs are filled
  const char *grid_y_who;    // grid.y = ceil(iterations / 4), at most 65535 x 4 iterations per launch: the name its refusal carries; nullptr: no cap
  const char *buffers_null;  // the text for a missing pointer argument (%s: name); the _sse forms of recompute and walk answer as those do
  bool (*has_buffers)(const Buffers &);   // its required pointers beyond prot_v, t_eval, n_accepted (all), grad_image (NN models, every
                                          // launch but SseGc) and packets (Recompute, Walk)
};
static_assert(ionode::GRAD_RECOMPUTE_IB == 4 && ionode::GRAD_GC_WAVES == 4, "Entry::grid_y_who");

inline bool adjoint(const Buffers &b) { return b.state && b.grad_params && b.grad_y0; }   // a launch that reads and writes the adjoint state
const Entry BACKWARD = {"ionode_dopri5_backward", Family::Any, Order::Oldest, Sweep::OnePhase, false, nullptr, OLDEST_NULL,
                        [](const Buffers &b) { return b.params && b.grad_y && adjoint(b); }};
const Entry BACKWARD_SSE = {"ionode_dopri5_backward_sse", Family::Closed, Order::SseClosed, Sweep::ClosedSse, true, nullptr, SSE_NULL,
                            [](const Buffers &b) { return b.params && b.grad_sse && adjoint(b); }};
const Entry BACKWARD_RECOMPUTE = {RECOMPUTE, Family::NN, Order::Oldest, Sweep::Recompute, false, RECOMPUTE, OLDEST_NULL,
                                  [](const Buffers &b) { return b.params && b.grad_y; }};
const Entry BACKWARD_SWEEP = {"ionode_dopri5_backward_sweep", Family::NN, Order::Oldest, Sweep::Walk, false, nullptr, OLDEST_NULL,
                              [](const Buffers &b) { return b.params && b.grad_y && adjoint(b); }};
const Entry SSE_GC = {"ionode_dopri5_backward_sse_gc", Family::NN, Order::SseNN, Sweep::SseGc, true, "ionode_dopri5_backward_sse_gc",
                      "%s: required buffer is NULL", [](const Buffers &b) { return b.grad_sse && b.packets && b.sse_grad_y0; }};
const Entry RECOMPUTE_SSE = {"ionode_dopri5_backward_recompute_sse", Family::NN, Order::SseNN, Sweep::Recompute, true, RECOMPUTE, OLDEST_NULL,
                             [](const Buffers &b) { return b.params != nullptr; }};
const Entry SWEEP_SSE = {"ionode_dopri5_backward_sweep_sse", Family::NN, Order::SseNN, Sweep::Walk, true, nullptr, OLDEST_NULL,
                         [](const Buffers &b) { return b.params && b.sse_grad_y0 && adjoint(b); }};

int checked_launch(const Entry &e, const ionode_desc *d, const Buffers &b, int obj_abs = 0) {
  constexpr const char *TWO_PHASE = "two-phase sweep: NN-f / NN-d only, `packets` required";
  constexpr const char *VARIANTS = "backward sweep: (L, N) outside the compiled variants (N pads to 16, 112, 208 or 512; at most 15 hidden layers)";
  if (!d) return refuse(IONODE_ERR_ARG, "null descriptor");
  const bool oldest = e.order == Order::Oldest, last = e.order == Order::SseNN;
  const bool nn = is_nn(d), two_phase = e.launch == Sweep::Recompute || e.launch == Sweep::Walk;
  // the three checks whose place depends on e.order
  auto packets = [&] { return two_phase && !b.packets ? refuse(IONODE_ERR_ARG, TWO_PHASE) : 0; };
  auto buffers = [&] {
    if (b.prot_v && b.t_eval && b.n_accepted && (b.grad_image || !nn || e.launch == Sweep::SseGc) && e.has_buffers(b)) return 0;
    return refuse(IONODE_ERR_ARG, e.buffers_null, e.name);
  };
  auto grid_y = [&] {
    if (!e.grid_y_who || (int64_t)b.it_end - b.it_begin <= (int64_t)65535 * 4) return 0;
    return refuse(IONODE_ERR_ARG, "%s: at most 65535 x 4 iterations per launch (HIP's grid.y limit): split the range", e.grid_y_who);
  };
  auto one_image = [&] {
    if (d->traj_per_image <= 0) return 0;
    return oldest ? refuse(IONODE_ERR_UNSUPPORTED, "backward sweep: one weight set per launch (traj_per_image must be 0)")
                  : refuse(IONODE_ERR_UNSUPPORTED, "%s: traj_per_image must be 0", e.name);
  };
  int rc;
  if (!last && (rc = packets())) return rc;
  if (e.family == Family::NN && !nn)
    return oldest ? refuse(IONODE_ERR_ARG, TWO_PHASE) : refuse(IONODE_ERR_UNSUPPORTED, "%s: NN-f / NN-d only (closed-form models: ionode_dopri5_backward_sse)", e.name);
  if (e.family == Family::Closed && d->model != IONODE_MODEL_HH2 && !is_m6(d)) return refuse(IONODE_ERR_UNSUPPORTED, "%s: closed-form models only (HH 2-state, 6-state)", e.name);
  if (!oldest && (rc = one_image())) return rc;
  if (d->model < 0 || d->model > 3) return refuse(IONODE_ERR_UNSUPPORTED, "backward sweep: unknown model");
  if (!desc_consistent(d)) return refuse(IONODE_ERR_ARG, "inconsistent descriptor");
  if ((e.sse_ref && !d->sse_ref) || !d->ckpt || d->ckpt_cap < 1) return oldest ? refuse(IONODE_ERR_ARG, OLDEST_NULL) : refuse(IONODE_ERR_ARG, SSE_NULL, e.name);
  if (!last && (rc = buffers())) return rc;
  if (b.it_begin < 0 || b.it_end <= b.it_begin || b.it_end > b.n_iter) return refuse(IONODE_ERR_ARG, "bad iteration range");
  if (!last && (rc = grid_y())) return rc;
  if (oldest && (rc = one_image())) return rc;
  if (nn && (d->mlp_layers < 1 || d->mlp_width < 1)) return refuse(IONODE_ERR_ARG, "bad MLP shape");
  const int NP = nn ? np_of(d->mlp_width) : 16, NT = NP / 16, L = nn ? d->mlp_layers : 0;   // closed-form models: (0, 16)
  const SweepFn fn = find_sweep(e.launch, d, NT);
  const size_t net_lds = ionode::grad_lds_bytes(L, NT), walk_lds = net_lds + 16 + ionode::grad_walk_lds_bytes();   // (what a recompute launch's walk needs)
  const size_t lds = !nn ? ionode::grad_closed_lds_bytes(d->n_state) : e.launch == Sweep::SseGc ? 0 : net_lds;
  if (!fn || L > 15 || (nn && (oldest ? net_lds : walk_lds) > 160 * 1024)) return refuse(IONODE_ERR_UNSUPPORTED, VARIANTS);
  if (two_phase && walk_lds > 160 * 1024) return refuse(IONODE_ERR_UNSUPPORTED, "two-phase sweep: LDS");
  if (last && ((rc = packets()) || (rc = buffers()) || (rc = grid_y()))) return rc;

  GArgs a;
  memset(&a, 0, sizeof a);
  a.k.params = b.params; a.k.prot_v = b.prot_v; a.k.prot_t = b.prot_t; a.k.prot_of_traj = b.prot_of_traj; a.k.t_eval = b.t_eval;
  a.k.B = d->n_traj; a.k.Nt = d->n_out; a.k.P = d->n_prot; a.k.Np = d->prot_n; a.k.n_params = d->n_params;
  a.k.L = L; a.k.N = d->mlp_width; a.k.NP = NP; a.k.NT = NT;
  a.k.prot_t0 = d->prot_t0; a.k.prot_dt = d->prot_dt; a.k.prot_rdt = 1.0 / d->prot_dt; a.k.v_oob = d->v_oob;
  a.img = b.grad_image; a.ckpt = d->ckpt; a.ckpt_cap = d->ckpt_cap; a.nacc = b.n_accepted; a.grad_y = b.grad_y; a.state = b.state;
  a.records = nn ? b.records : nullptr; a.record_floats = ionode::grad_record_floats(L, NT); a.packets = b.packets;
  a.grad_params = b.grad_params; a.grad_y0 = b.grad_y0; a.sse_y0 = b.sse_grad_y0;
  a.it_begin = b.it_begin; a.it_end = b.it_end; a.n_iter = b.n_iter;
  if (e.sse_ref) {
    a.grad_sse = b.grad_sse; a.sse_ref = d->sse_ref; a.v_tab = d->v_at_outputs;
    a.obs_g = d->obs_g; a.obs_e = d->obs_e; a.obs_open = d->obs_open_state_only ? 1 : 0;
    a.k.obj_abs = obj_abs;   // (the kind of the fused objective: read by the two kernels that form the residuals' weights)
  }
  fn(a, (unsigned)((a.k.B + 15) / 16), lds, reinterpret_cast<hipStream_t>(b.stream));
  const hipError_t err = hipGetLastError();
  if (err != hipSuccess) return refuse(IONODE_ERR_LAUNCH, "%s", hipGetErrorString(err));
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

// The sweep entry points (include/ionode.h): each names what it received and hands it to checked_launch with its row of the table above.
int ionode_dopri5_backward(const ionode_desc *d, int32_t it_begin, int32_t it_end, int32_t n_iter, const float *grad_image,
                           const double *params, const double *prot_v, const double *prot_t, const int32_t *prot_of_traj,
                           const double *t_eval, const int32_t *n_accepted, const void *grad_y, double *state,
                           float *records, double *grad_params, double *grad_y0, void *stream) {
  Buffers b = {};
  b.it_begin = it_begin; b.it_end = it_end; b.n_iter = n_iter; b.grad_image = grad_image; b.params = params; b.prot_v = prot_v;
  b.prot_t = prot_t; b.prot_of_traj = prot_of_traj; b.t_eval = t_eval; b.n_accepted = n_accepted; b.grad_y = grad_y; b.state = state;
  b.records = records; b.grad_params = grad_params; b.grad_y0 = grad_y0; b.stream = stream;
  return checked_launch(BACKWARD, d, b);
}

int ionode_dopri5_backward_sse(const ionode_desc *d, int32_t it_begin, int32_t it_end, int32_t n_iter, const double *params,
                               const double *prot_v, const double *prot_t, const int32_t *prot_of_traj, const double *t_eval,
                               const int32_t *n_accepted, const double *grad_sse, double *state, double *grad_params,
                               double *grad_y0, void *stream) {
  Buffers b = {};
  b.it_begin = it_begin; b.it_end = it_end; b.n_iter = n_iter; b.params = params; b.prot_v = prot_v; b.prot_t = prot_t;
  b.prot_of_traj = prot_of_traj; b.t_eval = t_eval; b.n_accepted = n_accepted; b.grad_sse = grad_sse; b.state = state;
  b.grad_params = grad_params; b.grad_y0 = grad_y0; b.stream = stream;
  return checked_launch(BACKWARD_SSE, d, b);
}

size_t ionode_grad_packet_doubles(void) { return (size_t)16 * ionode::GRAD_PACKET; }

// Phase A (the unit-seed products and packets of every (tile, step)) carries no adjoint state; phase B is the walk.
int ionode_dopri5_backward_recompute(const ionode_desc *d, int32_t it_begin, int32_t it_end, int32_t n_iter, const float *grad_image,
                                     const double *params, const double *prot_v, const double *prot_t, const int32_t *prot_of_traj,
                                     const double *t_eval, const int32_t *n_accepted, const void *grad_y, float *records,
                                     double *packets, void *stream) {
  Buffers b = {};
  b.it_begin = it_begin; b.it_end = it_end; b.n_iter = n_iter; b.grad_image = grad_image; b.params = params; b.prot_v = prot_v;
  b.prot_t = prot_t; b.prot_of_traj = prot_of_traj; b.t_eval = t_eval; b.n_accepted = n_accepted; b.grad_y = grad_y;
  b.records = records; b.packets = packets; b.stream = stream;
  return checked_launch(BACKWARD_RECOMPUTE, d, b);
}

int ionode_dopri5_backward_sweep(const ionode_desc *d, int32_t it_begin, int32_t it_end, int32_t n_iter, const float *grad_image,
                                 const double *params, const double *prot_v, const double *prot_t, const int32_t *prot_of_traj,
                                 const double *t_eval, const int32_t *n_accepted, const void *grad_y, double *state,
                                 float *records, const double *packets, double *grad_params, double *grad_y0,
                                 void *stream) {
  Buffers b = {};
  b.it_begin = it_begin; b.it_end = it_end; b.n_iter = n_iter; b.grad_image = grad_image; b.params = params; b.prot_v = prot_v;
  b.prot_t = prot_t; b.prot_of_traj = prot_of_traj; b.t_eval = t_eval; b.n_accepted = n_accepted; b.grad_y = grad_y; b.state = state;
  b.records = records; b.packets = const_cast<double *>(packets); b.grad_params = grad_params; b.grad_y0 = grad_y0; b.stream = stream;
  return checked_launch(BACKWARD_SWEEP, d, b);
}

// ---- the fused sum-of-squares objective on the two-phase sweep (NN-f / NN-d) ----
int ionode_dopri5_backward_sse_gc(const ionode_desc *d, int32_t it_begin, int32_t it_end, int32_t n_iter, const double *prot_v,
                                  const double *prot_t, const int32_t *prot_of_traj, const double *t_eval, const int32_t *n_accepted,
                                  const double *grad_sse, double *packets, double *sse_grad_y0, void *stream) {
  Buffers b = {};
  b.it_begin = it_begin; b.it_end = it_end; b.n_iter = n_iter; b.prot_v = prot_v; b.prot_t = prot_t; b.prot_of_traj = prot_of_traj;
  b.t_eval = t_eval; b.n_accepted = n_accepted; b.grad_sse = grad_sse; b.packets = packets; b.sse_grad_y0 = sse_grad_y0; b.stream = stream;
  return checked_launch(SSE_GC, d, b);
}

int ionode_dopri5_backward_recompute_sse(const ionode_desc *d, int32_t it_begin, int32_t it_end, int32_t n_iter, const float *grad_image,
                                         const double *params, const double *prot_v, const double *prot_t, const int32_t *prot_of_traj,
                                         const double *t_eval, const int32_t *n_accepted, float *records, double *packets, void *stream) {
  Buffers b = {};
  b.it_begin = it_begin; b.it_end = it_end; b.n_iter = n_iter; b.grad_image = grad_image; b.params = params; b.prot_v = prot_v;
  b.prot_t = prot_t; b.prot_of_traj = prot_of_traj; b.t_eval = t_eval; b.n_accepted = n_accepted; b.records = records;
  b.packets = packets; b.stream = stream;
  return checked_launch(RECOMPUTE_SSE, d, b);
}

int ionode_dopri5_backward_sweep_sse(const ionode_desc *d, int32_t it_begin, int32_t it_end, int32_t n_iter, const float *grad_image,
                                     const double *params, const double *prot_v, const double *prot_t, const int32_t *prot_of_traj,
                                     const double *t_eval, const int32_t *n_accepted, const double *sse_grad_y0, double *state,
                                     float *records, const double *packets, double *grad_params, double *grad_y0, void *stream) {
  Buffers b = {};
  b.it_begin = it_begin; b.it_end = it_end; b.n_iter = n_iter; b.grad_image = grad_image; b.params = params; b.prot_v = prot_v;
  b.prot_t = prot_t; b.prot_of_traj = prot_of_traj; b.t_eval = t_eval; b.n_accepted = n_accepted;
  b.sse_grad_y0 = const_cast<double *>(sse_grad_y0); b.state = state; b.records = records; b.packets = const_cast<double *>(packets);
  b.grad_params = grad_params; b.grad_y0 = grad_y0; b.stream = stream;
  return checked_launch(SWEEP_SSE, d, b);
}

// ---- the fused objective of either kind (IONODE_OBJECTIVE_*): the two launches that form the residuals' adjoint weights ----
// The kind is checked first, as ionode_dopri5_objective checks it; everything else is the squares' entry point's row and checks.
static int objective_kind(const char *who, int32_t objective) {
  if (objective == IONODE_OBJECTIVE_SSE || objective == IONODE_OBJECTIVE_SAE) return 0;
  return refuse(IONODE_ERR_ARG, "%s: objective must be IONODE_OBJECTIVE_SSE (0) or IONODE_OBJECTIVE_SAE (1)", who);
}

int ionode_objective_backward(const ionode_desc *d, int32_t objective, int32_t it_begin, int32_t it_end, int32_t n_iter, const double *params,
                              const double *prot_v, const double *prot_t, const int32_t *prot_of_traj, const double *t_eval,
                              const int32_t *n_accepted, const double *grad_sse, double *state, double *grad_params,
                              double *grad_y0, void *stream) {
  if (const int rc = objective_kind("ionode_objective_backward", objective)) return rc;
  Buffers b = {};
  b.it_begin = it_begin; b.it_end = it_end; b.n_iter = n_iter; b.params = params; b.prot_v = prot_v; b.prot_t = prot_t;
  b.prot_of_traj = prot_of_traj; b.t_eval = t_eval; b.n_accepted = n_accepted; b.grad_sse = grad_sse; b.state = state;
  b.grad_params = grad_params; b.grad_y0 = grad_y0; b.stream = stream;
  return checked_launch(BACKWARD_SSE, d, b, objective == IONODE_OBJECTIVE_SAE ? 1 : 0);
}

int ionode_objective_backward_gc(const ionode_desc *d, int32_t objective, int32_t it_begin, int32_t it_end, int32_t n_iter, const double *prot_v,
                                 const double *prot_t, const int32_t *prot_of_traj, const double *t_eval, const int32_t *n_accepted,
                                 const double *grad_sse, double *packets, double *sse_grad_y0, void *stream) {
  if (const int rc = objective_kind("ionode_objective_backward_gc", objective)) return rc;
  Buffers b = {};
  b.it_begin = it_begin; b.it_end = it_end; b.n_iter = n_iter; b.prot_v = prot_v; b.prot_t = prot_t; b.prot_of_traj = prot_of_traj;
  b.t_eval = t_eval; b.n_accepted = n_accepted; b.grad_sse = grad_sse; b.packets = packets; b.sse_grad_y0 = sse_grad_y0; b.stream = stream;
  return checked_launch(SSE_GC, d, b, objective == IONODE_OBJECTIVE_SAE ? 1 : 0);
}

static int reduce_impl(int32_t L, int32_t N, const float *records, int64_t n_records, int32_t n_slabs, float *partials, void *stream,
                       int unit_seed) {
  if (!records || !partials || n_records < 1 || n_slabs < 1 || L < 1 || N < 1) { gerr("ionode_grad_reduce: bad argument"); return IONODE_ERR_ARG; }
  if (N > 512) return refuse(IONODE_ERR_UNSUPPORTED, "ionode_grad_reduce: width outside the served shapes (N <= 512)");   // (no depth limit: the kernels have none)
  const int NT = np_of(N) / 16;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  // the tuned instantiation where for_width has one, the run-time-width kernel (inst_grad_gen.hip) otherwise or when forced
  const hipError_t e = ionode::grad_use_gen(NT) ? ionode::launch_grad_reduce_gen(L, NT, records, n_records, n_slabs, partials, s, unit_seed)
                                                : ionode::launch_grad_reduce(L, NT, records, n_records, n_slabs, partials, s, unit_seed);
  if (e != hipSuccess) { gerr(hipGetErrorString(e)); return IONODE_ERR_LAUNCH; }
  return IONODE_OK;
}

int32_t ionode_grad_reduce_slabs(int32_t L, int32_t N, int64_t n_records) {
  if (L < 1 || N < 1 || n_records < 1) return 1;
  const int cus = ionode::compute_units();
  const int NT = np_of(N) / 16;   // (the plan of the kernel that reduce_impl will launch for this width)
  return ionode::grad_use_gen(NT) ? ionode::grad_gen_reduce_slabs(L, NT, cus, n_records) : ionode::grad_reduce_slabs(L, NT, cus, n_records);
}

int ionode_grad_reduce(int32_t L, int32_t N, const float *records, int64_t n_records, int32_t n_slabs, float *partials,
                       void *stream) {
  return reduce_impl(L, N, records, n_records, n_slabs, partials, stream, 0);
}

int ionode_grad_reduce_unit(int32_t L, int32_t N, const float *records, int64_t n_records, int32_t n_slabs, float *partials,
                            void *stream) {
  return reduce_impl(L, N, records, n_records, n_slabs, partials, stream, 1);
}

// Pure host: which kernel serves the regression step at (L, N), its workgroups per compute unit and its LDS.  No HIP call in here.
int ionode_regress_plan(int32_t L, int32_t N, int32_t out[3]) {
  if (!out) { gerr("ionode_regress_plan: bad argument"); return IONODE_ERR_ARG; }
  if (L < 1 || L > ionode::GRAD_MAX_LAYERS || N < 1 || N > 512)
    return refuse(IONODE_ERR_UNSUPPORTED, "ionode_regress_step: (L = %d, N = %d) outside the served shapes (1 <= N <= 512, 1 to 15 hidden layers)", (int)L, (int)N);
  const int NT = np_of(N) / 16;
  const bool gen = ionode::grad_use_gen(NT);
  const size_t lds = gen ? ionode::grad_gen_lds_bytes(L, NT) : ionode::grad_lds_bytes(L, NT);
  if (lds > ionode::GRAD_LDS_LIMIT)
    return refuse(IONODE_ERR_UNSUPPORTED, "ionode_regress_step: (L = %d, N = %d) needs %zu bytes of LDS per workgroup, a compute unit has %zu", (int)L, (int)N,
                  lds, ionode::GRAD_LDS_LIMIT);
  out[0] = gen ? 1 : 0;
  out[1] = gen ? ionode::grad_gen_wg_per_cu(L, NT) : (NT <= 13 ? IONODE_REGRESS_WG_PER_CU : 1);
  out[2] = (int32_t)lds;
  return IONODE_OK;
}

int ionode_regress_step(int32_t L, int32_t N, const float *grad_image, const float *x, const float *offset, const float *y,
                        int32_t n_rows, float netscale, float *records, double *loss_partials, int32_t n_workgroups,
                        void *stream) {
  if (!grad_image || !x || !y || !records || !loss_partials || n_rows < 1 || n_workgroups < 1 || L < 1 || N < 1) {
    gerr("ionode_regress_step: bad argument"); return IONODE_ERR_ARG;
  }
  int32_t plan[3];
  if (const int rc = ionode_regress_plan(L, N, plan)) return rc;   // (refusals: its message)
  const int NT = np_of(N) / 16;
  ionode::RArgs a;
  memset(&a, 0, sizeof a);
  a.img = grad_image; a.x = x; a.y = y; a.offset = offset; a.records = records; a.loss_part = loss_partials;
  a.M = n_rows; a.L = L; a.N = N; a.NT = NT; a.record_floats = ionode::grad_record_floats(L, NT); a.netscale = netscale;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (plan[0]) ionode::launch_regress_gen(a, (unsigned)n_workgroups, s);   // inst_grad_gen.hip
  else ionode::for_width(NT, [&](auto nt) { ionode::launch_regress<decltype(nt)::value>(a, (unsigned)n_workgroups, s); },
                         [&] { ionode::launch_regress32(a, (unsigned)n_workgroups, s); });
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

// ---- tangent (forward-mode) sweep of the closed-form models: per-sample sensitivities and their Gauss-Newton sums (ionode_tangent.hpp) ----
// Every refusal is decided here, before the launch.
int ionode_tangent_sweep(const ionode_desc *d, const double *params, const double *prot_v, const double *prot_t,
                         const int32_t *prot_of_traj, const double *t_eval, const int32_t *n_accepted,
                         double *di_dp, double *jtr, double *jtj, void *stream) {
  constexpr const char *WHO = "ionode_tangent_sweep";
  if (!d) return refuse(IONODE_ERR_ARG, "null descriptor");
  if (d->model != IONODE_MODEL_HH2 && !is_m6(d)) return refuse(IONODE_ERR_UNSUPPORTED, "%s: closed-form models only (HH 2-state, 6-state)", WHO);
  if (d->traj_per_image > 0) return refuse(IONODE_ERR_UNSUPPORTED, "%s: traj_per_image must be 0", WHO);
  if (!desc_consistent(d)) return refuse(IONODE_ERR_ARG, "inconsistent descriptor");
  if (!params || !prot_v || !t_eval || !n_accepted || !d->ckpt || d->ckpt_cap < 1)
    return refuse(IONODE_ERR_ARG, "%s: required buffer is NULL (ckpt / ckpt_cap come from the descriptor)", WHO);
  if (!di_dp && !jtr && !jtj) return refuse(IONODE_ERR_ARG, "%s: nothing to compute (di_dp, jtr and jtj are all NULL)", WHO);
  if ((jtr || jtj) && !d->sse_ref) return refuse(IONODE_ERR_ARG, "%s: jtr / jtj need the reference currents (sse_ref comes from the descriptor)", WHO);

  ionode::TArgs t;
  memset(&t, 0, sizeof t);
  GArgs &a = t.g;
  a.k.params = params; a.k.prot_v = prot_v; a.k.prot_t = prot_t; a.k.prot_of_traj = prot_of_traj; a.k.t_eval = t_eval;
  a.k.B = d->n_traj; a.k.Nt = d->n_out; a.k.P = d->n_prot; a.k.Np = d->prot_n; a.k.n_params = d->n_params;
  a.k.NP = 16; a.k.NT = 1;
  a.k.prot_t0 = d->prot_t0; a.k.prot_dt = d->prot_dt; a.k.prot_rdt = 1.0 / d->prot_dt; a.k.v_oob = d->v_oob;
  a.ckpt = d->ckpt; a.ckpt_cap = d->ckpt_cap; a.nacc = n_accepted;
  a.sse_ref = d->sse_ref; a.v_tab = d->v_at_outputs;
  a.obs_g = d->obs_g; a.obs_e = d->obs_e; a.obs_open = d->obs_open_state_only ? 1 : 0;
  t.di_dp = di_dp; t.jtr = jtr; t.jtj = jtj;
  ionode::launch_tangent(d->model, d->state_f32 ? 1 : 0, t, reinterpret_cast<hipStream_t>(stream));
  const hipError_t err = hipGetLastError();
  if (err != hipSuccess) return refuse(IONODE_ERR_LAUNCH, "%s", hipGetErrorString(err));
  return IONODE_OK;
}

// ---- tangent sweep of NN-f / NN-d (ionode_tangent_nn.hpp): per chunk the recompute kernel without grad_y and without records -- the
// packets' stage fields alone -- then the tangent walk over them, both on `stream`.  The recompute launcher is reached here and not
// through ionode_dopri5_backward_recompute_sse, which requires d->sse_ref: the trace needs none.  Every refusal is decided before the
// first launch.
size_t ionode_tangent_nn_state_doubles(void) { return (size_t)ionode::TANGENT_NN_STATE; }

int ionode_tangent_sweep_nn(const ionode_desc *d, int32_t it_begin, int32_t it_end, int32_t n_iter, const float *grad_image,
                            const double *params, const double *prot_v, const double *prot_t, const int32_t *prot_of_traj,
                            const double *t_eval, const int32_t *n_accepted, double *packets, double *state,
                            double *di_dp, double *jtr, double *jtj, void *stream) {
  constexpr const char *WHO = "ionode_tangent_sweep_nn";
  if (!d) return refuse(IONODE_ERR_ARG, "null descriptor");
  if (d->model == IONODE_MODEL_HH2 || is_m6(d)) return refuse(IONODE_ERR_UNSUPPORTED, "%s: NN-f / NN-d only (closed-form models: ionode_tangent_sweep)", WHO);
  if (!is_nn(d)) return refuse(IONODE_ERR_UNSUPPORTED, "%s: unknown model", WHO);
  if (d->traj_per_image > 0) return refuse(IONODE_ERR_UNSUPPORTED, "%s: traj_per_image must be 0", WHO);
  if (!desc_consistent(d)) return refuse(IONODE_ERR_ARG, "inconsistent descriptor");
  if (!grad_image || !params || !prot_v || !t_eval || !n_accepted || !packets || !state || !d->ckpt || d->ckpt_cap < 1)
    return refuse(IONODE_ERR_ARG, "%s: required buffer is NULL (ckpt / ckpt_cap come from the descriptor)", WHO);
  if (!di_dp && !jtr && !jtj) return refuse(IONODE_ERR_ARG, "%s: nothing to compute (di_dp, jtr and jtj are all NULL)", WHO);
  if ((jtr || jtj) && !d->sse_ref) return refuse(IONODE_ERR_ARG, "%s: jtr / jtj need the reference currents (sse_ref comes from the descriptor)", WHO);
  if (it_begin < 0 || it_end <= it_begin || it_end > n_iter) return refuse(IONODE_ERR_ARG, "bad iteration range");
  if ((int64_t)it_end - it_begin > (int64_t)65535 * 4)
    return refuse(IONODE_ERR_ARG, "%s: at most 65535 x 4 iterations per launch (HIP's grid.y limit): split the range", WHO);
  if (d->mlp_layers < 1 || d->mlp_width < 1) return refuse(IONODE_ERR_ARG, "bad MLP shape");
  const int NP = np_of(d->mlp_width), NT = NP / 16, L = d->mlp_layers;
  const SweepFn recompute = find_sweep(Sweep::Recompute, d, NT);
  const size_t net_lds = ionode::grad_lds_bytes(L, NT);
  if (!recompute || L > 15 || net_lds + 16 + ionode::grad_walk_lds_bytes() > 160 * 1024)   // (the two-phase backward sweep's own rule)
    return refuse(IONODE_ERR_UNSUPPORTED, "%s: (L, N) outside the backward sweep's compiled variants (N pads to 16, 112, 208 or 512; at most 15 hidden layers)", WHO);

  ionode::TArgs t;
  memset(&t, 0, sizeof t);
  GArgs &a = t.g;
  a.k.params = params; a.k.prot_v = prot_v; a.k.prot_t = prot_t; a.k.prot_of_traj = prot_of_traj; a.k.t_eval = t_eval;
  a.k.B = d->n_traj; a.k.Nt = d->n_out; a.k.P = d->n_prot; a.k.Np = d->prot_n; a.k.n_params = d->n_params;
  a.k.L = L; a.k.N = d->mlp_width; a.k.NP = NP; a.k.NT = NT;
  a.k.prot_t0 = d->prot_t0; a.k.prot_dt = d->prot_dt; a.k.prot_rdt = 1.0 / d->prot_dt; a.k.v_oob = d->v_oob;
  a.img = grad_image; a.ckpt = d->ckpt; a.ckpt_cap = d->ckpt_cap; a.nacc = n_accepted;
  a.record_floats = ionode::grad_record_floats(L, NT); a.packets = packets;   // (grad_y, records: NULL -- the packets' stage fields alone)
  a.it_begin = it_begin; a.it_end = it_end; a.n_iter = n_iter;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  recompute(a, (unsigned)((a.k.B + 15) / 16), net_lds, s);
  hipError_t err = hipGetLastError();
  if (err != hipSuccess) return refuse(IONODE_ERR_LAUNCH, "%s", hipGetErrorString(err));
  // what the walk reads beside the packets: the carried state, the observation model and (for the sums) the reference currents
  a.state = state; a.sse_ref = d->sse_ref; a.v_tab = d->v_at_outputs;
  a.obs_g = d->obs_g; a.obs_e = d->obs_e; a.obs_open = d->obs_open_state_only ? 1 : 0;
  t.di_dp = di_dp; t.jtr = jtr; t.jtj = jtj;
  ionode::launch_tangent_nn(d->model, d->state_f32 ? 1 : 0, t, s);
  err = hipGetLastError();
  if (err != hipSuccess) return refuse(IONODE_ERR_LAUNCH, "%s", hipGetErrorString(err));
  return IONODE_OK;
}

}  // extern "C"
