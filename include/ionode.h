/*
 * ionode.h -- C ABI of libionode.so: the MI355X-native batched neural-ODE integrator for
 * ion-channel gating models (adaptive Dormand-Prince RK45 + dense output, HIP, gfx950).
 *
 * What it replaces.  The reference (chonlei/neural-ode-ion-channels) has no FFI: its hot path is the
 * Python call
 *     odeint(func, y0, t)                      train-s1.py:322,327  train-d0.py:428  train-r1.py:273 ...
 * into torchdiffeq==0.2.1 (requirements.txt:1), which calls back func.forward(t, y) six times per
 * step (train-s1.py:231-247 NN-f, train-d2.py:257-272 NN-d, train-s1.py:161-177 HH,
 * train-d1.py:165-187 6-state).  The entry points below are what a binding for that call binds:
 * ONE launch integrates a whole batch of independent trajectories, with the RHS fused into the
 * kernel.  Caller owns every buffer; the library allocates nothing and keeps no state.
 *
 *   reference interface                                    entry point here
 *   -----------------------------------------------------  --------------------------------------
 *   odeint(func, y0, t, rtol, atol, method='dopri5')       ionode_dopri5()
 *   func.net state_dict  (net.{0,2,..}.weight/.bias)       ionode_mlp_packed_floats()/ionode_mlp_pack()
 *   func.set_fixed_form_voltage_protocol(t, v)             prot_v / prot_t / prot_t0 / prot_dt arguments
 *   pred_y[:,0,0]*pred_y[:,0,1]*(func._v(t)+86)            optional fused epilogue -> i_out
 *       (train-s1.py:328, train-r1.py:274, train-d1.py:299)
 *   AssertionError 'underflow in dt' / 'non-finite' /      per-trajectory status[] codes
 *       'max_num_steps exceeded' (torchdiffeq)
 *
 * All pointers passed to ionode_dopri5 are DEVICE pointers (HBM), except the descriptor.
 */
#ifndef IONODE_H
#define IONODE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define IONODE_ABI_VERSION 10

/* RHS families (func.forward variants of the reference) */
#define IONODE_MODEL_HH2 0     /* 2-state Hodgkin-Huxley: Lambda, train-s1.py:134-177; candidate ODEFunc train-d0.py:321-374 */
#define IONODE_MODEL_MARKOV6 1 /* 6-state Markov: Lambda, train-d1.py:134-187 */
#define IONODE_MODEL_NNF 2     /* NN-f: da/dt = MLP(V/100, a)/1000, train-s1.py:181-247 */
#define IONODE_MODEL_NND 3     /* NN-d: da/dt = HH + MLP(V/100, a)/1000, train-d2.py:191-272 */

/* per-trajectory status (torchdiffeq's assertion messages) */
#define IONODE_STATUS_OK 0
#define IONODE_STATUS_DT_UNDERFLOW 1 /* 'underflow in dt' */
#define IONODE_STATUS_NONFINITE 2    /* 'non-finite values in state `y`' */
#define IONODE_STATUS_MAX_STEPS 3    /* 'max_num_steps exceeded' */

/* return codes of the entry points */
#define IONODE_OK 0
#define IONODE_ERR_ARG (-1)      /* inconsistent descriptor / NULL where a buffer is required */
#define IONODE_ERR_UNSUPPORTED (-2) /* shape outside what the kernels are built for */
#define IONODE_ERR_LAUNCH (-3)   /* hipLaunchKernel failed; see ionode_last_error() */

typedef struct ionode_desc {
  int32_t model;       /* IONODE_MODEL_* */
  int32_t state_f32;   /* 1: solver state (y, k, dense output) in fp32 = the reference scripts' y0.dtype;
                          0: fp64 state (BASELINE configs 2-3).  Time/step control is fp64 either way. */
  int32_t n_state;     /* D: 2 (HH2, NNF, NND) or 6 (MARKOV6) */
  int32_t n_out;       /* len(t) */
  int32_t n_traj;      /* B */
  int32_t n_prot;      /* P voltage protocols of prot_n samples each */
  int32_t prot_n;      /* samples per protocol */
  int32_t mlp_layers;  /* L: hidden N x N Linear layers (architectures/sNN.py: n_layers) */
  int32_t mlp_width;   /* N: nodes per layer (architectures/sNN.py: n_nodes) */
  int32_t n_params;    /* doubles per trajectory in params[]: >= 8 (p1..p8), >= 12 for MARKOV6 */
  int64_t max_steps;   /* torchdiffeq's max_num_steps: step attempts allowed between two emitted outputs (its _advance
                          resets the counter for every output time); 0 = torchdiffeq's default 2**31 - 1 */
  double prot_t0;      /* uniform protocol grid t_i = prot_t0 + i*prot_dt (used when prot_t == NULL) */
  double prot_dt;
  double v_oob;        /* voltage substituted outside the protocol's time range: -80 (train-s1.py:237) */
  double rtol, atol;   /* torchdiffeq defaults 1e-7 / 1e-9; the reference never overrides them */
  double obs_g;        /* observation epilogue i = g * gate * (V(t_k) - obs_e); gate = y0*y1 or y[D-1] */
  double obs_e;
  int32_t obs_open_state_only; /* 1: gate = last state (6-state O, train-d1.py:299) */
  int32_t tile_waves;  /* tuning, 0 = auto.  MLP models: wavefronts cooperating on one 16-trajectory tile (1, 4); N <= 16 nets
                          also 64 = one trajectory per lane, 64 per wavefront (auto from ionode_lane_wise_from() trajectories); N = 200 also 8 / 2 / 16 = 32 / 4 / 1
                          trajectories per tile (auto: 1 up to 256 trajectories, 4 up to 1024, 16 up to 8191, 32 beyond).  Closed-form models: trajectories per wavefront (64 or 16; auto = 16 below ionode_lane_wise_from()) */
  double *step_log;    /* optional DEVICE buffer [step_log_cap][4] fp64: (t0, dt, error ratio, accepted) of every
                          step attempt of trajectory 0 -- the per-step trace parity tests compare; NULL = off */
  int64_t step_log_cap;
  double t_eval_t0_hint; /* optional hint t_eval[k] ~ t0_hint + k*dt_hint (dt_hint <= 0: none).  Only a starting guess for */
  double t_eval_dt_hint; /* the output cursor, verified against t_eval in the kernel: a wrong hint costs time, not results */
  int64_t max_total_steps; /* runaway bound: step attempts allowed over the whole solve of one trajectory (a tile runs until
                          its slowest trajectory ends; the reference bounds a solve with a 600 s SIGALRM, train-d0.py:309-318).
                          0 = library default IONODE_DEFAULT_MAX_TOTAL_STEPS; < 0 = unbounded.  Exceeding it gives
                          IONODE_STATUS_MAX_STEPS like max_steps. */
  double *ckpt;        /* optional DEVICE buffer [n_traj][ckpt_cap][4 + 8*n_state] fp64, one record per ACCEPTED step:
                          {t0, dt, first output index of the step, outputs emitted, y[D], k1..k7[D]} -- what the backward
                          sweep (ionode_dopri5_backward) replays.  Steps beyond ckpt_cap are not recorded (the caller
                          compares stats[b][0] with ckpt_cap and retries with a larger buffer).  NULL = off */
  int32_t ckpt_cap;
  int32_t t_eval_exact; /* 1: the caller has VERIFIED t_eval[k] == t_eval_t0_hint + (double)k * t_eval_dt_hint bit for bit (fp64
                          multiply, then add) for every k.  The closed-form kernels then form output times arithmetically and
                          take their store-friendly emission path; results are identical either way.  0 = not verified */
  const double *sse_ref; /* fused objective (PINTS SumOfSquaresError over Model.simulate, train-d0.py:415-439, :508-540), optional:
                          DEVICE [n_prot][n_out] reference currents.  With sse_out set, every trajectory's
                          sum_k (i_k - sse_ref[protocol][k])^2 (i as in the i_out epilogue) is accumulated in the kernel and
                          written to sse_out[b] (inf where the solve failed -- the reference's time-limit rule); y_out and i_out
                          may then be NULL, so that no trace leaves the chip: BASELINE configs[3]'s 65 536 candidates x 32
                          sweeps x 1e5 samples would be 4.5 TB of traces.  Needs the output-grid hint. */
  double *sse_out;     /* DEVICE [n_traj] fp64 or NULL.  Through ionode_dopri5_objective(IONODE_OBJECTIVE_SAE) the sums are of
                          |i_k - sse_ref[protocol][k]| instead (both fields keep their names) */
  double max_step;     /* EXTENSION (torchdiffeq 0.2.1's dopri5 has no such option; 0 = off = reference behaviour): cap on the
                          step size in ms.  At an equilibrium dopri5 grows dt until h*lambda leaves its stability region
                          (the error estimate of a state AT equilibrium is ~0); the forward solve copes through rejections,
                          but the reverse-mode derivative of such accepted-but-unstable steps multiplies adjoints by
                          |R(h*lambda)| >> 1 per step.  max_step < 3.3 / lambda_max keeps the backward sweep bounded. */
  const double *v_at_outputs; /* optional (NULL = off), closed-form models with i_out or sse_out: DEVICE [n_prot][n_out] protocol
                          voltage at the output times, filled by ionode_protocol_at_outputs() for the same protocols and t_eval.
                          The current / objective epilogue then loads V(t_k) instead of re-deriving it per trajectory per sample
                          (same values: the pre-pass runs the integrator's own lookup).  Pays when n_prot << n_traj. */
  int64_t mlp_image_stride; /* NN models, several weight sets in one launch (an ensemble of trained nets, a population of random
                          initialisations): floats between consecutive packed images in `mlp_packed` (>= ionode_mlp_packed_floats) ... */
  int32_t traj_per_image;   /* ... and the number of CONSECUTIVE trajectories that share one image: trajectory b uses image
                          b / traj_per_image.  A multiple of 16 (of 64 with tile_waves = 64).  0 = one image for every trajectory.
                          Forward path only (the backward sweep differentiates one weight set). */
  const int32_t *launch_order; /* optional (NULL = index order), DEVICE [n_traj]: a permutation of 0..n_traj-1.  Launch slot s
                          integrates trajectory launch_order[s]; every input and output stays at the trajectory's OWN index, so the
                          results are those of index order, bit for bit -- only which trajectories share a tile / a wavefront, and
                          in which sequence the tiles start, changes.  What the reference's callers would sort by: predicted cost
                          (tiles become homogeneous, the launch a longest-first list schedule) or protocol (the lanes of a
                          wavefront interpolate one protocol).  Not with traj_per_image.  Since ABI 6. */
} ionode_desc;

#define IONODE_DEFAULT_MAX_TOTAL_STEPS 1000000

/* Number of floats of the device-side weight image for an (L, N) MLP  Linear(2,N) + L x Linear(N,N) + Linear(N,1). */
size_t ionode_mlp_packed_floats(int32_t mlp_layers, int32_t mlp_width);

/* HOST -> HOST.  Re-lays a state dict (flat fp32, order net.0.weight [N][2], net.0.bias [N],
 * {net.2i.weight [N][N], net.2i.bias [N]} x L, net.last.weight [1][N], net.last.bias [1]; row-major as
 * torch stores nn.Linear) into the MFMA-fragment order the kernels stream.  The caller uploads `packed`.
 * The image is an opaque, derived artefact of THIS library build (its sections and their order follow the kernels:
 * fragment streams, the 4-trajectory tile's section, the per-lane net's scalar row pairs): pack after loading the
 * library, do not persist images across library versions. */
int ionode_mlp_pack(const float *state_dict_flat, int32_t mlp_layers, int32_t mlp_width, float *packed);

/*
 * Integrate d->n_traj independent trajectories on the current device, asynchronously on `stream`.
 *
 *   mlp_packed    device, ionode_mlp_packed_floats() floats (NULL for HH2 / MARKOV6)
 *   params        device, [B][n_params] fp64: p1..p8 (NNF reads p5..p8) or p1..p12
 *   prot_v        device, [P][prot_n] fp64 mV
 *   prot_t        device, [prot_n] fp64 ms shared by all protocols, or NULL for the uniform grid
 *   prot_of_traj  device, [B] int32 protocol index per trajectory, or NULL (trajectory b uses b % P)
 *   y0            device, [B][D] in the state dtype
 *   t_eval        device, [n_out] fp64, strictly increasing; t_eval[0] is the initial time
 *   y_out         device, [B][n_out][D] in the state dtype (may be NULL when d->sse_out is set)
 *   i_out         device, [B][n_out] fp64 current trace, or NULL
 *   status        device, [B] int32 IONODE_STATUS_*
 *   stats         device, [B][4] int64 {accepted steps, rejected steps, RHS evaluations, status}, or NULL
 *   stream        hipStream_t (NULL = default stream)
 *
 * Returns IONODE_OK once the kernel is enqueued; per-trajectory failures are reported in status[]
 * (their remaining outputs are NaN), never as a return code.  d == NULL is IONODE_ERR_ARG ("null descriptor") here and on
 * ionode_dopri5_deferred / _composed / _objective, which share this entry point's checks (earlier builds dereferenced it).
 */
int ionode_dopri5(const ionode_desc *d, const float *mlp_packed, const double *params, const double *prot_v,
                  const double *prot_t, const int32_t *prot_of_traj, const void *y0, const double *t_eval,
                  void *y_out, double *i_out, int32_t *status, int64_t *stats, void *stream);

/*
 * Deferred dense output (since ABI 10, added later: new symbols only, ionode_desc and every earlier entry point unchanged).
 * The lean N = 200 16-trajectory tile kernels (NN-f / NN-d, both state dtypes: verified uniform output grid, uniform protocol grid,
 * no step log, no checkpoints) can leave the dense output of their accepted steps to a second, store-bound kernel: a step writes one
 * 112-byte record (t0, step length, its reciprocal, first output index and output count, the 5 x 2 interpolant coefficients) into a
 * caller-owned workspace, and ionode_dense_expand_kernel evaluates and stores the samples after the solve, on the same stream.
 * y_out, i_out, status and stats are bit for bit those of ionode_dopri5().
 *
 * ionode_dense_defer_plan(): pure host code.  out = {records per trajectory, workspace bytes} for `d` (want_current: an i_out buffer
 * will be passed), both 0 when nothing would be deferred -- another kernel variant, the fused objective (sse_out), or
 * IONODE_DEFER_DENSE=0 in the environment.  The records may take a quarter of the bytes of the requested outputs:
 * capacity = min(n_out - 1, that / (n_traj * 112)), and a capacity under 64 defers nothing.  A trajectory that fills its records
 * emits its later steps itself, as without the workspace.  IONODE_DEFER_DENSE_CAP=n forces a capacity (both are development
 * switches, read per plan).  Workspace layout: int32 count per trajectory, then (16-byte aligned) records [n_traj][capacity][14] fp64,
 * indexed by trajectory whatever the launch order.
 *
 * ionode_dopri5_deferred(): ionode_dopri5() plus `workspace` (DEVICE, 16-byte aligned, at least the plan's bytes, contents
 * undefined before and after) and its size.  workspace == NULL, or a descriptor whose plan defers nothing (an explicit prot_t
 * included), is exactly ionode_dopri5(); IONODE_ERR_ARG for a workspace smaller than the plan's.
 *
 * The solve kernel's tail (new symbol ionode_dense_tail_plan; everything above unchanged).  A launch lasts as long as its slowest tile,
 * so the tiles that end early expand their own records before they leave, on compute units that would otherwise idle, and store
 * -(records + 1) as the trajectory's count; the follow-up kernel expands the trajectories with a positive count.  A finish counter
 * ranks the tiles (one atomic add per tile, nothing waits on it); it lives in the workspace's LAST record slot, which is used
 * internally: with the tail on a trajectory fills capacity - 1 records.  ionode_dense_tail_plan(): pure host code.  out = {tiles that
 * expand in the solve kernel (the first out[0] to end), records a trajectory may fill}; {0, capacity} where the tail is off (capacity
 * < 2, IONODE_DEFER_TAIL=0).  The default is 5/8 of the tiles, rounded down; IONODE_DEFER_TAIL=all: every tile,
 * IONODE_DEFER_TAIL_RANK=n: n tiles (development switches, read per plan).
 */
int ionode_dense_defer_plan(const ionode_desc *d, int32_t want_current, int64_t out[2]);
int ionode_dense_tail_plan(const ionode_desc *d, int32_t want_current, int64_t out[2]);
int ionode_dopri5_deferred(const ionode_desc *d, const float *mlp_packed, const double *params, const double *prot_v,
                           const double *prot_t, const int32_t *prot_of_traj, const void *y0, const double *t_eval,
                           void *y_out, double *i_out, int32_t *status, int64_t *stats, void *stream, void *workspace,
                           int64_t workspace_bytes);

/*
 * Shrink-aware tile composition (since ABI 10, added later: new symbols only, ionode_desc and every earlier entry point unchanged).
 * The lean N = 200 16-trajectory tile steps its 16 slots in lock step and finishes on the 4-trajectory net once at most 4 of them are
 * live, so a tile takes  A5 * 6 e16 + (A1 - A5) * 6 e4  (A1, A5: largest and fifth-largest attempt count of its trajectories; e16, e4:
 * one evaluation on either net), and a launch of at most one tile per compute unit lasts as long as its slowest tile: it depends on
 * which trajectories share a tile.  The rule (csrc/ionode_compose.hpp): sort by cost descending, ties by index, a non-finite or
 * negative cost counting as 0; tile k takes sorted entries 4 k .. 4 k + 3 into its slots 0 .. 3 and fills its other 12 slots from the
 * light end, lightest first; only the last tile is ragged (the lightest heavies, at most 4, and the lights that remain); equal costs
 * everywhere leave index order.  The result is an ionode_desc.launch_order: outputs stay at the trajectories' own indices, bit for bit.
 *
 * ionode_compose_plan(): out = {1 if `d` qualifies, the cost source IONODE_COMPOSE allows}.  It qualifies when ionode_dopri5 would run
 * one of the four lean N = 200 shrink kernels (NN-f / NN-d, both state dtypes) with the shrink on (IONODE_TILE_SHRINK), with at most
 * one tile per compute unit of the CALLER's current device (asked on every call; 256 where there is none), without traj_per_image,
 * without a launch_order of the caller's, and n_traj <= 8192.  Source: 3 = any (default), 1 = the pilot only (IONODE_COMPOSE=pilot),
 * 2 = an earlier call's stats only (IONODE_COMPOSE=hint), 0 = IONODE_COMPOSE=0, which also makes out[0] 0 (a development switch,
 * read per plan).  Like ionode_dense_defer_plan it takes the protocol grid to be uniform (prot_t == NULL).
 *
 * ionode_compose_order(): DEVICE, asynchronous on `stream`, no host synchronisation.  Reads cost[b * cost_stride], b < n_traj, as fp64
 * (cost_is_int64 = 0) or int64 (1: e.g. column 2 of a stats tensor in place, cost = stats + 2, cost_stride = 4) and writes
 * order[n_traj] int32 by the rule.  One workgroup, bitonic sort in LDS; n_traj <= 8192, IONODE_ERR_UNSUPPORTED beyond.  Any cost
 * values, garbage included, give a valid permutation.
 *
 * ionode_compose_order_host(): HOST -> HOST mirror of the same rule (cost fp64 [n_traj]), for tests and replays.
 *
 * ionode_dopri5_composed(): ionode_dopri5_deferred() for a launch whose d->launch_order came from ionode_compose_order(), plus where
 * its cost came from -- cost_source 1: a pilot, 2: the counts of an earlier solve of the same batch (or the caller's own costs), 0 or
 * d->launch_order == NULL: exactly ionode_dopri5_deferred().  A composed launch ends its tiles at other times than index order, so the
 * solve kernel's tail takes its fraction of the tiles from the cost source (the rule of ionode_dense_tail_plan on the composed launch's
 * own stamps).  Results do not depend on it.  ionode_compose_tail_plan(): ionode_dense_tail_plan() for such a launch.
 */
int ionode_dopri5_composed(const ionode_desc *d, const float *mlp_packed, const double *params, const double *prot_v,
                           const double *prot_t, const int32_t *prot_of_traj, const void *y0, const double *t_eval,
                           void *y_out, double *i_out, int32_t *status, int64_t *stats, void *stream, void *workspace,
                           int64_t workspace_bytes, int32_t cost_source);
int ionode_compose_tail_plan(const ionode_desc *d, int32_t want_current, int32_t cost_source, int64_t out[2]);
int ionode_compose_plan(const ionode_desc *d, int32_t want_current, int32_t out[2]);
int ionode_compose_order(const void *cost, int32_t cost_is_int64, int64_t cost_stride, int32_t n_traj, int32_t *order, void *stream);
int ionode_compose_order_host(const double *cost, int32_t n_traj, int32_t *order);

/*
 * The kind of the fused objective (since ABI 10, added later: new symbols only, ionode_desc and every earlier entry point unchanged).
 * What a trajectory's samples add to d->sse_out[b], against d->sse_ref (the field names stay, whatever the kind):
 *   IONODE_OBJECTIVE_SSE  sum_k (i_k - sse_ref[protocol][k])^2 -- what sse_out has always held (PINTS SumOfSquaresError);
 *   IONODE_OBJECTIVE_SAE  sum_k |i_k - sse_ref[protocol][k]| -- n_out times the reference's prediction loss
 *                         torch.mean(torch.abs(pred_yo - data)) (train-s1.py:275-353, the validation of train-r1.py:930-959), which it
 *                         only ever evaluates under torch.no_grad(); its gradient: ionode_objective_backward[_gc]() below.
 * Same kernels, same summation order, same inf for a failed trajectory: the kind is a wave-uniform kernel argument that selects the
 * term a residual contributes (csrc/ionode_interp.hpp residual_term), and with IONODE_OBJECTIVE_SSE every output is bit for bit what
 * the earlier entry points write.  One exception in the choice of kernel, none in the results: the lean N = 200 16-trajectory tile
 * kernels (the ones that shrink and defer) fill the register file and are compiled for the squares alone, so IONODE_OBJECTIVE_SAE on
 * that tile runs its general variant.
 *
 * ionode_dopri5_objective(): ionode_dopri5_composed() plus `objective`.  IONODE_OBJECTIVE_SSE is exactly ionode_dopri5_composed().
 * IONODE_OBJECTIVE_SAE needs d->sse_out (and, as every fused objective, d->sse_ref and the output-grid hint; nothing is deferred).
 * IONODE_ERR_ARG, checked before any other argument and before any launch, for another value of `objective` and for
 * IONODE_OBJECTIVE_SAE without d->sse_out.
 */
#define IONODE_OBJECTIVE_SSE 0
#define IONODE_OBJECTIVE_SAE 1
int ionode_dopri5_objective(const ionode_desc *d, const float *mlp_packed, const double *params, const double *prot_v,
                            const double *prot_t, const int32_t *prot_of_traj, const void *y0, const double *t_eval,
                            void *y_out, double *i_out, int32_t *status, int64_t *stats, void *stream, void *workspace,
                            int64_t workspace_bytes, int32_t cost_source, int32_t objective);

/* Pre-pass for ionode_desc.v_at_outputs: v_out[p][k] = V_p(t_eval[k]) for the d->n_prot protocols at the d->n_out output
 * times, by the integrator's own lookup (linear interpolation, -80 mV / v_oob outside the protocol: train-s1.py:218-237).
 * Reads d->n_out, n_prot, prot_n, prot_t0, prot_dt, v_oob.  Asynchronous on `stream`. */
int ionode_protocol_at_outputs(const ionode_desc *d, const double *prot_v, const double *prot_t, const double *t_eval,
                               double *v_out, void *stream);

/* Launch geometry the dispatcher would use for `d` (for tests / bench reporting): grid, block, LDS bytes, tile_waves. */
int ionode_launch_geometry(const ionode_desc *d, int32_t out[4]);

/* Name of the kernel instantiation ionode_dopri5 would launch for `d` (matches rocprofv3 kernel-trace).  The descriptor does
 * not say whether an i_out buffer will be passed; a fused objective or a v_at_outputs table implies the epilogue variant. */
const char *ionode_kernel_name(const ionode_desc *d);

/* Name of the instantiation this thread's last successful ionode_dopri5 call launched ("" before the first). */
const char *ionode_last_kernel_name(void);

/* Batch size from which ionode_dopri5 (tile_waves = 0) takes the one-trajectory-per-lane kernel (64 trajectories per wavefront) of
 * `model` (mlp_width: the net's width for the NN models, ignored otherwise); 0 if the model has no such kernel.  Callers that sort
 * trajectories by protocol for those kernels (launch_order) read the crossover here instead of keeping a copy.  Since ABI 8. */
int32_t ionode_lane_wise_from(int32_t model, int32_t mlp_width);

const char *ionode_last_error(void);
int32_t ionode_abi_version(void);

/* ---------------------------------------------------------------------------------------------------------------------
 * Gradients through the solve (BASELINE.json configs[4]).  Reference interface: `from torchdiffeq import odeint_adjoint as
 * odeint` (train-s1.py:29-32) -- the reference only switches this import and never differentiates (SURVEY.md finding 3),
 * so what is computed is defined here: the exact reverse-mode derivative of the discretisation the forward launch executed,
 * with its accepted steps (t0, dt) as constants; rejected attempts do not contribute.  NN-f / NN-d for the widths of
 * architectures s00-s11 (N = 10, 100, 200, 500) with at most 15 hidden layers, and the closed-form HH 2-state and 6-state
 * models (no grad_image, no records: gradients with respect to the rate parameters and y0 only; D = 6 and 12 parameters
 * for the 6-state model).
 *
 * Flow (all pointers DEVICE unless noted):
 *   1. forward:  ionode_dopri5() with d->ckpt / d->ckpt_cap set; n_accepted[b] = stats[b][0] for status[b] == 0, else 0
 *   2. sweep:    ionode_dopri5_backward() over iterations [0, n_iter), n_iter = max(n_accepted) + 1, in one launch or in
 *                chunks [it_begin, it_end) (the adjoint state is carried in `state`); each tile-evaluation appends one record
 *                of ionode_grad_record_floats() floats to `records` ([tiles][it_end - it_begin][6] records per chunk)
 *   3. reduce:   ionode_grad_reduce() contracts a chunk's records into n_slabs partial weight gradients; the caller sums
 *                the partials (and the chunks) and un-pads them (layout: ionode_grad_partial_floats)
 * ------------------------------------------------------------------------------------------------------------------- */

/* HOST -> HOST: flat state dict (ionode_mlp_pack's input order) -> grad image (forward AND transposed MFMA fragments). */
size_t ionode_grad_image_floats(int32_t mlp_layers, int32_t mlp_width);
int ionode_grad_pack(const float *state_dict_flat, int32_t mlp_layers, int32_t mlp_width, float *image);

/* floats of one record (one MLP vector-Jacobian product of one 16-trajectory tile): h_0..h_L, d_0..d_L tiles + 64 scalars */
size_t ionode_grad_record_floats(int32_t mlp_layers, int32_t mlp_width);

/*
 * Backward sweep, asynchronous on `stream`.  d: the forward launch's descriptor (model, state dtype, sizes, protocol grid,
 * v_oob, ckpt, ckpt_cap).
 *   (D = n_state, NPAR = 8, or 12 for the 6-state model)
 *   grad_image   device, ionode_grad_image_floats() floats (NULL for the closed-form models)
 *   n_accepted   device, [B] int32: accepted steps to replay per trajectory (0 = contributes nothing)
 *   grad_y       device, [B][n_out][D] dL/dy_out in the state dtype
 *   state        device, [B][2 D + NPAR] fp64 scratch carried between chunk launches (need not be initialised for it_begin == 0)
 *   records      device, [ceil(B/16)][it_end - it_begin][6][record floats] fp32, or NULL to skip the weight-gradient stream
 *   grad_params  device, [B][NPAR] fp64 dL/dp      (written by the launch with it_end == n_iter)
 *   grad_y0      device, [B][D] fp64 dL/dy0
 */
int ionode_dopri5_backward(const ionode_desc *d, int32_t it_begin, int32_t it_end, int32_t n_iter, const float *grad_image,
                           const double *params, const double *prot_v, const double *prot_t, const int32_t *prot_of_traj,
                           const double *t_eval, const int32_t *n_accepted, const void *grad_y, double *state,
                           float *records, double *grad_params, double *grad_y0, void *stream);

/*
 * Fused sum-of-squares gradient (closed-form HH 2-state and 6-state models; since ABI 10): the same sweep as
 * ionode_dopri5_backward, for the objective sse[b] = sum_k (i_k - sse_ref[protocol][k])^2 of the fused forward (i as in the
 * i_out epilogue, sample 0 = y0 included).  The upstream gradient is one scalar per trajectory, grad_sse[b] = dL/dsse[b]; the
 * sweep re-evaluates each output sample from the step's checkpoint and forms dL/dy_k itself, so neither y nor dL/dy is ever
 * materialised.  The forward is ionode_dopri5 with d->ckpt and d->sse_out set (y_out = i_out = NULL allowed).  Reads sse_ref,
 * obs_g, obs_e, obs_open_state_only, v_at_outputs (optional), ckpt and ckpt_cap from the descriptor; chunking over iterations,
 * n_accepted, state, grad_params and grad_y0 as for ionode_dopri5_backward (n_accepted[b] = 0: zero rows).  IONODE_ERR_ARG when
 * sse_ref, ckpt or grad_sse is NULL; IONODE_ERR_UNSUPPORTED for the NN models and for traj_per_image > 0.
 */
int ionode_dopri5_backward_sse(const ionode_desc *d, int32_t it_begin, int32_t it_end, int32_t n_iter, const double *params,
                               const double *prot_v, const double *prot_t, const int32_t *prot_of_traj, const double *t_eval,
                               const int32_t *n_accepted, const double *grad_sse, double *state, double *grad_params,
                               double *grad_y0, void *stream);

/*
 * Two-phase form of the same sweep (NN-f / NN-d).  A stage's vector-Jacobian product is LINEAR in its seed, and the seed is a scalar
 * per trajectory: product(seed) = seed * product(1).  Everything else the product needs -- the stage inputs, protocol voltages, rate
 * exponentials -- and the reduction of the step's output gradients depend on the step's checkpoint only.  So
 *   ionode_dopri5_backward_recompute()  runs, for EVERY (tile, step) of the chunk at once (the whole chip instead of one workgroup per
 *       16-trajectory tile), the unit-seed product of all six stages: records with unit-seed D tiles, and per tile and step
 *       ionode_grad_packet_doubles() doubles of scalars (`packets`: [ceil(B/16)][it_end - it_begin][doubles]);
 *   ionode_dopri5_backward_sweep()      walks the steps with the adjoint algebra alone (one wavefront per tile, no MLP work) and
 *       writes each evaluation's seed into its record;
 *   ionode_grad_reduce_unit()           contracts such records, scaling the D tiles by the seeds while staging them.
 * Same gradients as ionode_dopri5_backward() up to fp32 rounding (the seed multiplies at the end of the product instead of at its
 * start).  Call order per chunk: recompute, sweep, reduce_unit; recompute of chunk k + 1 may run beside the sweep of chunk k.
 */
size_t ionode_grad_packet_doubles(void);
int ionode_dopri5_backward_recompute(const ionode_desc *d, int32_t it_begin, int32_t it_end, int32_t n_iter, const float *grad_image,
                                     const double *params, const double *prot_v, const double *prot_t, const int32_t *prot_of_traj,
                                     const double *t_eval, const int32_t *n_accepted, const void *grad_y, float *records,
                                     double *packets, void *stream);
int ionode_dopri5_backward_sweep(const ionode_desc *d, int32_t it_begin, int32_t it_end, int32_t n_iter, const float *grad_image,
                                 const double *params, const double *prot_v, const double *prot_t, const int32_t *prot_of_traj,
                                 const double *t_eval, const int32_t *n_accepted, const void *grad_y, double *state,
                                 float *records, const double *packets, double *grad_params, double *grad_y0,
                                 void *stream);
int ionode_grad_reduce_unit(int32_t mlp_layers, int32_t mlp_width, const float *records, int64_t n_records, int32_t n_slabs,
                            float *partials, void *stream);

/*
 * Fused sum-of-squares gradient for NN-f / NN-d on the two-phase sweep (since ABI 10, added later: new symbols only, ionode_desc and
 * every earlier entry point unchanged).  The objective and the forward are ionode_dopri5_backward_sse's (d->ckpt and d->sse_out set,
 * y_out = i_out = NULL allowed); the upstream gradient is grad_sse[b] = dL/dsse[b].  Output gradients enter the two-phase sweep in one
 * place -- the G_c sums of a step's packet -- and in the sample-0 term of dL/dy0; both depend on the step's checkpoint, the protocol,
 * sse_ref and grad_sse only:
 *   ionode_dopri5_backward_sse_gc()         one wavefront per (trajectory, iteration) of the chunk: re-evaluates the step's output samples
 *       from its checkpoint and writes G_c into `packets` (the chunk's buffer, as for _recompute; zeros where a trajectory has no step);
 *       the launch with it_end == n_iter also writes sse_grad_y0 [B][2] fp64, the sample-0 term 2 grad_sse[b] r_0 dr_0/dy0;
 *   ionode_dopri5_backward_recompute_sse()  ionode_dopri5_backward_recompute without grad_y: leaves the packets' G_c alone;
 *   ionode_dopri5_backward_sweep_sse()      ionode_dopri5_backward_sweep with sse_grad_y0 in the place of grad_y.
 * Per chunk: sse_gc and recompute_sse (either order, the same `packets`), then sweep_sse, then ionode_grad_reduce_unit.  Neither y
 * nor dL/dy is ever materialised.  All three read sse_ref, ckpt, ckpt_cap (sse_gc also obs_g, obs_e, obs_open_state_only and the
 * optional v_at_outputs) from the descriptor.  IONODE_ERR_ARG for a missing buffer (sse_ref, ckpt, grad_sse, packets, sse_grad_y0,
 * ...) or a bad iteration range; IONODE_ERR_UNSUPPORTED for traj_per_image > 0, for the closed-form models (ionode_dopri5_backward_sse
 * serves those) and for widths or depths the sweep does not serve.
 */
int ionode_dopri5_backward_sse_gc(const ionode_desc *d, int32_t it_begin, int32_t it_end, int32_t n_iter, const double *prot_v,
                                  const double *prot_t, const int32_t *prot_of_traj, const double *t_eval, const int32_t *n_accepted,
                                  const double *grad_sse, double *packets, double *sse_grad_y0, void *stream);
int ionode_dopri5_backward_recompute_sse(const ionode_desc *d, int32_t it_begin, int32_t it_end, int32_t n_iter, const float *grad_image,
                                         const double *params, const double *prot_v, const double *prot_t, const int32_t *prot_of_traj,
                                         const double *t_eval, const int32_t *n_accepted, float *records, double *packets, void *stream);
int ionode_dopri5_backward_sweep_sse(const ionode_desc *d, int32_t it_begin, int32_t it_end, int32_t n_iter, const float *grad_image,
                                     const double *params, const double *prot_v, const double *prot_t, const int32_t *prot_of_traj,
                                     const double *t_eval, const int32_t *n_accepted, const double *sse_grad_y0, double *state,
                                     float *records, const double *packets, double *grad_params, double *grad_y0, void *stream);

/*
 * The gradient of the fused objective of either kind (IONODE_OBJECTIVE_*; since ABI 10, added later: new symbols only, ionode_desc and
 * every earlier entry point unchanged).  The forward is ionode_dopri5_objective() with the same `objective`, d->ckpt and d->sse_out
 * set; grad_sse[b] = dL/dsse_out[b] is the upstream gradient of that trajectory's sum, whatever its kind.  A sample's residual
 * r_k = i_k - sse_ref[protocol][k] enters the sweep through one weight w_k = d term / d r_k times grad_sse[b]
 * (csrc/ionode_interp.hpp residual_weight), dL/dy_k = w_k dr_k/dy_k:
 *   IONODE_OBJECTIVE_SSE  w_k = 2 grad_sse[b] r_k
 *   IONODE_OBJECTIVE_SAE  w_k = grad_sse[b] sign(r_k), sign(0) = 0 and sign(NaN) = NaN: the subgradient torch.abs's backward takes,
 *                         so that this is the derivative of n_out times the reference's torch.mean(torch.abs(pred_yo - data))
 * Only the two launches that form the weights know the kind:
 *   ionode_objective_backward()     ionode_dopri5_backward_sse() (closed-form models) plus `objective`;
 *   ionode_objective_backward_gc()  ionode_dopri5_backward_sse_gc() (NN-f / NN-d) plus `objective`; the rest of a chunk is
 *                                   ionode_dopri5_backward_recompute_sse(), ionode_dopri5_backward_sweep_sse() and
 *                                   ionode_grad_reduce_unit() for both kinds: the products and the walk never see a residual.
 * With IONODE_OBJECTIVE_SSE both are those entry points bit for bit.  IONODE_ERR_ARG, checked before any other argument and before
 * any launch, for another value of `objective`; every other refusal is the squares' entry point's, code and text.
 */
int ionode_objective_backward(const ionode_desc *d, int32_t objective, int32_t it_begin, int32_t it_end, int32_t n_iter, const double *params,
                              const double *prot_v, const double *prot_t, const int32_t *prot_of_traj, const double *t_eval,
                              const int32_t *n_accepted, const double *grad_sse, double *state, double *grad_params,
                              double *grad_y0, void *stream);
int ionode_objective_backward_gc(const ionode_desc *d, int32_t objective, int32_t it_begin, int32_t it_end, int32_t n_iter, const double *prot_v,
                                 const double *prot_t, const int32_t *prot_of_traj, const double *t_eval, const int32_t *n_accepted,
                                 const double *grad_sse, double *packets, double *sse_grad_y0, void *stream);

/*
 * Forward sensitivities (since ABI 10, added later: new symbols only, ionode_desc and every earlier entry point unchanged).  The
 * closed-form HH 2-state and 6-state models: the Jacobian of the current trace with respect to the rate parameters, di_k/dp_j -- PINTS
 * ForwardModelS1.simulateS1 -- and its Gauss-Newton sums against the fused objective's reference currents.  A tangent-mode sweep over
 * the forward launch's accepted-step checkpoints (csrc/ionode_tangent.hpp): the same discretise-then-differentiate rule as the
 * gradients above (accepted steps are constants, rejected attempts contribute nothing, FSAL and the dense output differentiated as
 * written), S = dy/dp zero at y0 (y0 is given), one lane per (trajectory, parameter), one launch, no chunking, no scratch state.  y_k is
 * re-evaluated from the step's checkpoint in the state dtype (the forward's bits), tangents are fp64 whatever the state dtype, and a
 * rate's derivative comes from the exponential the rate uses (no division by a parameter).
 *   (NPAR = 8 for HH2, 12 for MARKOV6; all pointers DEVICE)
 *   di_dp   [B][n_out][NPAR] fp64: di_k/dp_j, i as in the i_out epilogue; row k = 0 (y0) is zero
 *   jtr     [B][NPAR] fp64: sum_k di_k/dp_j r_k, r_k = i_k - sse_ref[protocol][k] as in the fused objective
 *   jtj     [B][NPAR][NPAR] fp64 (full, exactly symmetric): sum_k di_k/dp_j di_k/dp_l
 * Each may be NULL, not all three; jtr / jtj need d->sse_ref.  The trace and the sums come from one per-sample routine and differ by
 * summation order only (sample order per trajectory, the same bits whatever the batch).  n_accepted[b] = 0 (a failed trajectory):
 * zero rows.  Reads model, state_f32, sizes, protocol grid, v_oob, ckpt, ckpt_cap, obs_*, sse_ref and the optional v_at_outputs from
 * the descriptor of the forward launch that wrote the checkpoints (ionode_dopri5 with d->ckpt set).  Refusals, all before any launch,
 * text in ionode_grad_last_error(): IONODE_ERR_ARG for a NULL descriptor, a missing required buffer (params, prot_v, t_eval,
 * n_accepted, d->ckpt), all three outputs NULL, or sums without sse_ref; IONODE_ERR_UNSUPPORTED for NN-f / NN-d (their tangent walks
 * the two-phase sweep's packets and needs the weights and a chunk range: ionode_tangent_sweep_nn below) and for traj_per_image > 0.
 */
int ionode_tangent_sweep(const ionode_desc *d, const double *params, const double *prot_v, const double *prot_t,
                         const int32_t *prot_of_traj, const double *t_eval, const int32_t *n_accepted,
                         double *di_dp, double *jtr, double *jtj, void *stream);

/*
 * Forward sensitivities for NN-f / NN-d (since ABI 10, added later: new symbols only, ionode_desc and every earlier entry point
 * unchanged).  Outputs, rule of differentiation and dtypes as ionode_tangent_sweep (NPAR = 8; NN-f: the columns p1..p4 are exactly
 * zero).  The state the net sees is one scalar, a, and ionode_dopri5_backward_recompute already computes d net / d a of every
 * (trajectory, accepted step, stage) into its packets; so per chunk [it_begin, it_end) of the two-phase sweep's iterations this entry
 * point launches two kernels on `stream`: that recompute kernel without grad_y and without records (the packets' stage fields alone),
 * and the tangent walk over the packets (csrc/ionode_tangent_nn.hpp), forward in time.  Iteration numbering is the backward sweep's
 * (trajectory b runs its step s at it = n_accepted[b] - 1 - s, n_iter = max n_accepted + 1), so forward in time is DESCENDING: call
 * the chunks from [n_iter - c, n_iter) down to [0, c).  The same bits for any chunking and any batch around a trajectory.
 *   grad_image  ionode_grad_pack's image of the one weight set
 *   packets     [ceil(B/16)][it_end - it_begin][ionode_grad_packet_doubles()] fp64 scratch of the chunk
 *   state       [B][ionode_tangent_nn_state_doubles()] fp64: S, Kd_7 and the running sums between the launches; the launch with
 *               it_end == n_iter does not read it
 *   di_dp       rows are written as their steps are walked (row 0 and failed trajectories' rows by the launch with it_end == n_iter)
 *   jtr, jtj    written by the launch with it_begin == 0
 * Refusals, all before any launch, text in ionode_grad_last_error(): IONODE_ERR_ARG for a NULL descriptor, a missing required buffer
 * (grad_image, params, prot_v, t_eval, n_accepted, packets, state, d->ckpt), all three outputs NULL, sums without sse_ref (the trace
 * alone needs none), a bad iteration range or more than 65535 x 4 iterations; IONODE_ERR_UNSUPPORTED for the closed-form models
 * (ionode_tangent_sweep serves those), for traj_per_image > 0 and for a width or depth outside the backward sweep's compiled variants.
 */
size_t ionode_tangent_nn_state_doubles(void);
int ionode_tangent_sweep_nn(const ionode_desc *d, int32_t it_begin, int32_t it_end, int32_t n_iter, const float *grad_image,
                            const double *params, const double *prot_v, const double *prot_t, const int32_t *prot_of_traj,
                            const double *t_eval, const int32_t *n_accepted, double *packets, double *state,
                            double *di_dp, double *jtr, double *jtj, void *stream);

/* floats of one slab's partial gradient: [NP][4]{db0, dW0[.][0], dW0[.][1], 0} | L x (dW_l [NP][NP] + db_l [NP]) | dwl [NP] +
 * {dbl, 0, 0, 0}, NP = 16 * ceil(N / 16), rows/columns >= N are padding */
size_t ionode_grad_partial_floats(int32_t mlp_layers, int32_t mlp_width);

/* The slab count that makes one round of workgroups of ionode_grad_reduce() on the current device (256 compute units when there is
 * none): a slab costs mlp_layers x (column blocks of the width) heavy workgroups + one light one, N = 200 runs three workgroups per
 * compute unit.  It is the plan of the kernel that will run for the width: a width without a tuned reduce kernel (N does not pad to
 * 16, 112, 208 or 512), or any width under IONODE_GRAD_GENERIC=1, gets the run-time-width kernel's -- mlp_layers x
 * ceil(NT / 8) x ceil(NT / 16) heavy workgroups + one light one per slab (NT = ceil(N / 16)), two workgroups per compute unit.
 * Any n_slabs >= 1 is valid; this one is the fastest.  Since ABI 9. */
int32_t ionode_grad_reduce_slabs(int32_t mlp_layers, int32_t mlp_width, int64_t n_records);

/* partials[n_slabs][ionode_grad_partial_floats()] = per-slab sums over records [n_records * s / n_slabs, ...); asynchronous.
 * Every 1 <= N <= 512 at any depth: the tuned kernel where N pads to 16, 112, 208 or 512, the run-time-width kernel
 * otherwise (same records, same partial layout, every element one chain over the slab's records in record order).
 * IONODE_GRAD_GENERIC=1 in the environment (read on every call; a development switch) sends every width, and
 * ionode_grad_reduce_unit() with it, to the run-time-width kernel. */
int ionode_grad_reduce(int32_t mlp_layers, int32_t mlp_width, const float *records, int64_t n_records, int32_t n_slabs,
                       float *partials, void *stream);

/* ---------------------------------------------------------------------------------------------------------------------
 * MLP state-space regression step -- the reference's actual training loop, train-s1.py:891-909 /
 * train-d2.py:901-915:  p = net(x_av.float()) / netscale [+ model_dadt];  loss = MSELoss(reduction='sum')(p, y.float());
 * loss.backward(); Adam(lr 1e-3).step(); StepLR.step().  One iteration = ionode_regress_step -> ionode_grad_reduce ->
 * ionode_adam_step -> ionode_image_refresh, all asynchronous on one stream, no host synchronisation.
 * ------------------------------------------------------------------------------------------------------------------- */

/* Forward + backward of the net for every 16-row tile of x (fp32 MFMA, activations LDS-resident): one record per tile into
 * `records` ([ceil(n_rows/16)][ionode_grad_record_floats()]) and sum((p - y)^2) partials into loss_partials[n_workgroups]
 * (fp64).  x [n_rows][2], y [n_rows], offset [n_rows] or NULL: device fp32.  n_workgroups = persistent grid size (<= tiles).
 * Served shapes: 1..15 hidden layers, 1 <= N <= 512, and the tile's LDS (ionode_regress_plan) within a compute unit's 160 KiB.
 * N that pads to 16, 112, 208 or 512 runs its tuned kernel (N = 497..512: up to 10 layers); every other width runs the run-time-width
 * kernel (same arithmetic order, records bit-identical where both exist): all of 1..15 layers up to N = 416 and for N = 433..448, up to
 * 10 layers for N = 417..432, up to 14 for N = 449..464, up to 7 for N = 465..480, and none for N = 481..496 (IONODE_ERR_UNSUPPORTED, the message names the LDS need).
 * IONODE_GRAD_GENERIC=1 (read on every call; a development switch) sends every width to the run-time-width kernel. */
int ionode_regress_step(int32_t mlp_layers, int32_t mlp_width, const float *grad_image, const float *x, const float *offset,
                        const float *y, int32_t n_rows, float netscale, float *records, double *loss_partials,
                        int32_t n_workgroups, void *stream);

/* Pure host code (no HIP call; ABI 10, new symbol): the plan of ionode_regress_step() at (mlp_layers, mlp_width).
 * out = {1 if the run-time-width kernel serves the shape, 0 if a tuned one does; workgroups of the kernel per compute unit (the
 * persistent grid's size is that times the device's compute units, at most the tile count); LDS bytes per workgroup}.
 * IONODE_ERR_UNSUPPORTED with ionode_grad_last_error() set when nothing serves the shape. */
int ionode_regress_plan(int32_t mlp_layers, int32_t mlp_width, int32_t out[3]);

/* g[i] = sum over slabs of partials[s][padmap[i]] (flat state-dict order), then torch.optim.Adam's update (no amsgrad, no
 * weight decay), element-wise in fp32.  `step` counts from 1.  grad_out (optional) receives g; apply = 0 only gathers g. */
int ionode_adam_step(int32_t n_params, int32_t n_slabs, int32_t mlp_layers, int32_t mlp_width, const float *partials,
                     const int32_t *padmap, float *weights, float *exp_avg, float *exp_avg_sq, float lr, float beta1,
                     float beta2, float eps, int32_t step, float *grad_out, int32_t apply, void *stream);

/* grad_image[k] = weights[image_map[k] - 1] (image_map[k] == 0: padding).  image_map = ionode_grad_pack() of the values
 * 1, 2, ..., n_params (exact in fp32), converted to int32 by the caller. */
int ionode_image_refresh(int32_t mlp_layers, int32_t mlp_width, const int32_t *image_map, const float *weights,
                         float *grad_image, void *stream);

const char *ionode_grad_last_error(void);

/* ---------------------------------------------------------------------------------------------------------------------
 * Levenberg-Marquardt step for a population of candidates (closed-form models; new symbols, ABI stays 10).
 * A fit is a loop of two launches on one stream with no host synchronisation between them: the Gauss-Newton evaluation
 * (the checkpointed forward with the fused objective, then the tangent sweep's jtr / jtj) of the trial tensor, then the step
 * entry point below on its outputs, which decides about the trial points and writes the next trial tensor in place.
 *
 * Candidate c has nf free parameters x (columns free_idx[] of its NPAR rate parameters; the others are base[]) and the search
 * variables u = log x (log_parameters) or u = x.  Launch slot s holds candidate active[s] (active == NULL: candidate s): the
 * evaluation arrays and the trial tensor are indexed by slot -- the slot's P trajectories are rows s * P .. s * P + P - 1, one per
 * protocol -- and state / flag / iters by candidate.
 *
 * One call, for every slot whose candidate is running (flag 0):
 *   reduce   f_t = sum_p sse, g_t = 2 sum_p jtr[free], H_t = 2 sum_p jtj[free][free], each over p = 0 .. P - 1 in that order; a
 *            non-zero status on any of the P trajectories makes f_t = +inf.  log_parameters: g_j x_j and H_jl (x_j x_l).  Only the
 *            lower triangle of jtj is read; H is stored with its mirror and is exactly symmetric.
 *   decide   rho = (f - f_t) / pred, pred as the previous call stored it.  Accepted when f_t < f and rho > rho_accept: (u, x, f,
 *            g, H) <- trial, lam <- lam max(1/3, 1 - (2 rho - 1)^3), nu <- 2.  Otherwise lam <- lam nu, nu <- 2 nu (Nielsen's rule).
 *            A state with f = +inf -- the first call of a fit -- accepts any finite evaluation and leaves lam and nu alone.
 *   stop     IONODE_LM_FTOL: accepted with f - f_t <= ftol f;  IONODE_LM_GTOL: accepted and max_j |g_j| <= gtol over the variables
 *            that are not held (below);
 *            IONODE_LM_STALLED: lam > lam_max (after a rejection, or after the retries below);  IONODE_LM_XTOL: the projected step
 *            d has |d|_2 <= xtol (|u|_2 + xtol);  IONODE_LM_MAXITER: evaluations >= max_iter;  IONODE_LM_NONFINITE: the first
 *            evaluation is not finite (a non-finite start), or an accepted evaluation has a non-finite g or H.  Where several
 *            hold, the first of FTOL / NONFINITE, GTOL, STALLED, XTOL, MAXITER is stored.  A candidate whose flag is not 0 is frozen:
 *            a later call changes nothing of its state, flag or iters and writes its accepted x into its slot's trial rows.
 *   propose  (H + lam D) delta = -g by Cholesky, D_j = max(H_jj, IONODE_LM_FLOOR_REL max_l H_ll, IONODE_LM_FLOOR_ABS): Marquardt's
 *            diagonal scaling with a floor that keeps D positive for every finite H.  A pivot that is not a positive finite number,
 *            or a non-finite delta, sets lam <- lam nu, nu <- 2 nu and factors again, at most IONODE_LM_RETRIES times; then the
 *            candidate is IONODE_LM_STALLED.  A variable at a bound whose gradient points out of the box (u_j <= lo_j and g_j > 0,
 *            or u_j >= hi_j and g_j < 0) is held: delta_j = 0 and its row and column leave the system.  Trial point ut = min(max(u + delta, lo), hi) in the search space, d = ut - u,
 *            xt = exp(ut) clamped into [lo, hi] (log_parameters; the library's deterministic exp) or xt = ut, and
 *            pred = -(g . d + d . H d / 2).  The slot's P trial rows are base[] with the free columns replaced by xt.
 *
 * state [n_cand][IONODE_LM_STATE_U + 6 nf + nf^2] fp64, per candidate:
 *   [IONODE_LM_STATE_F] f, [IONODE_LM_STATE_LAM] lam, [IONODE_LM_STATE_NU] nu, [IONODE_LM_STATE_PRED] pred, then from
 *   IONODE_LM_STATE_U on: u[nf], x[nf], g[nf], ut[nf], xt[nf], delta[nf] (the last solution of the damped system, before the
 *   projection), H[nf][nf].
 * To start a fit the caller sets f = +inf, lam = its initial damping, nu = 2, pred = 0, u = ut = the start in the search space,
 * x = xt = the start, the rest 0, flag = 0, iters = 0, and writes the starts into the trial tensor.
 *
 * The host entry point is the same per-candidate routine compiled for the host, on host pointers, no HIP call: its results equal
 * the kernel's bit for bit.  Results of a candidate do not depend on the other candidates of the call.
 * Refusals, all before any launch, text in ionode_grad_last_error(): IONODE_ERR_ARG for a NULL descriptor or buffer (active may
 * be NULL), n_free outside 1 .. IONODE_LM_MAX_FREE, n_params not 8 or 12, a free index outside n_params, lo > hi (or a NaN
 * bound), non-positive bounds with log_parameters, or n_cand / n_active / n_prot / max_iter < 1 or n_active > n_cand.
 * ------------------------------------------------------------------------------------------------------------------- */
#define IONODE_LM_MAX_FREE 12
#define IONODE_LM_RETRIES 8            /* factorisations after the first that one call may try */
#define IONODE_LM_FLOOR_REL 0x1p-20    /* D_j >= this times the largest diagonal entry of H */
#define IONODE_LM_FLOOR_ABS 0x1p-256   /* D_j >= this, whatever H */
#define IONODE_LM_STATE_F 0
#define IONODE_LM_STATE_LAM 1
#define IONODE_LM_STATE_NU 2
#define IONODE_LM_STATE_PRED 3
#define IONODE_LM_STATE_U 4
#define IONODE_LM_RUNNING 0
#define IONODE_LM_GTOL 1
#define IONODE_LM_XTOL 2
#define IONODE_LM_FTOL 3
#define IONODE_LM_STALLED 4
#define IONODE_LM_MAXITER 5
#define IONODE_LM_NONFINITE 6

typedef struct ionode_lm_desc {
  int32_t n_cand;          /* candidates the state arrays hold */
  int32_t n_active;        /* launch slots of this call, <= n_cand */
  int32_t n_prot;          /* P: trajectories per candidate */
  int32_t n_params;        /* NPAR: 8 (HH 2-state) or 12 (6-state) */
  int32_t n_free;          /* nf */
  int32_t log_parameters;
  int32_t max_iter;        /* evaluations a candidate may use */
  int32_t reserved;
  int32_t free_idx[IONODE_LM_MAX_FREE];
  double base[IONODE_LM_MAX_FREE];
  double lo[IONODE_LM_MAX_FREE], hi[IONODE_LM_MAX_FREE];   /* the box, in the parameters; -inf / +inf: none (log_parameters: lo > 0, DBL_MIN for none) */
  double gtol, xtol, ftol, rho_accept, lam_max;
} ionode_lm_desc;

int ionode_lm_step(const ionode_lm_desc *d, const int32_t *active, const double *sse, const double *jtr, const double *jtj,
                   const int32_t *status, double *state, int32_t *flag, int32_t *iters, double *trial, void *stream);
int ionode_lm_step_host(const ionode_lm_desc *d, const int32_t *active, const double *sse, const double *jtr, const double *jtj,
                        const int32_t *status, double *state, int32_t *flag, int32_t *iters, double *trial);

/* ---------------------------------------------------------------------------------------------------------------------
 * CMA-ES step for many independent runs (all four models, either objective kind; new symbols, ABI stays 10).
 * The reference fits its candidate models with PINTS' CMA-ES (train-d0.py:508-540).  Here K runs -- restarts, cells, start
 * points, seeds -- advance together, each with lambda candidates per generation and P protocols per candidate.  A generation
 * of all runs is two launches on one stream with no host synchronisation between them: the forward solve with the fused
 * objective (either kind) on the trial tensor [n_active * lambda * P][NPAR], then the step entry point below on its
 * per-trajectory values and statuses: the TELL of the generation just evaluated, then the ASK of the next, which overwrites
 * the trial tensor in place.  A run whose generation counter iters[run][0] is 0 skips the tell: the first call only samples.
 *
 * Launch slot s holds run active[s] (active == NULL: run s).  value / status / trial are indexed by slot -- candidate k of the
 * slot owns rows (s lambda + k) P .. + P - 1, one per protocol -- and state / flag / iters by run.
 *
 * The algorithm is Hansen's (mu/mu_w, lambda)-CMA-ES ("The CMA Evolution Strategy: A Tutorial", arXiv 1604.00772) with positive
 * weights only, in n = n_free search variables u = log x (log_parameters) or u = x:
 *   mu = floor(lambda / 2), w_i = (ln(mu + 1/2) - ln i) / sum, i = 1 .. mu, mu_eff = 1 / sum w_i^2,
 *   c_sigma = (mu_eff + 2) / (n + mu_eff + 5), d_sigma = 1 + 2 max(0, sqrt((mu_eff - 1) / (n + 1)) - 1) + c_sigma,
 *   c_c = (4 + mu_eff / n) / (n + 4 + 2 mu_eff / n), c_1 = 2 / ((n + 1.3)^2 + mu_eff),
 *   c_mu = min(1 - c_1, 2 (mu_eff - 2 + 1 / mu_eff) / ((n + 2)^2 + mu_eff)), chi_n = sqrt(n) (1 - 1 / (4 n) + 1 / (21 n^2)).
 *   (The default lambda, 4 + floor(3 ln n), is the caller's to set: lambda arrives in the descriptor, 2 .. IONODE_CMAES_MAX_LAMBDA.)
 *   tell   f_k = sum_p value, p = 0 .. P - 1 in that order; a non-zero status on any of the P rows, or a NaN, makes f_k = +inf.
 *          Rank by (f, k).  The best-ever (f, x) of the run is updated.  Fewer than mu finite values: IONODE_CMAES_NONFINITE and
 *          nothing else of the state moves.  Otherwise, with y_k = (u_k - m) / sigma of the points AS EVALUATED (after redraws
 *          and clipping) and y_w = sum w_rank(k) y_k:  m <- m + sigma y_w;  p_sigma <- (1 - c_sigma) p_sigma + sqrt(c_sigma (2 -
 *          c_sigma) mu_eff) B D^-1 B^T y_w;  sigma <- sigma exp(min(1, (c_sigma / d_sigma) (|p_sigma| / chi_n - 1)));
 *          h_sigma = |p_sigma| / sqrt(1 - (1 - c_sigma)^(2 g)) / chi_n < 1.4 + 2 / (n + 1), g the number of tells so far;
 *          p_c <- (1 - c_c) p_c + h_sigma sqrt(c_c (2 - c_c) mu_eff) y_w;  C <- (1 - c_1 - c_mu + (1 - h_sigma) c_1 c_c (2 - c_c)) C
 *          + c_1 p_c p_c^T + c_mu sum w_rank(k) y_k y_k^T, symmetrised first and written as a symmetric pair;  then C = B D^2 B^T
 *          by cyclic Jacobi, every generation: row-cyclic sweeps over (p, q), p < q, a rotation wherever |a_pq| > 2^-54
 *          sqrt(|a_pp a_qq|), until a sweep rotates nothing or IONODE_CMAES_JACOBI_SWEEPS sweeps are done.  D_j = sqrt(max(eigenvalue, 0)),
 *          in the order the diagonal leaves them (not sorted).
 *   stop   the first that holds of IONODE_CMAES_NONFINITE (above, or a non-finite sigma or D), IONODE_CMAES_UNCHANGED (the best
 *          f did not fall by more than unchanged_threshold below the last significant best for unchanged_iters tells: PINTS' rule),
 *          IONODE_CMAES_TOLX (sigma max_j max(sqrt(C_jj), |p_c,j|) < tolx), IONODE_CMAES_CONDITION (max D / min D >
 *          IONODE_CMAES_CONDITION_LIMIT), IONODE_CMAES_MAXITER (tells >= max_iter).  A run whose flag is not 0 is frozen: a later
 *          call changes nothing of its state, flag or iters and writes its best x into all of its slot's trial rows.
 *   ask    candidate k, generation g: z from the generator below, u_k = m + sigma B (D z).  A point outside the box is
 *          redrawn whole with the next attempt index, IONODE_CMAES_RESAMPLES times at most, then clipped into the box.
 *          x_k = exp(u_k) clamped into [lo, hi] (log_parameters; the library's deterministic exp) or x_k = u_k.  u_k and x_k are
 *          kept in the state; the candidate's P trial rows are base[] with the free columns replaced by x_k.
 *
 * Random numbers: Philox4x32-10 (Salmon et al. 2011), counter (run_base + run, generation, candidate, pair + 65536 attempt), key (low, high
 * word of seed); words 0, 1 and 2, 3 give two uniforms ((w_hi 2^21 + (w_lo >> 11)) + 1/2) 2^-53 and Wichura's AS241 PPND16 turns
 * each into a normal deviate: coordinates 2 pair and 2 pair + 1.  Its logarithm is the library's own operation sequence (exponent
 * by bit extraction, mantissa in [sqrt(1/2), sqrt(2)], the atanh series in s = (m - 1) / (m + 1) to s^23): a draw is a pure
 * function of its indices, the same on the host and on the device, whoever shares the launch.
 *
 * state [n_run][IONODE_CMAES_STATE_M + 8 n + 3 n^2 + 2 lambda + 2 lambda n] fp64, per run: the scalars IONODE_CMAES_STATE_SIGMA ..
 * _COND (sigma, sigma before the last tell, best f, the last significant best f, tells since then, h_sigma, finite values of the
 * last tell, the flag, the last rotation's c and s, the rotations of the last sweep, max D / min D), then from IONODE_CMAES_STATE_M
 * on: m, m before the last tell, p_c, p_sigma, D, best x, y_w, D^-1 B^T y_w [n each]; C, B, the Jacobi work matrix [n][n each,
 * row-major]; f, the weight each candidate's rank earned [lambda each]; the points u [lambda][n] and x [lambda][n].
 * To start a fit the caller sets sigma = sigma0, best f = last significant best = +inf, m = the start in the search space,
 * best x = the start, D_j = s_j, C = diag(s_j^2), B = I, the rest 0, flag = 0, iters = 0.  iters [n_run][2]: generations sampled,
 * evaluations told.
 *
 * Execution model: one 64-lane workgroup per run, the run's state staged in LDS, the step a sequence of phases with a workgroup
 * barrier between them; in a phase a lane writes only elements it owns and every sum is one lane's, in one written order.  The
 * host entry point runs the same phase functions, lane after lane, phase after phase, on host pointers, no HIP call: its results
 * equal the kernel's bit for bit, and a run's results do not depend on the other runs of the call.
 * Refusals, all before anything is touched, text in the gradient path's error string: IONODE_ERR_ARG for a NULL descriptor
 * or buffer (active may be NULL), n_free outside 1 .. IONODE_LM_MAX_FREE, lambda outside 2 .. IONODE_CMAES_MAX_LAMBDA, n_params outside
 * 1 .. IONODE_LM_MAX_FREE, a free index outside n_params, lo > hi (or a NaN bound), non-positive bounds with log_parameters, or
 * n_run / n_active / n_prot / max_iter / unchanged_iters < 1 or n_active > n_run.
 * ------------------------------------------------------------------------------------------------------------------- */
#define IONODE_CMAES_MAX_LAMBDA 64
#define IONODE_CMAES_RESAMPLES 8          /* redraws of a point outside the box before it is clipped */
#define IONODE_CMAES_JACOBI_SWEEPS 30
#define IONODE_CMAES_CONDITION_LIMIT 1e7  /* max D / min D */
#define IONODE_CMAES_STATE_SIGMA 0
#define IONODE_CMAES_STATE_SIGMA_OLD 1
#define IONODE_CMAES_STATE_BEST_F 2
#define IONODE_CMAES_STATE_F_SIG 3
#define IONODE_CMAES_STATE_UNCHANGED 4
#define IONODE_CMAES_STATE_HSIG 5
#define IONODE_CMAES_STATE_NFINITE 6
#define IONODE_CMAES_STATE_FLAG 7
#define IONODE_CMAES_STATE_ROT_C 8
#define IONODE_CMAES_STATE_ROT_S 9
#define IONODE_CMAES_STATE_NROT 10
#define IONODE_CMAES_STATE_COND 11
#define IONODE_CMAES_STATE_M 12
#define IONODE_CMAES_RUNNING 0
#define IONODE_CMAES_MAXITER 1
#define IONODE_CMAES_UNCHANGED 2
#define IONODE_CMAES_TOLX 3
#define IONODE_CMAES_CONDITION 4
#define IONODE_CMAES_NONFINITE 5

typedef struct ionode_cmaes_desc {
  int32_t n_run;           /* K: runs the state arrays hold */
  int32_t n_active;        /* launch slots of this call, <= n_run */
  int32_t lambda;          /* candidates per generation, 2 .. IONODE_CMAES_MAX_LAMBDA */
  int32_t n_prot;          /* P: trajectories per candidate */
  int32_t n_params;        /* NPAR: 8 (HH 2-state, NN-f, NN-d rate parameters) or 12 (6-state) */
  int32_t n_free;          /* n */
  int32_t log_parameters;
  int32_t max_iter;        /* generations a run may be told */
  int32_t unchanged_iters;
  int32_t run_base;        /* index of the state arrays' first run among all runs of the fit (sharding): the generator sees run_base + run */
  double unchanged_threshold, tolx;
  int64_t seed;
  int32_t free_idx[IONODE_LM_MAX_FREE];
  double base[IONODE_LM_MAX_FREE];
  double lo[IONODE_LM_MAX_FREE], hi[IONODE_LM_MAX_FREE];   /* the box, in the parameters (log_parameters: lo > 0) */
} ionode_cmaes_desc;

int ionode_cmaes_step(const ionode_cmaes_desc *d, const int32_t *active, const double *value, const int32_t *status, double *state,
                      int32_t *flag, int32_t *iters, double *trial, void *stream);
int ionode_cmaes_step_host(const ionode_cmaes_desc *d, const int32_t *active, const double *value, const int32_t *status, double *state,
                           int32_t *flag, int32_t *iters, double *trial);
/* Pure host code, for tests of the generator: the four Philox words and the two normal deviates of one draw, and the step's
 * logarithm (finite x > 0; 0 gives -inf, x < 0 or NaN gives NaN, +inf gives +inf). */
void ionode_cmaes_draw_host(int64_t seed, int32_t run, int32_t generation, int32_t candidate, int32_t pair, int32_t attempt,
                            uint32_t words[4], double z[2]);
double ionode_cmaes_log_host(double x);

/* ---------------------------------------------------------------------------------------------------------------------
 * Adaptive Metropolis step for many independent chains (all four models; new symbols, ABI stays 10).
 * What follows a fit of noisy data in the reference's workflow (noise_sigma = 0.1, train-d0.py:487-492) is posterior sampling
 * under a Gaussian noise model.  Here K chains -- restarts for R-hat, start points, seeds -- advance together, each with P
 * protocols.  An iteration of all chains is two launches on one stream with no host synchronisation between them: the forward
 * solve with the fused sum of squares on the trial tensor [n_active * P][NPAR], then the step entry point below on its
 * per-trajectory values and statuses: the TELL of that evaluation (the Metropolis decision, the adaptation, a recorded sample, the
 * stop flags), then the PROPOSAL of the next, which overwrites the trial tensor in place.
 *
 * Launch slot s holds chain active[s] (active == NULL: chain s).  value / status / trial are indexed by slot -- the slot's P
 * trajectories are rows s P .. s P + P - 1, one per protocol -- and state / flag / iters / samples by chain.
 *
 * The algorithm is adaptive Metropolis (Haario, Saksman, Tamminen 2001) with global adaptive scaling, as Algorithm 4 of Andrieu
 * and Thoms, "A tutorial on adaptive MCMC" (2008).  Coordinates: the n_free free rate parameters as u_j = log x_j (log_parameters)
 * or u_j = x_j and, with sample_sigma, one more, the last: u_sigma = log sigma (always the logarithm); n = n_free + sample_sigma <=
 * IONODE_MCMC_MAX_DIM.  With S = sum_p value, p = 0 .. P - 1 in that order (a non-zero status on any of the P rows, or a NaN,
 * makes S = +inf) and N = n_samples (P times the samples of a trace):
 *   target   lp = -N u_sigma - (S / 2) exp(-2 u_sigma); without sample_sigma u_sigma = log sigma of the descriptor's sigma.  The
 *            prior is uniform over the box [lo, hi] x [sigma_lo, sigma_hi] IN THE SEARCH SPACE (log-uniform in x under
 *            log_parameters, log-uniform in sigma); outside the box lp = -inf.  The bounds are required to be finite.
 *   t = 0    (iters[chain][0] == 0) the evaluation is the start's: lp becomes its log-posterior; IONODE_MCMC_NONFINITE if the
 *            start is outside the box or lp is not finite.  Nothing is decided, nothing adapts.
 *   tell     t >= 1: alpha = 0 if the proposal was outside the box (IONODE_MCMC_STATE_OUTSIDE, left by the previous call) or
 *            lp_t is not finite, otherwise alpha = exp(min(lp_t - lp, 0)).  Accepted iff alpha > 0 and log w < lp_t - lp, w the
 *            uniform below: then (u, x, lp) <- (ut, xt, lp_t) and iters[chain][1] goes up.
 *   adapt    t >= adapt_start: k = t - adapt_start + 2 (it starts at 2: gamma = 1 would collapse C to zero), gamma =
 *            exp(-eta log k); mu <- mu + gamma (u - mu); C <- C + gamma ((u - mu)(u - mu)^T - C) with the mu just updated,
 *            written as a symmetric pair; log_lambda <- log_lambda + gamma (alpha - target_accept).  Before adapt_start none of
 *            the three moves.
 *   record   t % thin == 0 and t / thin < sample_cap: row t / thin of samples[chain] <- (x [n_free], sigma if sampled, lp): the
 *            parameters, not the search variables.  samples may be NULL.
 *   stop     the first that holds of IONODE_MCMC_NONFINITE (t = 0, above), IONODE_MCMC_DEGENERATE (a pivot of the factorisation
 *            below is not a positive finite number, or log_lambda or C is not finite; the factor in the state then stays the
 *            last good one), IONODE_MCMC_MAXITER (t >= max_iter).  A chain whose flag is not 0 is frozen: a later call changes
 *            nothing of its state, flag or iters and writes its current x into its slot's trial rows.
 *   propose  L L^T = exp(log_lambda) (C + epsilon I) by Cholesky, every call; ut = u + L z.  A ut outside the box is not redrawn:
 *            the OUTSIDE word is set and the slot's trial rows get the current x (its solve is wasted, its tell rejects without
 *            using the value).  Otherwise xt = exp(ut) clamped into [lo, hi] (the library's deterministic exp) or xt = ut, and
 *            the P trial rows are base[] with the free columns replaced by xt.  Sigma never enters the rows.
 *
 * Random numbers: the CMA-ES step's generator, unchanged -- Philox4x32-10, key (low, high word of seed), the same 53-bit
 * uniforms, PPND16 and logarithm.  The proposal evaluated at iteration t takes its deviates from the counters (chain_base + chain,
 * t, 0, pair): coordinates 2 pair and 2 pair + 1; the acceptance uniform of iteration t is the first uniform of (chain_base +
 * chain, t, 1, 0).  A draw is a pure function of its indices: compaction, the chain's company and the host mirror see the same.
 *
 * state [n_chain][IONODE_MCMC_STATE_U + 5 n + 2 n^2] fp64, per chain: [IONODE_MCMC_STATE_LP] lp, [IONODE_MCMC_STATE_LOG_LAMBDA]
 * log_lambda, [IONODE_MCMC_STATE_OUTSIDE] 1 if the proposal in flight left the box, else 0, [IONODE_MCMC_STATE_ALPHA] the last
 * alpha; then from IONODE_MCMC_STATE_U on: u, ut, x, xt, mu [n each; with sample_sigma the last entry of x and xt is sigma]; C
 * [n][n], exactly symmetric; L [n][n], lower triangular, row-major both.
 * To start a chain the caller sets u = ut = mu = the start in the search space, x = xt = the start, C = diag(s_j^2), the rest 0,
 * flag = 0, iters = 0, and writes the start into the slot's trial rows.  iters [n_chain][2]: the iteration the chain is at (the
 * t of its next call; a stopped chain keeps the t it stopped at: max_iter decisions for IONODE_MCMC_MAXITER), accepted proposals.
 *
 * Execution model: one lane per chain, n a compile-time constant; no LDS, no cross-lane operation, no atomic, every sum in one
 * written order.  The host entry point runs the same per-chain routine on host pointers, no HIP call: its results equal the
 * kernel's bit for bit, and a chain's results do not depend on the other chains of the call or on its slot.
 * Refusals, all before anything is touched, text in the gradient path's error string: IONODE_ERR_ARG for a NULL descriptor or
 * buffer (active and samples may be NULL), n_free or n_params outside 1 .. IONODE_LM_MAX_FREE, a free index outside n_params,
 * lo > hi (or a NaN bound), an infinite bound, non-positive bounds with log_parameters, sigma_lo <= 0 or sigma_lo > sigma_hi (or an
 * infinite sigma_hi) with sample_sigma, sigma <= 0 without it, eta outside (0.5, 1], target_accept outside (0, 1), thin < 1, or
 * n_chain / n_active / n_prot / max_iter < 1 or n_active > n_chain.
 * ------------------------------------------------------------------------------------------------------------------- */
#define IONODE_MCMC_MAX_DIM 13
#define IONODE_MCMC_STATE_LP 0
#define IONODE_MCMC_STATE_LOG_LAMBDA 1
#define IONODE_MCMC_STATE_OUTSIDE 2
#define IONODE_MCMC_STATE_ALPHA 3
#define IONODE_MCMC_STATE_U 4
#define IONODE_MCMC_RUNNING 0
#define IONODE_MCMC_MAXITER 1
#define IONODE_MCMC_DEGENERATE 2
#define IONODE_MCMC_NONFINITE 3

typedef struct ionode_mcmc_desc {
  int32_t n_chain;         /* K: chains the state arrays hold */
  int32_t n_active;        /* launch slots of this call, <= n_chain */
  int32_t n_prot;          /* P: trajectories per chain */
  int32_t n_params;        /* NPAR: 8 (HH 2-state, NN-f, NN-d rate parameters) or 12 (6-state) */
  int32_t n_free;          /* nf */
  int32_t log_parameters;
  int32_t sample_sigma;    /* 1: log sigma is the last coordinate, within [sigma_lo, sigma_hi]; 0: sigma is fixed */
  int32_t max_iter;        /* Metropolis decisions a chain makes */
  int32_t adapt_start;     /* first iteration that adapts */
  int32_t thin;            /* every thin-th iteration is recorded */
  int32_t sample_cap;      /* rows of samples[chain] */
  int32_t chain_base;      /* index of the state arrays' first chain among all chains of the run (sharding): the generator sees chain_base + chain */
  int64_t seed;
  double n_samples;        /* N: residuals behind S, P times the samples of a trace */
  double sigma, sigma_lo, sigma_hi;
  double eta, target_accept, epsilon;
  int32_t free_idx[IONODE_LM_MAX_FREE];
  double base[IONODE_LM_MAX_FREE];
  double lo[IONODE_LM_MAX_FREE], hi[IONODE_LM_MAX_FREE];   /* the box, in the parameters: finite (log_parameters: lo > 0) */
} ionode_mcmc_desc;

int ionode_mcmc_step(const ionode_mcmc_desc *d, const int32_t *active, const double *value, const int32_t *status, double *state,
                     int32_t *flag, int32_t *iters, double *trial, double *samples, void *stream);
int ionode_mcmc_step_host(const ionode_mcmc_desc *d, const int32_t *active, const double *value, const int32_t *status, double *state,
                          int32_t *flag, int32_t *iters, double *trial, double *samples);

/* ---------------------------------------------------------------------------------------------------------------------
 * Manifold MALA step for many independent chains (closed-form models; new symbols, ABI stays 10).
 * The adaptive-Metropolis step above learns the posterior's shape from its own history.  Under the Gaussian noise model it
 * samples, J^T J / sigma^2 -- the Gauss-Newton matrix the tangent sweep sums for the Levenberg-Marquardt step -- is the expected
 * Fisher information: the local metric of the posterior, at every point, from iteration 0.  This step is the "simplified manifold
 * MALA" of Girolami and Calderhead (2011): a Metropolis-adjusted Langevin proposal preconditioned by that metric.  An iteration
 * of all chains is the Levenberg-Marquardt step's evaluation (the checkpointed forward with the fused sum of squares, then the
 * tangent sweep's jtr / jtj) of the trial tensor [n_active * P][NPAR], then the entry point below: the TELL of that evaluation,
 * then the PROPOSAL of the next, which overwrites the trial tensor in place.  No host synchronisation in between.
 *
 * Launch slot s holds chain active[s] (active == NULL: chain s).  sse / jtr / jtj / status (laid out as ionode_lm_step takes them)
 * and trial are indexed by slot -- the slot's P trajectories are rows s P .. s P + P - 1, one per protocol -- and state / flag /
 * iters / samples (laid out as ionode_mcmc_step takes them) by chain.
 *
 * Coordinates, target and prior are the adaptive-Metropolis step's: u_j = log x_j (log_parameters) or x_j for the n_free free
 * parameters and, with sample_sigma, u_sigma = log sigma as the last; n = n_free + sample_sigma <= IONODE_MCMC_MAX_DIM;
 * lp = -N u_sigma - (S / 2) exp(-2 u_sigma), S = sum_p sse over p = 0 .. P - 1 in that order (a non-zero status on any of the P
 * rows, or a NaN, makes S = +inf), N = n_samples; the prior is uniform over the finite box in the search space.
 * One call, for every slot whose chain is running (flag 0), at the chain's iteration t = iters[chain][0], in this order:
 *   metric   at the evaluated point (x, sigma) -- the start at t = 0, else the proposal: g_x = sum_p jtr, H_x = sum_p jtj over the
 *            free rows and columns, p in order (only the lower triangle of jtj is read); log_parameters: g_j x_j and H_jl (x_j x_l);
 *            grad_j = -g_j / sigma^2, G_jl = H_jl / sigma^2 (1 / sigma^2 = exp(-2 u_sigma), the library's exp); with sample_sigma
 *            grad_s = -N + S / sigma^2, G_ss = 2 N and zero cross terms: the expected information.  Then the ridge, a function of
 *            the point alone: G_jj += ridge max(G_jj, IONODE_LM_FLOOR_REL max_l G_ll, IONODE_LM_FLOOR_ABS), the Levenberg-Marquardt
 *            step's diagonal.  G = L_t L_t^T by Cholesky, lower triangle packed by rows, ld_t = sum_j log L_jj (the library's log).
 *            The metric "does not factor" when a pivot is not a positive finite number or an entry of grad or ld_t is not finite.
 *   t = 0    the evaluation is the start's: lp becomes its log-posterior.  IONODE_MALA_NONFINITE if the start is outside the box
 *            or lp is not finite; else IONODE_MALA_DEGENERATE if the metric does not factor; else (grad, L, ld) become its.
 *   tell     t >= 1, with eps = exp(log_eps) as the state holds it (the step size the proposal was drawn with): alpha = 0 if the
 *            proposal was outside the box (IONODE_MALA_STATE_OUTSIDE), lp_t is not finite or the metric does not factor.
 *            Otherwise y = L_t^-1 grad_t, d = L_t^-T y, mu_t = ut + (eps^2 / 2) d, v = L_t^T (u - mu_t),
 *            lq_r = (ld_t - n log_eps) - (v . v) / (2 eps^2), ratio = ((lp_t + lq_r) - lp) - lq_f with lq_f as the proposing call
 *            stored it (IONODE_MALA_STATE_LQF), alpha = exp(min(ratio, 0)) (0 for a NaN ratio).  Accepted iff alpha > 0 and
 *            log w < ratio, w the uniform below: then (u, x, lp, grad, L, ld) <- the proposal's and iters[chain][1] goes up.  A
 *            factor that failed is never stored.
 *   adapt    t >= 1: log_eps <- log_eps + exp(-eta log(t + 1)) (alpha - target_accept).  Nothing else adapts.
 *   record   t % thin == 0 and t / thin < sample_cap: row t / thin of samples[chain] <- (x [n_free], sigma if sampled, lp).
 *   stop     IONODE_MALA_NONFINITE and IONODE_MALA_DEGENERATE come from t = 0 only (a bad trial metric is a rejection, not a
 *            stop); IONODE_MALA_MAXITER: t >= max_iter.  A chain whose flag is not 0 is frozen: a later call changes nothing of
 *            its state, flag or iters and writes its current x into its slot's trial rows.
 *   propose  z: n normal deviates (below); eps = exp(log_eps) after the adaptation; y = L^-1 grad, w_j = (eps^2 / 2) y_j + eps z_j,
 *            ut = u + L^-T w, that is u + (eps^2 / 2) G^-1 grad + eps L^-T z; lq_f = (ld - n log_eps) - (z . z) / 2.  A ut outside
 *            the box (or not a number) is not redrawn: the OUTSIDE word is set and the slot's trial rows get the current x (its
 *            evaluation is wasted, its tell rejects without using the values).  Otherwise xt = exp(ut) clamped into [lo, hi] or
 *            xt = ut, and the P trial rows are base[] with the free columns replaced by xt.  Sigma never enters the rows.
 *
 * Random numbers: the CMA-ES step's generator, unchanged.  The proposal evaluated at iteration t takes its deviates from the
 * counters (chain_base + chain, t, 0, pair): coordinates 2 pair and 2 pair + 1; the acceptance uniform of iteration t is the first
 * uniform of (chain_base + chain, t, 1, 0).
 *
 * state [n_chain][IONODE_MALA_STATE_U + 5 n + n^2] fp64, per chain: [IONODE_MALA_STATE_LP] lp, [IONODE_MALA_STATE_LOG_EPS] log_eps,
 * [IONODE_MALA_STATE_OUTSIDE] 1 if the proposal in flight left the box, else 0, [IONODE_MALA_STATE_ALPHA] the last alpha,
 * [IONODE_MALA_STATE_LD] ld of the current point, [IONODE_MALA_STATE_LQF] lq_f of the proposal in flight; then from
 * IONODE_MALA_STATE_U on: u, ut, x, xt, grad [n each; with sample_sigma the last entry of x and xt is sigma]; L [n][n], lower
 * triangular, row-major.  To start a chain the caller sets log_eps = log eps0, u = ut = the start in the search space, x = xt =
 * the start, the rest 0, flag = 0, iters = 0, and writes the start into the slot's trial rows.  iters as the adaptive-Metropolis
 * step's.
 *
 * Execution model: one lane per chain, n a compile-time constant; one packed triangle live at a time (L_t through the tell, then
 * word by word L_t or the stored L for the proposal); no scratch, no LDS, no cross-lane operation, no atomic, every sum in one
 * written order.  The host entry point runs the same per-chain routine on host pointers, no HIP call: its results equal the
 * kernel's bit for bit, and a chain's results do not depend on the other chains of the call or on its slot.
 * Refusals, all before anything is touched, text in the gradient path's error string: those of ionode_mcmc_step (jtr and jtj are
 * required buffers too), and a ridge that is negative or not finite, or n_samples that is not positive and finite.
 * ------------------------------------------------------------------------------------------------------------------- */
#define IONODE_MALA_STATE_LP 0
#define IONODE_MALA_STATE_LOG_EPS 1
#define IONODE_MALA_STATE_OUTSIDE 2
#define IONODE_MALA_STATE_ALPHA 3
#define IONODE_MALA_STATE_LD 4
#define IONODE_MALA_STATE_LQF 5
#define IONODE_MALA_STATE_U 6
#define IONODE_MALA_RUNNING 0
#define IONODE_MALA_MAXITER 1
#define IONODE_MALA_DEGENERATE 2
#define IONODE_MALA_NONFINITE 3

typedef struct ionode_mala_desc {
  int32_t n_chain;         /* K: chains the state arrays hold */
  int32_t n_active;        /* launch slots of this call, <= n_chain */
  int32_t n_prot;          /* P: trajectories per chain */
  int32_t n_params;        /* NPAR: 8 (HH 2-state) or 12 (6-state) */
  int32_t n_free;          /* nf */
  int32_t log_parameters;
  int32_t sample_sigma;    /* 1: log sigma is the last coordinate, within [sigma_lo, sigma_hi]; 0: sigma is fixed */
  int32_t max_iter;        /* Metropolis-Hastings decisions a chain makes */
  int32_t thin;            /* every thin-th iteration is recorded */
  int32_t sample_cap;      /* rows of samples[chain] */
  int32_t chain_base;      /* index of the state arrays' first chain among all chains of the run (sharding): the generator sees chain_base + chain */
  int32_t reserved;
  int64_t seed;
  double n_samples;        /* N: residuals behind S, P times the samples of a trace */
  double sigma, sigma_lo, sigma_hi;
  double eta, target_accept, ridge;
  int32_t free_idx[IONODE_LM_MAX_FREE];
  double base[IONODE_LM_MAX_FREE];
  double lo[IONODE_LM_MAX_FREE], hi[IONODE_LM_MAX_FREE];   /* the box, in the parameters: finite (log_parameters: lo > 0) */
} ionode_mala_desc;

int ionode_mala_step(const ionode_mala_desc *d, const int32_t *active, const double *sse, const double *jtr, const double *jtj,
                     const int32_t *status, double *state, int32_t *flag, int32_t *iters, double *trial, double *samples, void *stream);
int ionode_mala_step_host(const ionode_mala_desc *d, const int32_t *active, const double *sse, const double *jtr, const double *jtj,
                          const int32_t *status, double *state, int32_t *flag, int32_t *iters, double *trial, double *samples);

/* ---------------------------------------------------------------------------------------------------------------------
 * Multi-exponential fits of a(t) segments: the objective a CMA-ES run minimises, and the fitted curve with its derivatives
 * (new symbols, ABI stays 10).
 * The reference's real-data route turns a measured current into a(t), da/dt and d2a/dt2 with one tri- or bi-exponential fit
 * per constant-voltage segment (train-r1.py:427-451: tri_exp / bi_exp and their derivatives; :487-494: f = sqrt(mean((model -
 * a)^2)) minimised per segment) and hands its hardest segments, the -90 mV steps, to PINTS' CMA-ES (train-r1.py:553-555, :641;
 * train-r2.py:595, :671).  Here K runs -- every segment of a protocol, each restarted a few times -- advance together: a
 * generation of all runs is ionode_multi_exp_objective on the trial tensor, then ionode_cmaes_step (above, n_prot = 1, n_params
 * = n_free = 5 or 7, log_parameters = 0) on its value / status, on one stream with no host synchronisation between them.
 *
 * The model.  n_params = 7 (tri-exponential, NT = 3) or 5 (bi-exponential, NT = 2); x = (A_1, b_1, ..., A_NT, b_NT, c) and
 *   m(t) = ((A_1 e_1 + A_2 e_2) + A_3 e_3) + c,  e_j = exp((-b_j) t),
 * summed from the first term with the offset added last (train-r1.py:427-451's order); exp is the library's deterministic
 * exponential (the step units' operation sequence: the only fma of these units is inside it).
 *
 * ionode_multi_exp_objective.  The indexing is ionode_cmaes_step's with P = 1: launch slot s holds run active[s] (active ==
 * NULL: run s), candidate k of the slot is row s lambda + k of trial [n_active lambda][n_params], value and status are indexed by
 * row.  Run r fits segment seg_of_run[r] (int32 [n_run]); several runs may share a segment: those are the restarts.  Segment g
 * owns the samples seg_off[g] .. seg_off[g + 1] - 1 (int64 [segments + 1]) of t_rel and a (fp64): t_rel is the time measured
 * from the segment's first fitted sample, a the activation estimate.  With n = the segment's samples
 *   value[row] = sqrt(sum_k (m(t_k) - a_k)^2 / n)   (the reference's f),  status[row] = 0;
 * an empty segment (n = 0, or a negative segment index) gives value = +inf, status = 1.  Non-finite parameters or an
 * exponential that overflows simply propagate (+inf or NaN in value, status 0): ionode_cmaes_step ranks a NaN as +inf.  A slot
 * whose active[] entry names no run is not touched.  The caller guarantees seg_of_run[r] < segments.
 * Execution model: one 256-lane workgroup per row.  Lane l sums the squared residuals of the samples k = l, l + 256, l + 512,
 * ... in ascending order.  The 256 partial sums are combined in ONE WRITTEN ORDER: inside each of the four wavefronts an
 * xor-butterfly, v_l <- v_l + v_(l xor s) for the strides s = 32, 16, 8, 4, 2, 1 in that order (both partners of an exchange
 * form the same sum, so after the last stride every lane of wavefront i holds w_i); then (w_0 + w_1) + (w_2 + w_3) through LDS,
 * the division by n and the square root.  No atomics, no scratch.
 *
 * ionode_multi_exp_eval.  x [n_seg][n_params] fp64, one fitted parameter vector per segment; segment g's full grid -- which
 * includes the samples the capacitance mask removed from the fit -- is full_off[g] .. full_off[g + 1] - 1 (int64 [n_seg + 1])
 * of t_full (fp64, measured from the segment's first FITTED sample).  For every sample the fitted curve and its first and
 * second time derivative (train-r1.py:430-438, :444-451) are written to a_fit / dadt / d2adt2: the term of order q is
 * ((-b_j)^q A_j) e_j with the coefficient formed first, (-b)^2 written b b; each sum starts from its first term; the offset is
 * added for q = 0 only.  One lane per sample: 32 workgroups of 256 lanes stride over a segment's grid.
 *
 * The _host entry points run the same functions on host pointers with no HIP call, lane after lane in the written order;
 * their results equal the kernels' bit for bit.
 * Refusals, all before anything is touched, text in the gradient path's error string: IONODE_ERR_ARG for a NULL buffer
 * (active may be NULL), n_params not 5 or 7, lambda outside 2 .. IONODE_CMAES_MAX_LAMBDA, n_run / n_active < 1 or n_active >
 * n_run, n_active lambda beyond 2^31 - 1 rows, n_seg < 1.
 * ------------------------------------------------------------------------------------------------------------------- */
int ionode_multi_exp_objective(int32_t n_run, int32_t n_active, int32_t lambda, int32_t n_params, const int32_t *active,
                               const int32_t *seg_of_run, const int64_t *seg_off, const double *t_rel, const double *a, const double *trial,
                               double *value, int32_t *status, void *stream);
int ionode_multi_exp_objective_host(int32_t n_run, int32_t n_active, int32_t lambda, int32_t n_params, const int32_t *active,
                                    const int32_t *seg_of_run, const int64_t *seg_off, const double *t_rel, const double *a,
                                    const double *trial, double *value, int32_t *status);
int ionode_multi_exp_eval(int32_t n_seg, int32_t n_params, const double *x, const int64_t *full_off, const double *t_full, double *a_fit,
                          double *dadt, double *d2adt2, void *stream);
int ionode_multi_exp_eval_host(int32_t n_seg, int32_t n_params, const double *x, const int64_t *full_off, const double *t_full, double *a_fit,
                               double *dadt, double *d2adt2);

/* ---------------------------------------------------------------------------------------------------------------------
 * Affine-invariant ensemble step: E independent ensembles of W walkers (all four models; new symbols, ABI stays 10).
 * The two samplers above run every chain alone.  Here a walker's proposal is built from the CURRENT POSITIONS of the other walkers
 * of its ensemble: Goodman and Weare's stretch move ("Ensemble samplers with affine invariance", Comm. App. Math. Comp. Sci. 5,
 * 2010) in its parallel form (Foreman-Mackey et al., "emcee", 2013), or its differential-evolution sibling (ter Braak, "A Markov
 * chain Monte Carlo version of the genetic algorithm Differential Evolution", Stat. Comput. 16, 2006) in the same two-halves
 * form.  Nothing is tuned, nothing adapts, and both moves are invariant under affine maps of the search space.
 *
 * Layout.  W is even, H = W / 2; half 0 is walkers 0 .. H - 1, half 1 walkers H .. W - 1.  A full iteration is two calls: half 0
 * moves with its partners drawn from half 1 as it stands, then half 1 with partners from half 0 -- a half's partners do not move
 * until it has been told, which is what makes moving a whole half at once a valid Metropolis-Hastings step.  A half-iteration of
 * all ensembles is two launches on one stream with no host synchronisation between them: the forward solve with the fused sum of
 * squares on the first E H P rows of the trial tensor, then the entry point below.
 *
 * Coordinates, target, prior, box, sigma and n_samples are ionode_mcmc_step's: u_j = log x_j (log_parameters) or x_j for the n_free
 * free parameters and, with sample_sigma, u_sigma = log sigma as the last; n = n_free + sample_sigma <= IONODE_MCMC_MAX_DIM;
 * lp = -N u_sigma - (S / 2) exp(-2 u_sigma), S = sum_p value over p = 0 .. P - 1 in that order (a non-zero status on any of the P
 * rows, or a NaN, makes S = +inf and lp = -inf), N = n_samples; the prior is uniform over the finite box in the search space.
 *
 * Calls.  An ensemble's counter t = iters[e][0] counts its calls.
 *   t = 0    value / status hold E W P rows, walker k of ensemble e at rows (e W + k) P ..: the starts' evaluation.  Every walker's
 *            lp is set and row 0 of samples written; IONODE_ENSEMBLE_NONFINITE if any start of the ensemble is outside the box or
 *            has a non-finite lp.  Otherwise the ASK for half 0, and t <- 1.
 *   t >= 1   value / status hold E H P rows, walker k of the half in turn at rows (e H + k) P ..  First the TELL for half
 *            (t - 1) % 2; then, behind a workgroup barrier, the ASK for half t % 2, and t <- t + 1.  The call with t = 2 max_iter
 *            tells half 1, sets IONODE_ENSEMBLE_MAXITER, asks nothing and leaves t: 2 max_iter + 1 calls make max_iter iterations.
 *   ask      walker k of half h, partners from half 1 - h at their current u, w1 and w2 the two uniforms below:
 *            IONODE_ENSEMBLE_STRETCH: j = min(floor(w1 H), H - 1); s = (a - 1) w2 + 1, z = (s s) / a, so z in [1 / a, a] with
 *              density proportional to 1 / sqrt(z); ut = u_j + z (u_k - u_j); lq = (n - 1) log z (the library's log).
 *            IONODE_ENSEMBLE_DE: two distinct partners ia = min(floor(w1 H), H - 1), ib = (ia + 1 + min(floor(w2 (H - 1)), H - 2))
 *              mod H; ut = (u_k + gamma (u_ia - u_ib)) + jitter xi, xi one standard normal deviate per coordinate; lq = 0.
 *            A ut outside the box (or not a number) is not redrawn: the walker's OUTSIDE word is set and its trial rows get its
 *            current x (that solve is wasted; its tell rejects without using the value).  Otherwise xt = exp(ut) clamped into
 *            [lo, hi] (the library's deterministic exp) or xt = ut, and the walker's P trial rows, (e H + k) P .., are base[] with
 *            the free columns replaced by xt.  Sigma never enters the rows.
 *   tell     lp_t from S at ut.  alpha = 0 if OUTSIDE or lp_t is not finite; otherwise ratio = (lp_t + lq) - lp.  Accepted iff
 *            alpha > 0 and log w3 < ratio: then (u, x, lp) <- (ut, xt, lp_t) and accepted[e][walker] goes up.
 *   record   after the tell of half 1 of full iteration i = t / 2 (t even, >= 2): if i % thin == 0 and i / thin < sample_cap, row
 *            i / thin of samples[e][walker] <- (x [n_free], sigma if sampled, lp) for all W walkers.  samples may be NULL.
 *   frozen   an ensemble whose flag is not 0: a later call changes nothing of its state, flag, iters, accepted or samples and
 *            writes the current x of half 0's walkers into its H slots of the trial rows (as does the call that flags it).
 * There is no active list and no compaction: nothing stops early.  iters [E][2]: (t, full iterations told).
 *
 * Random numbers: the CMA-ES step's generator, unchanged -- Philox4x32-10, key (low, high word of seed), the same 53-bit uniforms,
 * PPND16 and logarithm.  The counter is (ensemble_base + e, t, walker, pair + 65536 role), t the counter of the call that draws and
 * walker = 0 .. W - 1: role 0, pair 0: w1 = uniform of words 0, 1 and w2 = of words 2, 3 (the ask of call t); role 1, pair 0: w3 =
 * uniform of words 0, 1 (the tell of call t); role 2, pair p: xi of coordinates 2 p and 2 p + 1 (the DE ask of call t); role 3,
 * t = 0: the driver's spread of the starts.  A draw is a pure function of its indices: an ensemble's results do not depend on the
 * other ensembles of the call, and ensemble e under base b equals ensemble 0 under base b + e.
 *
 * state [E][W][IONODE_ENSEMBLE_STATE_U + 4 n] fp64, per walker: [IONODE_ENSEMBLE_STATE_LP] lp, [IONODE_ENSEMBLE_STATE_LQ] lq of
 * the proposal in flight, [IONODE_ENSEMBLE_STATE_OUTSIDE] 1 if it left the box, else 0; then u, ut, x, xt [n each; with
 * sample_sigma the last entry of x and xt is sigma].  flag [E], iters [E][2], accepted [E][W] int32.  To start, the caller writes
 * u = ut = the starts in the search space, x = xt = the starts, the starts into all E W P trial rows, and zeroes the rest.
 * trial [E W P][n_params] (calls t >= 1 touch its first E H P rows only); samples [E][W][sample_cap][n + 1].
 *
 * Execution model: one 256-lane workgroup per ensemble, the walkers of the half in turn strided over its lanes, n a compile-time
 * constant (1 .. 13).  Tell, __syncthreads(), ask: the partners' u are read from the state where the tell left them.  The one
 * cross-lane datum besides, "a start is bad" at t = 0, is one LDS word every finder stores 1 into.  No atomics, no scratch, every
 * sum in one written order.  The host entry point runs the same per-ensemble routine on host pointers as a single lane, no HIP
 * call: its results equal the kernel's bit for bit.
 * IONODE_ENSEMBLE_MAX_WALKERS: a half in eight passes of the workgroup.  More partners than 2048 buy the moves nothing, and past it
 * one workgroup serialises work that further ensembles would spread over the compute units: split a larger population into more
 * ensembles.
 * Refusals, all before anything is touched, text in the gradient path's error string: IONODE_ERR_ARG for a NULL descriptor or
 * buffer (samples may be NULL), everything ionode_mcmc_step refuses about n_free, n_params, the free indices, the box, sigma,
 * thin and the counts (n_ens, n_prot, max_iter < 1; max_iter above 2^30 - 1), W odd, W < 2 (n + 1) (a half must affinely span the
 * search space, or the moves stay in a subspace for ever), H < 2 for the DE move, W above IONODE_ENSEMBLE_MAX_WALKERS, n_ens W
 * n_prot beyond 2^31 - 1 rows, a <= 1 (or not finite), gamma or jitter not finite, jitter < 0, an unknown move, a negative
 * sample_cap, n_samples not positive and finite.
 * ------------------------------------------------------------------------------------------------------------------- */
#define IONODE_ENSEMBLE_MAX_WALKERS 4096
#define IONODE_ENSEMBLE_STATE_LP 0
#define IONODE_ENSEMBLE_STATE_LQ 1
#define IONODE_ENSEMBLE_STATE_OUTSIDE 2
#define IONODE_ENSEMBLE_STATE_U 3
#define IONODE_ENSEMBLE_RUNNING 0
#define IONODE_ENSEMBLE_MAXITER 1
#define IONODE_ENSEMBLE_NONFINITE 2
#define IONODE_ENSEMBLE_STRETCH 0
#define IONODE_ENSEMBLE_DE 1

typedef struct ionode_ensemble_desc {
  int32_t n_ens;           /* E: ensembles the arrays hold, all of them launched */
  int32_t n_walkers;       /* W: walkers of an ensemble, even */
  int32_t n_prot;          /* P: trajectories per walker */
  int32_t n_params;        /* NPAR: 8 (HH 2-state, NN-f, NN-d rate parameters) or 12 (6-state) */
  int32_t n_free;          /* nf */
  int32_t log_parameters;
  int32_t sample_sigma;    /* 1: log sigma is the last coordinate, within [sigma_lo, sigma_hi]; 0: sigma is fixed */
  int32_t max_iter;        /* full iterations: every walker decides max_iter times */
  int32_t thin;            /* every thin-th full iteration is recorded */
  int32_t sample_cap;      /* rows of samples[e][walker] */
  int32_t ensemble_base;   /* index of the arrays' first ensemble among all ensembles of the run (sharding): the generator sees ensemble_base + e */
  int32_t move;            /* IONODE_ENSEMBLE_STRETCH or IONODE_ENSEMBLE_DE */
  int64_t seed;
  double n_samples;        /* N: residuals behind S, P times the samples of a trace */
  double sigma, sigma_lo, sigma_hi;
  double a;                /* stretch: z in [1 / a, a]; > 1 (Goodman and Weare's 2) */
  double gamma;            /* DE: the difference's factor (ter Braak's 2.38 / sqrt(2 n)) */
  double jitter;           /* DE: standard deviation of the added noise, >= 0 */
  int32_t free_idx[IONODE_LM_MAX_FREE];
  double base[IONODE_LM_MAX_FREE];
  double lo[IONODE_LM_MAX_FREE], hi[IONODE_LM_MAX_FREE];   /* the box, in the parameters: finite (log_parameters: lo > 0) */
} ionode_ensemble_desc;

int ionode_ensemble_step(const ionode_ensemble_desc *d, const double *value, const int32_t *status, double *state, int32_t *flag,
                         int32_t *iters, int32_t *accepted, double *trial, double *samples, void *stream);
int ionode_ensemble_step_host(const ionode_ensemble_desc *d, const double *value, const int32_t *status, double *state, int32_t *flag,
                              int32_t *iters, int32_t *accepted, double *trial, double *samples);

/* ---------------------------------------------------------------------------------------------------------------------
 * Training through the solve: the update that follows the backward sweep (NN-f / NN-d; new symbols, ABI stays 10).
 * The reference trains its nets by regression on da/dt estimates and only WATCHES the prediction loss
 * torch.mean(torch.abs(pred_yo - data)) (train-r1.py:930-945).  The fused objective and its sweep give that loss and dL/dW through
 * the dopri5 solve; the three launches below turn the sweep's fp64 accumulator into one guarded, norm-clipped torch.optim.Adam
 * step on weights that stay in device memory, and rebuild both weight images from them.  All three are asynchronous on the
 * caller's stream, none reads anything back, and the decision whether the step happens is taken on the device.
 * n = the floats of the flat state dict of (mlp_layers, mlp_width): 3 N + L (N N + N) + N + 1.
 *
 * ionode_train_grad_norm.  grad[i] = (float)acc[padmap[i]], i = 0 .. n - 1: acc is the padded fp64 partial gradient (layout:
 * ionode_grad_partial_floats), padmap int32 [n] the flat-to-padded map (an entry that names no word of acc gives 0).
 * norm_partials [ionode_train_norm_partials(n)] fp64 receives sums of grad[i]^2: workgroup g of 256 lanes owns the elements
 * 4096 g .. 4096 g + 4095, lane l sums the squares (in fp64) of i = 4096 g + l, + 256, ... ascending, and the 256 lane sums are
 * combined in ONE WRITTEN ORDER: inside each of the four wavefronts the xor-butterfly v_l <- v_l + v_(l xor s), s = 32, 16, 8, 4, 2,
 * 1, then (w_0 + w_1) + (w_2 + w_3) through LDS.  The grid is a function of n alone.
 *
 * ionode_train_apply.  norm = sqrt(norm_partials[0] + norm_partials[1] + ...) in index order.  loss [1] fp64: the loss the
 * gradient belongs to.  state_in / state_out: two blocks of IONODE_TRAIN_STATE_DOUBLES fp64; the call READS state_in and WRITES the
 * whole of state_out (the caller alternates two blocks, so that no workgroup reads what another has written):
 *   [IONODE_TRAIN_STATE_T] applied steps t, [.._BETA1_T] beta1^t, [.._BETA2_T] beta2^t, [.._SKIPPED] skipped calls, and of the
 *   call that wrote the block: [.._LOSS] its loss, [.._NORM] its norm, [.._SCALE] its clip scale (0 when skipped), [.._APPLIED] 1 or 0.
 *   A fresh block is {0, 1, 1, 0, 0, 0, 0, 0}.
 * If norm or loss is not finite the call is SKIPPED: weights, exp_avg, exp_avg_sq, t and the products stay, SKIPPED goes up by
 * one.  Otherwise t <- t + 1, the products are advanced by ONE multiplication each (there is no pow: beta^t is the product of t
 * factors, in fp64, of the betas as given: the doubles torch.optim.Adam raises to the power t), scale = min(1, max_norm / (norm + 1e-6)) -- torch.nn.utils.clip_grad_norm_; max_norm <= 0: no clip, scale
 * exactly 1 -- and with g = grad[i] * (float)scale, element-wise in fp32, ionode_adam_step's operations in its order:
 *   m = m + (g - m) (1 - beta1);  v = v beta2 + (g g) (1 - beta2)        (beta2, 1 - beta1, 1 - beta2: formed in fp64, rounded to fp32 once)
 *   w = w - (lr / bc1) (m / (sqrt(v) / bc2s + eps)),  bc1 = (float)(1 - beta1^t), bc2s = (float)sqrt(1 - beta2^t).
 * grad itself is left unclipped.  lr arrives from the host: a schedule counts calls, Adam's t counts applied steps.
 *
 * ionode_train_refresh.  forward_image [ionode_mlp_packed_floats()] and grad_image [ionode_grad_image_floats()] of `weights`
 * from their int32 maps, one launch; grad_map and grad_image may both be NULL (a width the gradient path does not serve).  A
 * map entry s means: s > 0: weights[s - 1]; 0: padding, +0.0f; IONODE_TRAIN_MAP_NEG_ZERO: -0.0f (the fill of the 4-trajectory and
 * one-trajectory sections); s <= IONODE_TRAIN_MAP_PLUS_ZERO: weights[IONODE_TRAIN_MAP_PLUS_ZERO - s] + 0.0f (the scalar
 * section's hidden biases); an entry that names no weight gives +0.0f.  The grad map is ionode_image_refresh's.  The forward map
 * needs no packer of its own: ionode_mlp_pack of the values 1 .. n gives the indices and, in the sign bit of its zeros, the -0.0f
 * fill; ionode_mlp_pack of n times -0.0f gives +0.0f exactly where a weight passes through "+ 0.0f".  With such maps the images
 * equal ionode_mlp_pack / ionode_grad_pack of the same weights bit for bit, the sign of zeros included.
 *
 * The _host entry points run the same functions on host pointers with no HIP call, lane after lane in the written order; their
 * results equal the kernels' bit for bit.
 * Refusals, all before anything is touched, text in the gradient path's error string: IONODE_ERR_ARG for a NULL buffer, (mlp_layers,
 * mlp_width) that is no net or n not its state-dict size, no hidden layer (grad_norm), state_in == state_out, betas outside
 * [0, 1), eps <= 0, lr or max_norm not finite; IONODE_ERR_UNSUPPORTED for a width no image exists for.
 * ------------------------------------------------------------------------------------------------------------------- */
#define IONODE_TRAIN_STATE_DOUBLES 8
#define IONODE_TRAIN_STATE_T 0
#define IONODE_TRAIN_STATE_BETA1_T 1
#define IONODE_TRAIN_STATE_BETA2_T 2
#define IONODE_TRAIN_STATE_SKIPPED 3
#define IONODE_TRAIN_STATE_LOSS 4
#define IONODE_TRAIN_STATE_NORM 5
#define IONODE_TRAIN_STATE_SCALE 6
#define IONODE_TRAIN_STATE_APPLIED 7
#define IONODE_TRAIN_MAP_NEG_ZERO (-1)
#define IONODE_TRAIN_MAP_PLUS_ZERO (-2)

int32_t ionode_train_norm_partials(int32_t n);
int ionode_train_grad_norm(int32_t n, int32_t mlp_layers, int32_t mlp_width, const double *acc, const int32_t *padmap, float *grad,
                           double *norm_partials, void *stream);
int ionode_train_grad_norm_host(int32_t n, int32_t mlp_layers, int32_t mlp_width, const double *acc, const int32_t *padmap, float *grad,
                                double *norm_partials);
int ionode_train_apply(int32_t n, int32_t mlp_layers, int32_t mlp_width, const float *grad, const double *norm_partials, const double *loss,
                       const double *state_in, double *state_out, float *weights, float *exp_avg, float *exp_avg_sq, float lr, double beta1,
                       double beta2, float eps, double max_norm, void *stream);
int ionode_train_apply_host(int32_t n, int32_t mlp_layers, int32_t mlp_width, const float *grad, const double *norm_partials,
                            const double *loss, const double *state_in, double *state_out, float *weights, float *exp_avg,
                            float *exp_avg_sq, float lr, double beta1, double beta2, float eps, double max_norm);
int ionode_train_refresh(int32_t n, int32_t mlp_layers, int32_t mlp_width, const int32_t *forward_map, const int32_t *grad_map,
                         const float *weights, float *forward_image, float *grad_image, void *stream);
int ionode_train_refresh_host(int32_t n, int32_t mlp_layers, int32_t mlp_width, const int32_t *forward_map, const int32_t *grad_map,
                              const float *weights, float *forward_image, float *grad_image);

/* ---------------------------------------------------------------------------------------------------------------------
 * Posterior predictive bands: moments and exact quantiles of the current ACROSS parameter draws (new symbols, ABI stays 10).
 * After a posterior run (the three samplers above) a user wants, per protocol p and output sample k, the mean, the spread and a
 * credible band of i(t_k) over the S draws, and with sigma the prediction band that includes the observation noise.  The traces
 * of all draws would be S P Nt doubles; here they go by in chunks and only [P][Nt] moments and, for quantiles, the column store
 * cols [P][Nt][S_cap] stay.
 *
 * ionode_predictive_accumulate folds one chunk.  trace [n_draw P][Nt] fp64, candidate-major (row = c P + p, c the draw within
 * the chunk; the layout of the population functions' trial tensors), status [n_draw P] int32, sigma [>= draw_base + n_draw] fp64
 * indexed by draw_base + c, or NULL: d->sigma for every draw.  State, carried from chunk to chunk:
 * mean, m2, min, max [P][Nt] fp64 (fresh: 0, 0, +inf, -inf), count [P] int64 (fresh: 0), cols or NULL (no quantiles wanted).
 * Element (p, k) walks c = 0 .. n_draw - 1 in that order; a row with status != 0 is skipped (count[p] does not advance, its
 * slot cols[p][k][draw_base + c] is +inf); otherwise, with x = trace[c P + p][k] -- plus sigma z under d->noise, z the AS241
 * normal deviate of the first uniform of the Philox counter (draw_offset + draw_base + c, p, k, IONODE_PREDICTIVE_TAG) under d->seed --
 *   n <- n + 1;  delta = x - mean;  mean <- mean + delta / n;  m2 <- m2 + delta (x - mean);  min, max by < and >
 * and cols[p][k][draw_base + c] = x.  Every operation has one written order and the random numbers are a function of the
 * draw's index among all draws, so the state after all chunks does not depend on how the draws were cut into chunks, bit for bit.  The
 * sample variance is m2 / (count - 1).  count[p] is advanced by a second launch on the same stream.
 *
 * ionode_predictive_quantiles: quant [P][Q][Nt] from cols and count.  Every column is read as order-preserving 64-bit keys
 * (negative doubles: all bits flipped, the others: the sign bit set -- a total order, -0 before +0, +inf behind every finite
 * value), padded to a power of two with the key of all ones, and sorted; with m = count[p] (at most S_cap) the m smallest are
 * the surviving draws' values, and for each q: h = q (m - 1), lo = floor(h), g = h - lo, x_lo + g (x_hi - x_lo) with x_hi the
 * element min(lo + 1, m - 1).  m = 0: NaN.  A NaN among the surviving values has no place in that order and is not supported.
 *
 * ionode_predictive_plan: pure host code.  out[0] the quantile kernel's LDS bytes (8 * 2^L, 2^L >= max(s_cap, 2)), out[1] the
 * column store's bytes 8 n_prot n_out s_cap, out[2] L.  Refuses what ionode_predictive_quantiles refuses about the shape, and a
 * column store above budget_bytes (budget_bytes <= 0: no budget).
 *
 * Execution model: accumulate runs one 64-lane workgroup per (protocol, 64 consecutive samples), a lane per sample; the chunk's
 * rows are read along k (coalesced) in tiles of 32 draws and stored to cols along s through a padded LDS tile.  quantiles runs
 * one workgroup per column with the keys in LDS (128 KiB at the cap) and a bitonic network.  No atomics, no scratch.  The _host
 * entry points run the same element routines on host pointers with no HIP call; their results equal the kernels' bit for bit.
 * Refusals, all before anything is touched, text in the gradient path's error string: IONODE_ERR_ARG for a NULL descriptor or
 * buffer (sigma and cols may be NULL), n_prot (above 65 535 too), n_out or n_draw < 1, n_draw n_prot beyond 2^31 - 1 rows,
 * draw_base or draw_offset < 0, noise with neither a sigma array nor a finite d->sigma >= 0, with cols: s_cap < 1 or draw_base + n_draw >
 * s_cap; for the quantiles: n_q outside 1 .. IONODE_PREDICTIVE_MAX_Q, a q outside [0, 1] (or NaN), n_prot n_out beyond
 * 2^31 - 1 columns; IONODE_ERR_UNSUPPORTED for s_cap above IONODE_PREDICTIVE_MAX_DRAWS (the message names max_draws, the
 * argument of predictive.draws that thins a pool to fit) and for a column store above the budget.
 * ------------------------------------------------------------------------------------------------------------------- */
#define IONODE_PREDICTIVE_MAX_DRAWS 16384
#define IONODE_PREDICTIVE_MAX_Q 16
#define IONODE_PREDICTIVE_TAG 0x70720000u

typedef struct ionode_predictive_desc {
  int32_t n_prot;      /* P */
  int32_t n_out;       /* Nt */
  int32_t n_draw;      /* draws of this chunk: trace has n_draw * n_prot rows */
  int32_t s_cap;       /* draws the column store holds per (p, k); ignored without cols */
  int32_t draw_base;   /* index of the chunk's first draw among the caller's draws: its slot in cols and in the sigma array */
  int32_t draw_offset; /* index of the caller's first draw among ALL draws of the run (sharding): the generator sees draw_offset + draw_base + c */
  int32_t noise;       /* 1: accumulate and store i + sigma z */
  int32_t reserved;    /* 0 */
  int64_t seed;
  double sigma;        /* the one noise level, used when the sigma array is NULL */
} ionode_predictive_desc;

int ionode_predictive_plan(int32_t n_prot, int32_t n_out, int32_t s_cap, int64_t budget_bytes, int64_t out[3]);
int ionode_predictive_accumulate(const ionode_predictive_desc *d, const double *trace, const int32_t *status, const double *sigma,
                                 double *mean, double *m2, double *min, double *max, int64_t *count, double *cols, void *stream);
int ionode_predictive_accumulate_host(const ionode_predictive_desc *d, const double *trace, const int32_t *status, const double *sigma,
                                      double *mean, double *m2, double *min, double *max, int64_t *count, double *cols);
int ionode_predictive_quantiles(int32_t n_prot, int32_t n_out, int32_t s_cap, int32_t n_q, const double *q, const int64_t *count,
                                const double *cols, double *quant, void *stream);
int ionode_predictive_quantiles_host(int32_t n_prot, int32_t n_out, int32_t s_cap, int32_t n_q, const double *q, const int64_t *count,
                                     const double *cols, double *quant);

#ifdef __cplusplus
}
#endif
#endif /* IONODE_H */
