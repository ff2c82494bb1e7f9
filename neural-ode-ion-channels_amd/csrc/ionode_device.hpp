// ionode_device.hpp -- gfx950 (CDNA4, MI355X) device code of the batched dopri5 integrator.
//
// Execution model (DESIGN.md "Kernels"):
//   * A *tile* of trajectories advances in lock-step over step ATTEMPTS (every attempt costs the
//     same six RHS evaluations whether it is accepted or not), each trajectory with its own
//     t, dt and accept/reject decision.  Closed-form models: 64 trajectories per wavefront, one
//     per lane.  MLP models (NN-f / NN-d): 16 trajectories per tile, lane = 16*q + j holds
//     trajectory j (replicated over q = 0..3 and over the G wavefronts of the workgroup), which
//     is exactly the B-operand / accumulator column layout of v_mfma_f32_16x16x4_f32.
//   * The stage MLP of the tile is a chain of [NP x NP] x [NP x 16] products on the fp32 MFMA
//     (bit-for-bit an fmaf chain, i.e. the reference's fp32 arithmetic; same rate as the fp32 VALU
//     but one VGPR per operand and no broadcast traffic).  Accumulator tiles are handed to the
//     next layer as B operands without any transpose by permuting the contraction index:
//     register r of lane-group q of tile kt is k = 16*kt + 4*q + r.  Weights stream from L2 in
//     that fragment order (host-packed, 1 KiB per wave-load); activations are exchanged between
//     the G wavefronts through LDS (double-buffered, one barrier per layer).
//   * Dense output is emitted cooperatively: for every trajectory whose step was accepted, the
//     wavefront evaluates the 4th-order interpolant at 64 consecutive output times at once and
//     stores them coalesced (D*sizeof(S) bytes per lane).
//
// Arithmetic follows torchdiffeq 0.2.1's dopri5 operation by operation in the
// dtype torch would use; this translation unit is compiled with -ffp-contract=off so every a*b+c in
// the source is two IEEE operations, and the only fused operations are the explicit fmaf()/MFMA
// chains of the MLP.  Reference RHS definitions: train-s1.py:161-177 (HH), train-d1.py:165-187
// (6-state), train-s1.py:231-247 (NN-f), train-d2.py:247-272 (NN-d); protocol rule train-s1.py:218-237.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "../../include/ionode.h"
#include "ionode_form.hpp"
#include "ionode_kargs.hpp"   // KArgs, protocol_index / protocol_from / protocol_v
#include "ionode_math.hpp"
#include "ionode_interp.hpp"         // the dense-output interpolant and the observation model: the one definition
#include "ionode_dense_expand.hpp"   // DenseRecord: what a deferring tile writes per accepted step

namespace ionode {

// LDS layout of the lane-wise kernels (one trajectory per lane: closed-form models and the N <= 16 nets at 64 per wavefront),
// behind the MlpTile region when there is one.  Shared by the kernel and the host-side plan (ionode_capi.hip).
//   rows   [64][ROWB]  a lane's interpolant: {t0, step length} {1/step, 8 spare bytes} {5 x D fp64 coefficients}
//   aux    the fused objective's partial sums [64][8] fp64 (general and table variants; the lean variants sum no objective)
//   owp    [64] i32    the lane's protocol index
//   trl    [64] i32    the lane's trajectory index
//   clist  [512] u16   the attempt's dense-output WORK LIST: one entry per 8-sample chunk {lane, 8 * chunk number}
// gfx950 allocates LDS in 1280-byte granules; the lean 2-state kernels (<= 128 registers) want 16 wavefronts per compute unit:
// <= 10 240 bytes, the others 12: <= 12 800.
struct LwLds {
  // (D, tail): model states, KernelForm::lds_key (0 general, 1 lean, 2 table).  Row stride InterpRow<D>::BYTES = 112 / 272 bytes:
  // consecutive rows start on different LDS banks (128-byte rows put every row on the same banks: measured 30 % of the LDS
  // cycles in bank conflicts).
  static __host__ __device__ constexpr int rowb(int D) { return interp_row_doubles(D) * 8; }
  static __host__ __device__ constexpr int aux_off(int D) { return 64 * rowb(D); }
  static __host__ __device__ constexpr int aux_bytes(int tail) { return (tail == 1 && IONODE_LEAN) ? 0 : 64 * 64; }
  static __host__ __device__ constexpr int owp_off(int D, int tail) { return aux_off(D) + aux_bytes(tail); }
  static __host__ __device__ constexpr int trl_off(int D, int tail) { return owp_off(D, tail) + 256; }
  static __host__ __device__ constexpr int clist_off(int D, int tail) { return trl_off(D, tail) + 256; }
  static __host__ __device__ constexpr int bytes(int D, int tail) { return clist_off(D, tail) + 1024; }
};
static_assert(LwLds::bytes(2, 1) <= 10240 && LwLds::bytes(2, 0) <= 12800 && LwLds::bytes(2, 2) <= 12800, "2-state kernels: 16 / 12 wavefronts per compute unit");

}  // namespace ionode

// the nets and the right-hand sides (they take KArgs)
#include "ionode_mlp_tile.hpp"
#include "ionode_mlp_tile4.hpp"
#include "ionode_mlp_row1.hpp"
#include "ionode_mlp_lane.hpp"
#include "ionode_mlp_gen.hpp"
#include "ionode_rhs.hpp"

namespace ionode {

template <typename S, int D> __device__ __forceinline__ void store_state(S *dst, const S *v) {
  if constexpr (D == 2 && sizeof(S) == 8) {
    *reinterpret_cast<double2 *>(dst) = make_double2(v[0], v[1]);
  } else if constexpr (D == 2 && sizeof(S) == 4) {
    *reinterpret_cast<float2 *>(dst) = make_float2(v[0], v[1]);
  } else if constexpr (sizeof(S) == 8) {
#pragma unroll
    for (int d = 0; d < D; d += 2) *reinterpret_cast<double2 *>(dst + d) = make_double2(v[d], v[d + 1]);
  } else {
#pragma unroll
    for (int d = 0; d < D; d += 2) *reinterpret_cast<float2 *>(dst + d) = make_float2(v[d], v[d + 1]);
  }
}

// ---------------------------------------------------------------------------------------------
// The integrator.  One workgroup = one tile of TPW trajectories (G wavefronts for MLP models).
// ---------------------------------------------------------------------------------------------
// Lane-wise kernels (closed-form models, N <= 16 nets at 64 per wavefront): a tile is ONE wavefront, but a workgroup carries FOUR independent
// tiles (IONODE_LW_TILES_PER_WG), one per SIMD of a compute unit, each with its own LDS region and no barrier between them.  The
// hardware hands out whole workgroups, so the plan can cap the wavefronts per SIMD of a small launch through the workgroup's LDS
// reservation (ionode_capi.hip even_placement): single-wavefront workgroups of a launch that does not fill the chip get stacked three
// deep on some SIMDs while others idle (6-state, 65 536 trajectories: 24.2 ms stacked, 20.0 ms at one per SIMD).
// The seven template parameters are the variant's ENCODING (and its name); what they mean is decoded by KernelForm (ionode_form.hpp) alone.
template <int MODEL, typename S, int G, int RT, int NT, int PD, int TAIL>
__global__ void __launch_bounds__((KernelForm<MODEL, G, RT, NT, PD, TAIL>::block_threads), (KernelForm<MODEL, G, RT, NT, PD, TAIL>::waves_per_simd)) ionode_dopri5_kernel(const KArgs a_in) {
  using MT = ModelTraits<MODEL>;
  using F = KernelForm<MODEL, G, RT, NT, PD, TAIL>;
  // Per-variant CONTRACTS (ionode_capi.hip make_plan selects a variant only when they hold).  What a variant is never asked to do is
  // cleared in its private copy of the arguments: the branches fold away at compile time, and with them their code, their registers
  // and the scalars (pointers, caps) that would otherwise stay live through the attempt loop -- in SGPRs that spill into VGPR lanes.
  //   Lean::States (a lane-wise kernel): uniform protocol grid, VERIFIED uniform output grid, states only (no current trace, no
  //                fused objective), no step log, no checkpoints
  //   Lean::Table (a closed-form kernel): uniform protocol grid, no step log, no checkpoints
  constexpr bool LEAN = IONODE_LEAN && F::lean == Lean::States;
  constexpr bool LEANT = IONODE_LEAN && F::lean == Lean::Table;
  //   Lean::Tile (an MLP tile kernel): uniform protocol grid, VERIFIED uniform output grid, no step log, no checkpoints (states,
  //                current trace and fused objective stay run-time choices)
  constexpr bool LEANM = IONODE_LEAN && F::lean == Lean::Tile;
  KArgs a = a_in;
  if constexpr (LEANM) a.te_exact = 1;
  if constexpr (LEAN || LEANT || LEANM) { a.prot_t = nullptr; a.step_log = nullptr; a.step_log_cap = 0; a.ckpt = nullptr; a.ckpt_cap = 0; }
  if constexpr (LEAN) { a.i_out = nullptr; a.sse_out = nullptr; a.sse_ref = nullptr; a.v_tab = nullptr; a.te_exact = 1; }
#ifdef IONODE_STAMPS
  a.step_log = a_in.step_log; a.step_log_cap = a_in.step_log_cap;   // (the diagnostic build reports its stamps through the step log)
#endif
  using R = Real<S>;
  constexpr int D = MT::D, NPAR = MT::NPAR;
  // trajectories per wavefront: 16 for MLP tiles (MFMA column count); closed-form kernels: 64 (one per lane), or 16 (lanes
  // replicated 4x) for small batches, where 4x more wavefronts matter more than lane efficiency.
  // N <= 16 nets also at 64 per wavefront (MlpTile::eval_tiny64).  Such a kernel is "lane-wise" (LW) like the closed-form
  // ones -- one trajectory per lane -- and shares their dense-output machinery: interpolant rows in LDS (behind the MlpTile
  // region), arithmetic output times, carried stage voltages, work-list emission.
  constexpr bool T64 = F::t64, LW = F::lane_wise;
  // MLP tile kernels with two 16-trajectory column sets per workgroup (MlpTile::NSETS): wavefronts [0, WPS) integrate set 0,
  // [WPS, 2 WPS) set 1.  TPW = trajectories of the tile (4-trajectory tile: lane = 4 b + j holds trajectory j; one-trajectory
  // tile: every lane holds the trajectory), LPS = lanes of a wavefront that hold distinct trajectories.
  constexpr int NSETS = F::nsets, WPS = G / NSETS;
  constexpr int TPW = F::traj_per_tile, LPS = F::lanes_per_set;

  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

  const int lane = threadIdx.x & 63;
  const int wgw = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // wavefront inside the workgroup (wave-uniform: keeps tile guards scalar)
  const int wave = LW ? 0 : wgw;                                       // wavefront inside the TILE (lane-wise kernels: a tile is one wavefront)
  // lane-wise kernels: four tiles per workgroup.  Workgroups go round-robin over the 8 XCDs; tile t keeps landing on XCD t % 8 (the
  // protocol-major launch order deals the protocols out per XCD on that assumption): workgroup b, wavefront w -> tile (b % 8) + 8 (4 (b / 8) + w)
  const int tile = LW ? (int)((blockIdx.x & 7u) + 8u * ((blockIdx.x >> 3) * (unsigned)IONODE_LW_TILES_PER_WG + (unsigned)wgw)) : (int)blockIdx.x;
  unsigned char *const smem_t = LW ? smem + (size_t)wgw * (size_t)a.lw_bytes : smem;
  if constexpr (LW) {
    // the grid is rounded up to whole workgroups on every XCD: a tile past the batch leaves at once (it has no trajectory, and with
    // several weight images no image: its index would point past the caller's array).  No barrier joins the tiles of a lane-wise
    // workgroup after this point except MlpTile::init's, which the hardware completes without the wavefronts that have ended.
    if (tile * TPW >= a_in.B) return;
  }
  const int j = lane % LPS;
  const int cset = (NSETS > 1) ? wave / WPS : 0, wis = wave % WPS;  // column set of this wavefront, wavefront index inside the set
  const bool primary = (lane < LPS) && (wis == 0);  // the replica that writes per-trajectory scalars
  const int slot_raw = tile * TPW + cset * LPS + j;   // launch slot; the trajectory it integrates: a.order[slot] (or slot)
  const bool valid = slot_raw < a.B;
  const int slot_c = valid ? slot_raw : a.B - 1;
  const int traj = a.order ? a.order[slot_c] : slot_c;
  const int traj_raw = valid ? traj : a.B;   // (== 0 only for the lane that owns trajectory 0: the step log)

  using MlpT = typename F::Mlp;   // the variant's net (closed-form models: the empty NoMlp)
  MlpT mlp;
  if constexpr (MT::MLP) mlp.init(a, smem_t, wave, lane, tile * TPW);
  // lane-wise kernels: interpolant rows + tail buffers; behind the MlpTile region when there is one
  size_t lw_off = 0;
  if constexpr (T64) lw_off = (MlpT::lds_bytes(a.L) + 15) & ~(size_t)15;
  unsigned char *const lsm = smem_t + lw_off;
  STAMP_DECL
#ifdef IONODE_STAMPS
  [[maybe_unused]] const unsigned long long wall0_ = wall_clock64();
  if constexpr (MT::MLP) mlp.sp = &stamps_;
#endif

  double p[NPAR];   // (not const: made opaque once per attempt in the lane-wise kernels, below)
#pragma unroll
  for (int i = 0; i < NPAR; ++i) p[i] = a.params[(size_t)traj * a.n_params + i];
  const int pidx = a.prot_of_traj ? a.prot_of_traj[traj] : (traj % a.P);
  const double *__restrict__ pv = a.prot_v + (size_t)pidx * a.Np;

  const S rtol = (S)a.rtol, atol = (S)a.atol;
  S *__restrict__ yout = reinterpret_cast<S *>(a.y_out) + (size_t)traj * a.Nt * D;
  double *__restrict__ iout = a.i_out ? a.i_out + (size_t)traj * a.Nt : nullptr;
  const int Nt = a.Nt;

  S y[D], f[D];
#pragma unroll
  for (int d = 0; d < D; ++d) y[d] = reinterpret_cast<const S *>(a.y0)[(size_t)traj * D + d];

  double t = a.t_eval[0];
  {
    double v0;
    const bool in0 = protocol_v(a, pv, (double)(S)t, v0);
    rhs<MODEL, S, T64>(a, p, v0, in0, y, f, mlp);  // f0 = func(t[0], y0)
  }

  // _select_initial_step (order argument 4), all in the state dtype
  double dt;
  {
    const S t0s = (S)t;
    S scale[D], tmp[D], y1[D], f1[D];
#pragma unroll
    for (int d = 0; d < D; ++d) scale[d] = atol + abs_(y[d]) * rtol;
#pragma unroll
    for (int d = 0; d < D; ++d) tmp[d] = y[d] / scale[d];
    const S d0 = rms_norm<S, D>(tmp);
#pragma unroll
    for (int d = 0; d < D; ++d) tmp[d] = f[d] / scale[d];
    const S d1 = rms_norm<S, D>(tmp);
    S h0;
    if (d0 < (S)1e-5 || d1 < (S)1e-5) h0 = (S)1e-6;
    else h0 = (S)0.01 * d0 / d1;
#pragma unroll
    for (int d = 0; d < D; ++d) y1[d] = y[d] + h0 * f[d];
    {
      double v1;
      const bool in1 = protocol_v(a, pv, (double)(t0s + h0), v1);
      rhs<MODEL, S, T64>(a, p, v1, in1, y1, f1, mlp);
    }
#pragma unroll
    for (int d = 0; d < D; ++d) tmp[d] = (f1[d] - f[d]) / scale[d];
    const S d2 = rms_norm<S, D>(tmp) / h0;
    S h1;
    if (d1 <= (S)1e-15 && d2 <= (S)1e-15) {
      const S c = h0 * (S)1e-3;
      h1 = (S)1e-6 > c ? (S)1e-6 : c;
    } else {
      h1 = (S)det_root5((double)((S)0.01 / (d1 > d2 ? d1 : d2)));
    }
    const S h = ((S)100 * h0 < h1) ? (S)100 * h0 : h1;
    dt = (double)h;
    if (dt > a.dt_max) dt = a.dt_max;
  }

  // ---- lane-wise kernels: where the dense output goes through ----
  // gfx9 counts loads and stores in ONE in-order counter (vmcnt): a load issued behind a store cannot be consumed before that
  // store has been acknowledged by L2 -- for a store to a cold line that is an HBM round trip.  The round-1 emission loop
  // loaded t_eval once per 64-sample chunk behind the previous chunk's store, and the stage voltages of the next attempt
  // behind all of them: waves sat in s_waitcnt 82 % of the time (SQ_WAIT_ANY, profiles/r02_closed_form.md).  On a verified
  // uniform output grid (te_exact) output times are formed arithmetically and the next attempt's protocol lookups are issued
  // and consumed BEFORE the emission, so the emission is LDS reads + VALU + stores only and nothing waits on a store.
  // (Rounds 2-3 also held samples back in LDS tail buffers until a whole 64-byte sector could be written; L2 merges the partial
  // sectors of neighbouring steps on its own, and without the tail logic the lean 2-state kernel fits 128 registers and
  // 8.5 KiB of LDS -- four wavefronts per SIMD instead of three: 35.6 -> 30.5 ms at 393 216 x 20 001, profiles/r04_emission_ab.md.)
  constexpr bool CF2 = LW && D == 2;
  constexpr int LT = F::lds_key;   // the LDS layout's variant key
  constexpr int ROWB = LwLds::rowb(D);
  // table variant of a closed-form kernel: the current / objective epilogue reads V(t_k) from the pre-pass table a.v_tab (selected
  // by the dispatcher when ionode_desc.v_at_outputs is given); a compile-time variant so that neither variant carries the
  // other's code and registers
  constexpr bool VTAB = F::lean == Lean::Table;
  double *const ssep = reinterpret_cast<double *>(lsm + LwLds::aux_off(D));  // [64][8] partial sums of the fused objective (not in the lean variants)
  if constexpr (LW) {
    if (a.sse_out != nullptr) {
#pragma unroll
      for (int m = 0; m < 8; ++m) ssep[lane * 8 + m] = 0.0;
    }
  }
  // owp: protocol index of every lane's trajectory, trl: its trajectory index (read per lane group by the emission).  clist: the work list.
  int *const owp = reinterpret_cast<int *>(lsm + LwLds::owp_off(D, LT));
  int *const trl = reinterpret_cast<int *>(lsm + LwLds::trl_off(D, LT));
  unsigned short *const clist = reinterpret_cast<unsigned short *>(lsm + LwLds::clist_off(D, LT));
  if constexpr (LW) {
    if (lane < LPS) trl[lane] = traj, owp[lane] = pidx;
  }
  auto te_at = [&](int idx) -> double { return a.te_t0 + (double)idx * a.te_dt; };

  // solution[0] = y0
  double sse = 0.0;  // fused objective: this lane's trajectory (accumulated by the owner wavefront's replica lanes)
  if (valid && primary) {
    if (a.y_out) store_state<S, D>(yout, y);
    if (iout) {
      double v0;
      protocol_v(a, pv, t, v0);
      iout[0] = obs_current<S, D>(a, y, v0);
    }
  }
  if (a.sse_out != nullptr && valid) {
    double v0;
    protocol_v(a, pv, t, v0);
    const double r0 = obs_current<S, D>(a, y, v0) - a.sse_ref[(size_t)pidx * Nt];
    sse = residual_term(r0, F::objective_kinds ? a.obj_abs : 0);
  }

  int oi = 1;  // next output index
  int nacc = 0, nrej = 0;
  int since = 0;  // attempts since the last emitted output (torchdiffeq counts max_num_steps per _advance call)
  [[maybe_unused]] int nrec = 0;  // (KernelForm::defer) dense-output records this trajectory has written
  int status = IONODE_STATUS_OK;
  bool active = valid && Nt > 1;
  const S nan_s = (S)__builtin_nan("");

  // stage voltages of the coming attempt: pure functions of (t, dt).  Closed-form kernels carry them across iterations: they
  // are looked up for the NEXT attempt right after the controller, ahead of the emission's stores (see "where the dense output goes through" above)
  double vst[5];
  bool inst[5];
  auto lookup_stages = [&](double tt, double dd) {
    const S tts = (S)tt, dds = (S)dd, tt1s = (S)(tt + dd);
    // batched lookups: the MLP tiles and the closed-form kernels except the 2-state table variant (173 instead of 151 registers = two
    // wavefronts per SIMD instead of three) and the N <= 16 kernels (DESIGN_HISTORY.md "retired switches")
    if (((MT::MLP && G > 1) || (!MT::MLP && (D > 2 || !VTAB))) && a.prot_t == nullptr) {
      // uniform protocol grid: five indices, five 16-byte loads back to back, then the interpolations -- ONE memory round
      // trip per attempt (protocol_v() per stage time waited for each pair of samples in turn: 5 dependent round trips,
      // ~7 k cycles of the s00 attempt)
      double tq[5], lo[5], hi[5];
      int ix[5];
#pragma unroll
      for (int i = 0; i < 5; ++i) {
        tq[i] = (double)((i >= 4) ? R::prev_(tt1s) : tts + (S)kAlpha[i] * dds);
        inst[i] = protocol_index(a, tq[i], ix[i]);
      }
#pragma unroll
      for (int i = 0; i < 5; ++i) { lo[i] = pv[ix[i] - 1]; hi[i] = pv[ix[i]]; }
#pragma unroll
      for (int i = 0; i < 5; ++i) vst[i] = inst[i] ? protocol_from(a, lo[i], hi[i], ix[i], tq[i]) : a.v_oob;
      return;
    }
#pragma unroll
    for (int i = 0; i < 5; ++i) {
      const S ti = (i >= 4) ? R::prev_(tt1s) : tts + (S)kAlpha[i] * dds;  // alpha == 1: Perturb.PREV (stages 4 and 5)
      inst[i] = protocol_v(a, pv, (double)ti, vst[i]);
    }
  };
  // carried by the 2-state lane-wise kernels, the lean 6-state variant (224 registers, headroom for five more voltages) and the N <= 16
  // kernel at 16 trajectories per wavefront; not by the MLP tiles (DESIGN_HISTORY.md "retired switches")
  constexpr bool CARRY_V = (LW && D == 2) || (LW && D > 2 && LEAN) || (MT::MLP && G == 1);
  if constexpr (CARRY_V) lookup_stages(t, dt);

  // Lean N = 200 16-tile (round 6): once <= 4 of the tile's trajectories are live, the attempts run on the 4-trajectory net
  // (MlpShrink4) -- a second attempt loop with the same body, so that the two nets' registers are never live together
  constexpr bool SHRINK = F::shrink;
#ifdef IONODE_STAMPS
  unsigned long long att_cyc[2] = {0, 0}, att_n[2] = {0, 0};   // per net (0: the tile's own, 1: MlpShrink4): cycles of the attempts, attempts
#endif

  // live slots of a 16-tile: every wavefront integrates all 16 (lanes 16 q + j replicate slot j), so the mask is the same everywhere
  auto live_slots = [&]() { return (unsigned)__ballot(active) & 0xffffu; };
  bool more = true;   // (SHRINK) trajectories left when the first loop ends
  if (!SHRINK || !a.tile_shrink || __builtin_popcount(live_slots()) > 4) {   // (a ragged batch end with <= 4 valid slots: straight to the 4-tile)
    more = false;
    for (;;) {
#define IONODE_NET mlp
#include "ionode_attempt_body.hpp"
#undef IONODE_NET
      if constexpr (SHRINK) {
        if (a.tile_shrink && __builtin_popcount(live_slots()) <= 4) { more = true; break; }
      }
    }
  }
  if constexpr (SHRINK) {
    const unsigned live = live_slots();
    if (more && live != 0u) {
      // the asm stream leaves the next evaluation's weight loads in flight (into a[0:91]): they land before the registers and the LDS
      // region are handed to the 4-tile
      asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
      __syncthreads();
      MlpShrink4 net4;
      net4.init(a, smem_t, wave, lane, tile * TPW, live);
#ifdef IONODE_STAMPS
      net4.t4.sp = &stamps_;
#endif
      for (;;) {
#define IONODE_NET net4
#include "ionode_attempt_body.hpp"
#undef IONODE_NET
      }
    }
  }

#ifdef IONODE_STAMPS
  STAMP(stamps_, 0);
  if (blockIdx.x == 0 && threadIdx.x == 0 && a.step_log != nullptr && a.step_log_cap >= 4)
    for (int i_ = 0; i_ < 16; ++i_) a.step_log[i_] = (double)stamps_.acc[i_];
  // tile shrink (round 6, tools/tile_shrink_stamps.py): wavefront 0 of tile 0 -- cycles and count of the attempts on the tile's own net and
  // on MlpShrink4 at step_log[32..35]; every tile's attempts on MlpShrink4 at step_log[64 + tile] when the log has room
  if (threadIdx.x == 0 && a.step_log != nullptr) {
    if (blockIdx.x == 0 && a.step_log_cap >= 9) {
      a.step_log[32] = (double)att_cyc[0]; a.step_log[33] = (double)att_n[0];
      a.step_log[34] = (double)att_cyc[1]; a.step_log[35] = (double)att_n[1];
    }
    if (4 * a.step_log_cap >= 64 + (int64_t)gridDim.x) a.step_log[64 + blockIdx.x] = (double)att_n[1];
  }
#ifdef IONODE_ASM_STAMPS  // per-position cycle sums of the asm stream (tools/gen_mlp_asm.py --stamps): lanes of a[92]
  if constexpr (MT::MLP && G == 4 && NT == 13) {
    unsigned sv_;
    asm volatile("v_accvgpr_read_b32 %0, a92" : "=v"(sv_));
    if (blockIdx.x == 0 && threadIdx.x < 16 && a.step_log != nullptr && a.step_log_cap >= 8) a.step_log[16 + threadIdx.x] = (double)sv_;
  }
#endif
#endif
  if constexpr (LW) {
    if (a.sse_out != nullptr) {
#pragma unroll
      for (int m = 0; m < 8; ++m) sse += ssep[j * 8 + m];
    }
  }
  if (a.sse_out != nullptr && valid && lane < LPS && (WPS == 1 || (lane % WPS) == wis))
    a.sse_out[traj] = (status == IONODE_STATUS_OK) ? sse : __builtin_inf();  // the reference's time-limit rule: inf (train-d0.py:430-431)
  if (valid && primary) {
    a.status[traj] = status;
    if (a.stats) {
      int64_t *st = a.stats + (size_t)traj * 4;
      st[0] = nacc;
      st[1] = nrej;
      st[2] = 2 + 6 * ((int64_t)nacc + nrej);
      st[3] = status;
    }
  }
  // ---- deferred dense output: the tile's record counts, and the TAIL.  The launch lasts as long as its slowest tile (one tile per
  // compute unit at the headline shape), so a tile that ends early expands its own records here, on a compute unit that would idle until
  // the launch ends, and only the late tiles' records are left for ionode_dense_expand_kernel.  Early is decided by ONE atomic add on a
  // finish counter: the tile reads its rank once and nothing ever waits on the counter.
  if constexpr (F::defer) {
    if (a.defer_rec != nullptr) {
      int left = nrec;
      if (a.defer_tail_rank > 0) {
        // the asm stream leaves the next evaluation's weight loads in flight (into a[0:91]), and the workgroup's LDS is dead from here on
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        __syncthreads();
        int *const rank_lds = reinterpret_cast<int *>(smem);
        if (threadIdx.x == 0) *rank_lds = atomicAdd(a.defer_tail, 1);
        __syncthreads();
        const int rank = __builtin_amdgcn_readfirstlane(*rank_lds);
#ifdef IONODE_STAMPS
        const unsigned long long wall1_ = wall_clock64();
#endif
        if (rank < a.defer_tail_rank) {
          // records are written by lanes of all four wavefronts: every store acknowledged (above), visible device-wide, then the barrier
          __threadfence();
          __syncthreads();
          __threadfence();
#pragma unroll 1
          for (int jj = 0; jj < LPS; ++jj) {
            const int cj = __builtin_amdgcn_readlane(nrec, jj);   // (a slot past the batch, a NaN y0: no record)
            if (cj > 0) dense_expand_records<S, D, kExpandAheadTail>(a, __builtin_amdgcn_readlane(traj, jj), wave, cj, G, lane);
          }
          left = -(nrec + 1);
        }
#ifdef IONODE_STAMPS
        // per tile, 100 MHz wall clock (tools/defer_tail_stamps.py): start, end of the solve, end of the tail, behind the per-tile block
        if (threadIdx.x == 0 && a.step_log != nullptr && 4 * a.step_log_cap >= 64 + 4 * (int64_t)gridDim.x) {
          double *const w_ = a.step_log + 64 + gridDim.x + 3 * (size_t)blockIdx.x;
          asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // (the tail's stores acknowledged)
          w_[0] = (double)wall0_; w_[1] = (double)wall1_; w_[2] = (double)wall_clock64();
        }
#endif
      }
      if (valid && primary) a.defer_count[traj] = left;
    }
  }
}

}  // namespace ionode
