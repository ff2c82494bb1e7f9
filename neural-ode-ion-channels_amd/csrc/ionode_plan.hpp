// ionode_plan.hpp -- host only, included by ionode_capi.hip alone: the plan of one forward launch.  The dispatcher (which kernel
// variant, which geometry), the deferred dense output, the solve kernel's tail and the tile composition, all decided in ONE place,
// plan_launch(), from the descriptor, a Request (what the entry point received beyond it) and the development Switches.  The plan
// queries of include/ionode.h are projections of the LaunchPlan; the launch (ionode_capi.hip checked_solve) consumes the same struct.
#pragma once
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "ionode_compose.hpp"
#include "ionode_host.hpp"
#include "ionode_launch.hpp"

namespace {

// Dispatcher thresholds, in trajectories of one launch.
constexpr int kTile32From = 8192;    // N = 200: from here on 32-trajectory tiles (two 16-trajectory tiles per compute unit)
constexpr int kTile4Upto = 1024;     // N = 200: up to this many trajectories, 4 per tile = at most one tile per compute unit (16-tiles would use <= 64 of the 256 CUs)
constexpr int kTile1Upto = 256;      // N = 200: up to this many trajectories, ONE per tile (MlpRow1: a lane owns a row) = at most one tile per compute unit
constexpr int kTiny64From = 32769;   // N <= 16: one trajectory per lane.  Round 4, final build (per-lane packed net, even placement; 20 001 samples): 16 per wavefront 12.0-12.1 ms from 16 384 to 32 768 (two wavefronts per SIMD), 19.6 at 49 152, 23.1 at 65 536; 64 per wavefront 13.3-13.7 ms from 8 192 to 65 536
// closed-form models: 16 trajectories per wavefront (lanes replicated 4x, 4x the wavefronts) while the launch has fewer wavefronts than
// the chip has SIMDs to spread them over; measured crossovers (round 4, tools/gpu/r4_t4b.sh, 20 001 samples): 2-state 32 768: 6.3 ms at
// 16 per wavefront / 9.7 at 64, 65 536: 11.6 / 10.1; 6-state 16 384: 9.1 / 13.8, 32 768: 17.5 / 15.0
constexpr int kHh2LaneFrom = 49152;
constexpr int kMarkov6LaneFrom = 24576;

thread_local char g_err[256] = "";

void set_err(const char *fmt, const char *detail = "") { snprintf(g_err, sizeof g_err, fmt, detail); }

inline int np_of(int N) { return 16 * ((N + 15) / 16); }

// ---- the development switches (A/B runs and tests), read per plan: the forward path's only getenv ----
enum ComposeSource : int32_t { kComposeOff = 0, kComposePilot = 1, kComposeHint = 2, kComposeAuto = 3 };
enum class TailSwitch { Default, Off, All };
struct Switches {
  bool tile_shrink = true;                    // IONODE_TILE_SHRINK=0: the lean 16-tile never hands its tail to the 4-trajectory net
  bool defer_dense = true;                    // IONODE_DEFER_DENSE=0: nothing is deferred
  int64_t defer_cap = 0;                      // IONODE_DEFER_DENSE_CAP=n > 0: forces the record capacity
  TailSwitch tail = TailSwitch::Default;      // IONODE_DEFER_TAIL=0: no tile expands in the solve kernel, =all: every tile
  bool tail_rank_set = false;                 // IONODE_DEFER_TAIL_RANK=n: n tiles
  int64_t tail_rank = 0;
  ComposeSource compose = kComposeAuto;       // IONODE_COMPOSE=0|pilot|hint: where the composition's cost may come from
};
// a switch's text; nullptr -- the default -- when it is unset or empty
const char *switch_text(const char *name) {
  const char *s = getenv(name);
  return (s != nullptr && s[0] != '\0') ? s : nullptr;
}
Switches read_switches() {
  Switches s;
  if (const char *t = switch_text("IONODE_TILE_SHRINK")) s.tile_shrink = atoi(t) != 0;
  if (const char *t = switch_text("IONODE_DEFER_DENSE")) s.defer_dense = atoi(t) != 0;
  if (const char *t = switch_text("IONODE_DEFER_DENSE_CAP")) s.defer_cap = atoll(t);
  if (const char *t = switch_text("IONODE_DEFER_TAIL")) s.tail = strcmp(t, "all") == 0 ? TailSwitch::All : atoi(t) == 0 ? TailSwitch::Off : TailSwitch::Default;
  if (const char *t = switch_text("IONODE_DEFER_TAIL_RANK")) { s.tail_rank_set = true; s.tail_rank = atoll(t); }
  if (const char *t = switch_text("IONODE_COMPOSE"))
    s.compose = strcmp(t, "pilot") == 0 ? kComposePilot : strcmp(t, "hint") == 0 ? kComposeHint : atoi(t) == 0 ? kComposeOff : kComposeAuto;
  return s;
}

// ---- what an entry point received beyond the descriptor ----
struct Request {
  bool want_current = false;    // a current trace or the fused objective: the epilogue
  bool explicit_grid = false;   // prot_t given
  bool has_workspace = false;   // a record workspace given ...
  bool has_y_out = false;       // ... and states asked for: with a uniform protocol grid, the conditions of the deferred dense output
  int cost_source = 0;          // ionode_dopri5_composed's, 0 unless the launch is ordered
  int objective = IONODE_OBJECTIVE_SSE;
};
// The one place where "i_out or sse_out implies the epilogue" and "cost_source counts only with launch_order" are written.  The plan
// queries pass what include/ionode.h documents for them: uniform protocol grid, a workspace and y_out assumed.
Request request_of(const ionode_desc *d, bool i_out, bool prot_t = false, bool workspace = true, bool y_out = true, int cost_source = 0,
                   int objective = IONODE_OBJECTIVE_SSE) {
  return {i_out || (d && d->sse_out != nullptr), prot_t, workspace, y_out, (d && d->launch_order != nullptr) ? cost_source : 0, objective};
}

// ---- the dispatcher ----
struct Plan {
  const ionode::Variant *v = nullptr;
  unsigned grid = 0;
  unsigned block = 0;
  size_t lds = 0;
  size_t lw_bytes = 0;   // lane-wise kernels: LDS bytes of one wavefront's region (the workgroup reserves four)
  bool tile_shrink = false;   // lean N = 200 16-tile: the tail of a tile runs on the 4-trajectory net (KArgs::tile_shrink)
};

// Lane-wise kernels: four one-wavefront tiles per workgroup (ionode_form.hpp IONODE_LW_TILES_PER_WG), tile t on XCD t % 8.  The
// workgroup count is a multiple of 8 so that (workgroup, wavefront) -> tile is onto; empty tiles leave at once.
// EVEN PLACEMENT: the hardware places whole workgroups, and a four-wavefront workgroup occupies one slot on each SIMD of its compute
// unit -- so the workgroups that fit a CU are the wavefronts per SIMD.  A launch of fewer tiles than the kernel's natural residency
// reserves more LDS per workgroup (a multiple of the 1280-byte granule), capping the workgroups per CU at ceil(workgroups / CUs):
// without the cap the dispatcher stacks a small launch three deep on some SIMDs and leaves others idle.
void plan_lane_wise(Plan *pl, size_t tiles, size_t per_wave_bytes) {
  const size_t cap = 160 * 1024, gran = 1280, T = IONODE_LW_TILES_PER_WG;
  pl->lw_bytes = (per_wave_bytes + 15) & ~(size_t)15;
  pl->grid = (unsigned)(8 * ((tiles + 8 * T - 1) / (8 * T)));
  pl->block = (unsigned)(64 * T);
  size_t lds = T * pl->lw_bytes;
  // The padding assumes the 8-XCD round-robin of the whole chip (256 compute units): on a partitioned device (CPX / DPX) it is skipped;
  // without a device it is applied.  Read ONCE per process, unlike plan_compose's: the closed-form models' 6 ms calls come through
  // here, and a read per plan has not been measured on them.
  static const int ncu_dev = ionode::compute_units();
  const size_t ncu = 256;
  const size_t per_cu = (pl->grid + ncu - 1) / ncu;
  const size_t natural = cap / (((lds + gran - 1) / gran) * gran);
  if (ncu_dev == (int)ncu && per_cu >= 1 && per_cu < natural) {
    const size_t pad = (cap / per_cu) / gran * gran;
    if (pad > lds) lds = pad;
  }
  pl->lds = lds;
}

// Batch size from which the dispatcher takes the one-trajectory-per-lane (64 per wavefront) kernel of a model; 0: the model has none.
// Exported as ionode_lane_wise_from() so that host code (capi.py: protocol-major launch order) does not keep a copy of the numbers.
int lane_wise_from(int model, int mlp_width) {
  if (model == IONODE_MODEL_HH2) return kHh2LaneFrom;
  if (model == IONODE_MODEL_MARKOV6) return kMarkov6LaneFrom;
  if ((model == IONODE_MODEL_NNF || model == IONODE_MODEL_NND) && mlp_width >= 1 && mlp_width <= 16) return kTiny64From;
  return 0;
}

// The compiled variant with these decoded facts (ionode_launch.hpp Variant).  G == 0: any wavefront count.
const ionode::Variant *find_variant(int model, int f32, ionode::Net net, ionode::Lean lean, int traj_per_tile, int G, int NT) {
  using namespace ionode;
  typedef const Variant *(*TabFn)(int *);
  static const TabFn tabs[] = {variants_closed, variants_nnf_f64, variants_nnf_f32, variants_nnd_f64, variants_nnd_f32};
  for (TabFn tf : tabs) {
    int n = 0;
    const Variant *t = tf(&n);
    for (int i = 0; i < n; ++i)
      if (t[i].model == model && t[i].f32 == f32 && t[i].net == net && t[i].lean == lean && t[i].traj_per_tile == traj_per_tile &&
          (G == 0 || t[i].G == G) && t[i].NT == NT)
        return &t[i];
  }
  return nullptr;
}

// What the caller asks for beyond the descriptor's own fields, as the dispatcher reads it
struct Ask {
  bool want_current;    // a current trace or the fused objective
  bool explicit_grid;   // prot_t given
  bool has_step_log;
  bool abs_objective;   // the fused objective sums absolute residuals (ionode_dopri5_objective)
  bool tile_shrink;     // Switches::tile_shrink
};

// The specialised variants are compiled under a CONTRACT (ionode_form.hpp Lean): uniform protocol grid, no step log, no checkpoints --
// anything else takes the general variant.
bool no_side_outputs(const ionode_desc *d, const Ask &k) { return !k.explicit_grid && !k.has_step_log && !d->ckpt; }
bool has_grid_hint(const ionode_desc *d) { return d->t_eval_dt_hint > 0.0 && d->n_out > 1; }
bool has_exact_grid(const ionode_desc *d) { return d->t_eval_exact && has_grid_hint(d); }

int plan_closed(const ionode_desc *d, Plan *pl, const Ask &k, int D) {
  using ionode::Lean;
  // tile_waves = 64 / 16 forces the trajectories per wavefront
  const int tpw = (d->tile_waves == 64 || d->tile_waves == 16) ? d->tile_waves : (d->n_traj >= lane_wise_from(d->model, 0) ? 64 : 16);
  //   Table:  current trace / fused objective with the protocol-at-outputs table given (hint path)
  //   States: states only on a VERIFIED uniform output grid, no current trace / objective
  const Lean lean = !no_side_outputs(d, k)                                     ? Lean::General
                    : (k.want_current && d->v_at_outputs && has_grid_hint(d)) ? Lean::Table
                    : (has_exact_grid(d) && !k.want_current)                  ? Lean::States
                                                                              : Lean::General;
  // (Rounds 2-3 kept two builds of the 2-state kernels -- 2 and 3 wavefronts per SIMD -- and switched at 2048 wavefronts; since round 4
  // one build per variant: the lean one fits four per SIMD, the others three, without a spill: KernelForm::waves_per_simd.)
  // 6-state model: two wavefronts per SIMD (lean), otherwise one.
  pl->v = find_variant(d->model, d->state_f32 ? 1 : 0, ionode::Net::None, lean, tpw, 1, 0);
  if (!pl->v) { set_err("no kernel variant compiled for this descriptor"); return IONODE_ERR_UNSUPPORTED; }
  plan_lane_wise(pl, (size_t)((d->n_traj + tpw - 1) / tpw), (size_t)ionode::LwLds::bytes(D, pl->v->lds_key));
  return IONODE_OK;
}

int plan_mlp(const ionode_desc *d, Plan *pl, const Ask &k) {
  using ionode::Lean;
  using ionode::Net;
  if (d->mlp_width < 1 || d->mlp_layers < 0) { set_err("bad MLP shape"); return IONODE_ERR_ARG; }
  if (d->mlp_width <= 16 && d->mlp_layers > 10) { set_err("N <= 16 kernels keep at most 10 hidden layers resident"); return IONODE_ERR_UNSUPPORTED; }
  const int f32 = d->state_f32 ? 1 : 0, tw = d->tile_waves, L = d->mlp_layers;
  const int NP = np_of(d->mlp_width), NT = NP / 16;
  if (tw != 0 && tw != 1 && tw != 4 && !(tw == 64 && NT == 1) && !((tw == 8 || tw == 2 || tw == 16) && NT == 13)) {
    set_err("tile_waves must be 0, 1 or 4 for MLP models (64: the N <= 16 kernel at 64 trajectories per wavefront; 8 / 2 / 16: the N = 200 kernel with 32 / 4 / 1 trajectories per tile)");
    return IONODE_ERR_UNSUPPORTED;
  }
  // ---- 1. the net kind and the lean kind, from the descriptor ----
  auto images_fill = [&](int tile) { return d->traj_per_image <= 0 || d->traj_per_image % tile == 0; };
  const bool n200 = NT == 13 && L >= 1;   // the N = 200 tile forms need a hidden layer (asm stream / their own image sections)
  // N <= 16 (architectures s03-s05): from kTiny64From trajectories on, one trajectory per lane (64 per wavefront, four
  // MFMA column tiles per evaluation) instead of 16 per wavefront with the scalar integrator work replicated over 4 lane groups
  // (several weight images: the automatic choice takes the 64-per-wavefront kernel only when an image's trajectories fill whole
  // 64-lane tiles -- a population of nets padded to 16 / 32 / 48 trajectories per candidate stays on the 16-per-wavefront kernel;
  // an explicit tile_waves = 64 with such a population is still an argument error, below)
  const bool t64 = NT == 1 && (tw == 64 || (tw == 0 && d->n_traj >= kTiny64From && images_fill(64)));
  // N = 10 (architectures s03-s05) at one trajectory per lane: the per-lane vector-ALU net (MlpLane)
  const bool vnet = t64 && d->mlp_width == 10;
  // N = 200: from two 16-trajectory tiles per compute unit on, 32-trajectory tiles -- two column sets per weight fragment, the scalar
  // integrator work replicated twice instead of four times (tile_waves = 8 forces it, 4 forces the 16-tile).  Weight images must cover
  // whole 32-trajectory tiles.
  const bool t32 = !t64 && n200 && images_fill(32) && (tw == 8 || (tw == 0 && d->n_traj >= kTile32From));
  // N = 200, single calls and the smallest batches: ONE trajectory per tile (MlpRow1; tile_waves = 16 forces it, 2 / 4 / 8 exclude it)
  const bool t1 = !t64 && !t32 && n200 && L <= 15 && (tw == 16 || (tw == 0 && d->n_traj <= kTile1Upto));
  const bool t1deep = t1 && L > ionode::MlpRow1::max_layers();   // no room for LDS-resident steps: every step streamed
  // N = 200, small batches and single calls: 4 trajectories per tile (MlpTile4; tile_waves = 2 forces it, 4 / 8 exclude it)
  const bool t4 = !t64 && !t32 && !t1 && n200 && images_fill(4) && (tw == 2 || (tw == 0 && d->n_traj <= kTile4Upto));
  // lean contracts.  N <= 16 at one per lane: as for the closed-form kernels (verified uniform output grid, no current / objective);
  // tuned tiles with a hidden layer and the run-time-width tile: verified uniform output grid
  const bool lean_tile = L >= 1 && no_side_outputs(d, k) && has_exact_grid(d);
  const bool lean_t64 = t64 && has_exact_grid(d) && !k.want_current && no_side_outputs(d, k);
  const Net net = vnet ? Net::Lane : t1 ? (t1deep ? Net::Row1Deep : Net::Row1) : t4 ? Net::Tile4 : Net::Tile;
  const int tpt = t64 ? 64 : t32 ? 32 : t1 ? 1 : t4 ? 4 : 16;
  // (the lean N = 200 16-tile knows the squares alone, KernelForm::objective_kinds: absolute residuals take its general variant)
  const bool squares_only = net == Net::Tile && NT == 13 && tpt == 16;
  const bool lean_tuned = !t64 && (NT == 13 || NT == 7 || NT == 32) && lean_tile && !(k.abs_objective && squares_only);
  // ---- 2. the variant ----
  const int G = t64 ? 1 : ((tw == 8 || tw == 2 || tw == 16) ? 4 : tw);
  pl->v = find_variant(d->model, f32, net, lean_t64 ? Lean::States : (lean_tuned ? Lean::Tile : Lean::General), tpt, G, NT);
  // any other width up to 512 (table-s1.py:145-153 builds nets of any (n_layers, n_nodes)): the run-time-width tile (MlpGen)
  if (!pl->v && NT >= 2 && NT <= ionode::MlpGen::NT_MAX && (tw == 0 || tw == 4)) {
    pl->v = find_variant(d->model, f32, Net::Gen, lean_tile ? Lean::Tile : Lean::General, 16, 4, 0);
    if (pl->v && pl->v->lds_bytes(L, NT) > 160 * 1024) {
      set_err("this (layers, width) needs more than 160 KB of LDS for its biases and activations");
      return IONODE_ERR_UNSUPPORTED;
    }
  }
  if (!pl->v) {
    set_err("MLP width outside the compiled kernel variants: 1 <= N <= 512 (tuned tiles for N = 10, 100, 200, 500 -- architectures "
            "s00-s11 -- and the run-time-width tile for every other N; tile_waves must be 0 or 4 for the latter)");
    return IONODE_ERR_UNSUPPORTED;
  }
  // ---- 3. everything else from the variant ----
  const ionode::Variant *v = pl->v;
  const size_t tiles = (size_t)((d->n_traj + v->traj_per_tile - 1) / v->traj_per_tile);
  pl->grid = (unsigned)tiles;
  pl->block = 64u * v->G;
  pl->lds = v->lds_bytes(L, NT);
  // the lean 16-tile hands its LDS region to the 4-trajectory net when <= 4 of a tile's trajectories are left (MlpShrink4).  On by
  // default; IONODE_TILE_SHRINK=0 turns it off
  if (v->shrink) {
    pl->tile_shrink = k.tile_shrink;
    pl->lds = std::max(pl->lds, ionode::MlpTile4::lds_bytes(L));
  }
  if (v->lane_wise) plan_lane_wise(pl, tiles, ((pl->lds + 15) & ~(size_t)15) + (size_t)ionode::LwLds::bytes(2, v->lds_key));  // the net's region + the lane-wise region
  if (d->traj_per_image > 0) {
    // several weight images: a tile reads ONE image (first trajectory / traj_per_image), so an image's trajectories must fill whole tiles
    if (d->traj_per_image % v->traj_per_tile != 0 || d->mlp_image_stride < (int64_t)ionode_mlp_packed_floats(L, d->mlp_width)) {
      set_err("traj_per_image must be a multiple of the tile size (16; 64 with tile_waves = 64; 32 with tile_waves = 8) and mlp_image_stride at least one packed image");
      return IONODE_ERR_ARG;
    }
  }
  return IONODE_OK;
}

int make_plan(const ionode_desc *d, Plan *pl, const Request &r, const Switches &sw) {
#ifdef IONODE_STAMPS
  const bool has_step_log = false;   // diagnostic build: the step log carries the phase stamps and does not exclude the lean variants
#else
  const bool has_step_log = d->step_log != nullptr;
#endif
  const bool mlp = d->model == IONODE_MODEL_NNF || d->model == IONODE_MODEL_NND;
  const int D = d->model == IONODE_MODEL_MARKOV6 ? 6 : 2;
  if (d->model < 0 || d->model > 3) { set_err("unknown model"); return IONODE_ERR_ARG; }
  if (d->n_state != D) { set_err("n_state does not match model"); return IONODE_ERR_ARG; }
  if (d->n_traj < 1 || d->n_out < 1 || d->n_prot < 1 || d->prot_n < 2) { set_err("empty batch / grid / protocol"); return IONODE_ERR_ARG; }
  if (d->n_params < (D == 6 ? 12 : 8)) { set_err("n_params too small for model"); return IONODE_ERR_ARG; }
  if (!(d->rtol > 0) || !(d->atol >= 0) || !(d->prot_dt > 0)) { set_err("rtol/atol/prot_dt must be positive"); return IONODE_ERR_ARG; }
  const Ask k = {r.want_current, r.explicit_grid, has_step_log, r.objective == IONODE_OBJECTIVE_SAE, sw.tile_shrink};
  return mlp ? plan_mlp(d, pl, k) : plan_closed(d, pl, k, D);
}

// Deferred dense output (ionode_dense_expand.hpp): the record capacity per trajectory and the workspace bytes of a plan, both 0 when
// nothing is deferred -- a variant without KernelForm::defer, the fused objective, IONODE_DEFER_DENSE=0.  The records may take a
// quarter of the bytes of the requested outputs; fewer than 64 records per trajectory are not worth the second kernel.
// IONODE_DEFER_DENSE_CAP=n forces a capacity.
struct DeferPlan {
  int64_t cap = 0, bytes = 0;
};
DeferPlan plan_defer(const ionode_desc *d, const Plan &pl, bool want_i, const Switches &sw) {
  DeferPlan p;
  if (!pl.v->defer || d->sse_out != nullptr || d->n_state != 2 || !sw.defer_dense) return p;
  using Rec = ionode::DenseRecord<2>;
  const int64_t B = d->n_traj, Nt = d->n_out;
  int64_t cap = sw.defer_cap;
  const bool forced = cap > 0;
  if (!forced) {
    const int64_t out_bytes = B * Nt * 2 * (d->state_f32 ? 4 : 8) + (want_i ? B * Nt * 8 : 0);
    cap = (out_bytes / 4) / (B * Rec::BYTES);
  }
  cap = std::min<int64_t>(cap, Nt - 1);
  if (cap < (forced ? 1 : 64)) return p;
  p.cap = cap;
  p.bytes = (int64_t)Rec::workspace_bytes(B, cap);
  return p;
}

// The solve kernel's tail (ionode_device.hpp): how many tiles, in the order they end, expand their own records before they leave, and
// the records a trajectory may fill.  The launch lasts as long as its slowest tile; the first kDeferTailEighths / 8 of the tiles end at
// least twice a tile's expansion time before it does (profiles/defer_tail.md), the rest leave their records to the follow-up kernel.
// The finish counter lives in the workspace's last record slot, so with the tail on a trajectory fills cap - 1 records (the stride and
// the workspace stay what ionode_dense_defer_plan reports).  IONODE_DEFER_TAIL=0: no tile, IONODE_DEFER_TAIL=all: every tile,
// IONODE_DEFER_TAIL_RANK=n: n tiles.
// A composed launch (ionode_compose.hpp) ends its tiles at other times -- 255 of the headline's 256 within 10 ms of each other, the
// heaviest trajectory's tile 10 ms later -- so the fraction is a constant per cost source (ionode_dopri5_composed).  The rule's factor
// of two gives 0/8 and 1/8 there; the bench at 5/8 and 6/8 shows the in-kernel expansions still hidden (one expansion's margin), so all
// three are 5 (profiles/compose_order.md).
constexpr int64_t kDeferTailEighths = 5;
constexpr int64_t kDeferTailEighthsPilot = 5;
constexpr int64_t kDeferTailEighthsCounts = 5;
struct TailPlan {
  int64_t rank = 0, fill = 0;
};
TailPlan plan_tail(const Plan &pl, const DeferPlan &dp, int cost_source, const Switches &sw) {
  TailPlan t;
  t.fill = dp.cap;
  if (dp.cap < 2) return t;
  const int64_t tiles = (int64_t)pl.grid;
  t.rank = tiles * (cost_source == 1 ? kDeferTailEighthsPilot : cost_source == 2 ? kDeferTailEighthsCounts : kDeferTailEighths) / 8;
  if (sw.tail_rank_set) t.rank = std::max<int64_t>(0, std::min<int64_t>(sw.tail_rank, tiles));
  if (sw.tail == TailSwitch::All) t.rank = tiles;
  else if (sw.tail == TailSwitch::Off) t.rank = 0;
  if (t.rank > 0) t.fill = dp.cap - 1;
  return t;
}

// Shrink-aware tile composition (ionode_compose.hpp): a launch qualifies when it runs one of the four lean N = 200 shrink kernels with
// the shrink on, has at most one tile per compute unit of the caller's current device, asked on every plan (then every tile starts at
// once and the launch is as long as its slowest tile), no traj_per_image (a tile reads one image) and no order of the caller's.
// IONODE_COMPOSE=0|pilot|hint selects where the cost may come from: 0 composes nothing, pilot always runs the pilot, hint only ever
// reads an earlier call's stats.
bool plan_compose(const ionode_desc *d, const Plan &pl) {
  return pl.v->shrink && pl.tile_shrink && pl.v->traj_per_tile == ionode::kComposeTile && d->traj_per_image <= 0 &&
         d->launch_order == nullptr && d->n_traj <= ionode::kComposeMaxB && (int64_t)pl.grid <= (int64_t)ionode::compute_units();
}

// ---- everything decided about one launch ----
struct LaunchPlan {
  Plan kernel;
  DeferPlan defer;   // cap 0: nothing is deferred
  TailPlan tail;
  bool compose = false;   // the launch qualifies for the tile composition and IONODE_COMPOSE allows one
  ComposeSource source = kComposeAuto;
};
int plan_launch(const ionode_desc *d, const Request &r, LaunchPlan *lp) {
  if (!d) { set_err("null descriptor"); return IONODE_ERR_ARG; }
  const Switches sw = read_switches();
  const int rc = make_plan(d, &lp->kernel, r, sw);
  if (rc != IONODE_OK) return rc;
  // a workspace the plan does not use is ignored; with the fused objective want_current is not i_out, and nothing is deferred
  if (r.has_workspace && !r.explicit_grid && r.has_y_out) lp->defer = plan_defer(d, lp->kernel, r.want_current, sw);
  lp->tail = plan_tail(lp->kernel, lp->defer, r.cost_source, sw);
  lp->source = sw.compose;
  lp->compose = sw.compose != kComposeOff && plan_compose(d, lp->kernel);
  return IONODE_OK;
}

}  // namespace
