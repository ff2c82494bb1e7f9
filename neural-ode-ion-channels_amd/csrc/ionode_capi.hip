// ionode_capi.hip -- the C ABI of libionode.so (include/ionode.h): argument checking, choice of
// kernel instantiation and launch geometry, and the host-side re-layout of an nn.Sequential
// state dict into the MFMA fragment order the kernels stream.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ionode_compose.hpp"
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
thread_local const char *g_last_kernel = "";  // variant name of this thread's last successful ionode_dopri5 launch

void set_err(const char *fmt, const char *detail = "") { snprintf(g_err, sizeof g_err, fmt, detail); }

inline int np_of(int N) { return 16 * ((N + 15) / 16); }

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
  // compute units of the current device (256 on an unpartitioned MI355X).  The padding assumes the 8-XCD round-robin of the whole
  // chip: on a partitioned device (CPX / DPX) it is skipped; without a device (the plan is also computed on hosts without a GPU) it is applied
  static const int ncu_dev = [] {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) { (void)hipGetLastError(); return 0; }
    return n;
  }();
  const size_t ncu = 256;
  const size_t per_cu = (pl->grid + ncu - 1) / ncu;
  const size_t natural = cap / (((lds + gran - 1) / gran) * gran);
  if ((ncu_dev == 0 || ncu_dev == (int)ncu) && per_cu >= 1 && per_cu < natural) {
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

// What the caller asks for beyond the descriptor's own fields
struct Ask {
  bool want_current;    // a current trace or the fused objective
  bool explicit_grid;   // prot_t given
  bool has_step_log;
  bool abs_objective;   // the fused objective sums absolute residuals (ionode_dopri5_objective)
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
  // default; IONODE_TILE_SHRINK=0 turns it off (dev override for A/B runs, read per plan)
  if (v->shrink) {
    const char *ts = getenv("IONODE_TILE_SHRINK");
    pl->tile_shrink = ts == nullptr || ts[0] == '\0' || atoi(ts) != 0;
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

// Deferred dense output (ionode_dense_expand.hpp): the record capacity per trajectory and the workspace bytes of a plan, both 0 when
// nothing is deferred -- a variant without KernelForm::defer, the fused objective, IONODE_DEFER_DENSE=0.  The records may take a
// quarter of the bytes of the requested outputs; fewer than 64 records per trajectory are not worth the second kernel.
// IONODE_DEFER_DENSE_CAP=n forces a capacity (dev overrides for A/B runs and tests, read per plan like IONODE_TILE_SHRINK).
struct DeferPlan {
  int64_t cap = 0, bytes = 0;
};
DeferPlan plan_defer(const ionode_desc *d, const Plan &pl, bool want_i) {
  DeferPlan p;
  if (!pl.v->defer || d->sse_out != nullptr || d->n_state != 2) return p;
  const char *sw = getenv("IONODE_DEFER_DENSE");
  if (sw != nullptr && sw[0] != '\0' && atoi(sw) == 0) return p;
  using Rec = ionode::DenseRecord<2>;
  const int64_t B = d->n_traj, Nt = d->n_out;
  const char *fc = getenv("IONODE_DEFER_DENSE_CAP");
  int64_t cap = (fc != nullptr && fc[0] != '\0') ? atoll(fc) : 0;
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
// IONODE_DEFER_TAIL_RANK=n: n tiles (dev overrides for A/B runs and tests, read per plan like IONODE_TILE_SHRINK).
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
TailPlan plan_tail(const Plan &pl, const DeferPlan &dp, int cost_source = 0) {
  TailPlan t;
  t.fill = dp.cap;
  if (dp.cap < 2) return t;
  const int64_t tiles = (int64_t)pl.grid;
  t.rank = tiles * (cost_source == 1 ? kDeferTailEighthsPilot : cost_source == 2 ? kDeferTailEighthsCounts : kDeferTailEighths) / 8;
  const char *fr = getenv("IONODE_DEFER_TAIL_RANK");
  if (fr != nullptr && fr[0] != '\0') t.rank = std::max<int64_t>(0, std::min<int64_t>(atoll(fr), tiles));
  const char *sw = getenv("IONODE_DEFER_TAIL");
  if (sw != nullptr && sw[0] != '\0') {
    if (strcmp(sw, "all") == 0) t.rank = tiles;
    else if (atoi(sw) == 0) t.rank = 0;
  }
  if (t.rank > 0) t.fill = dp.cap - 1;
  return t;
}

// Shrink-aware tile composition (ionode_compose.hpp): a launch qualifies when it runs one of the four lean N = 200 shrink kernels with
// the shrink on, has at most one tile per compute unit (then every tile starts at once and the launch is as long as its slowest tile),
// no traj_per_image (a tile reads one image) and no order of the caller's.  IONODE_COMPOSE=0|pilot|hint selects where the cost may
// come from (dev override for A/B runs, read per plan like IONODE_TILE_SHRINK): 0 composes nothing, pilot always runs the pilot, hint
// only ever reads an earlier call's stats.
enum ComposeSource : int32_t { kComposeOff = 0, kComposePilot = 1, kComposeHint = 2, kComposeAuto = 3 };
ComposeSource compose_source() {
  const char *sw = getenv("IONODE_COMPOSE");
  if (sw == nullptr || sw[0] == '\0') return kComposeAuto;
  if (strcmp(sw, "pilot") == 0) return kComposePilot;
  if (strcmp(sw, "hint") == 0) return kComposeHint;
  return atoi(sw) == 0 ? kComposeOff : kComposeAuto;
}
// compute units of the CALLER's current device, asked on every plan (a process may drive several devices, or partitions of one);
// 256 -- an unpartitioned MI355X -- where there is no device (plans are also computed on hosts without a GPU)
int compute_units_now() {
  int dev = 0, n = 0;
  if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n < 1) {
    (void)hipGetLastError();
    return 256;
  }
  return n;
}
bool plan_compose(const ionode_desc *d, const Plan &pl) {
  return pl.v->shrink && pl.tile_shrink && pl.v->traj_per_tile == ionode::kComposeTile && d->traj_per_image <= 0 &&
         d->launch_order == nullptr && d->n_traj <= ionode::kComposeMaxB && (int64_t)pl.grid <= (int64_t)compute_units_now();
}

int make_plan(const ionode_desc *d, Plan *pl, bool want_current = false, bool explicit_grid = false, bool abs_objective = false) {
  if (!d) { set_err("null descriptor"); return IONODE_ERR_ARG; }
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
  const Ask k = {want_current, explicit_grid, has_step_log, abs_objective};
  return mlp ? plan_mlp(d, pl, k) : plan_closed(d, pl, k, D);
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

// ---- the packed weight image (ionode_mlp_pack): one size function and one packer per SECTION ----
// Tuned widths:   layer 0 | L x (fragment stream, bias[NP]) | output layer | N <= 16: scalar row pairs | N = 200: 4-trajectory, one-trajectory sections
// Other widths:   layer 0 | L x (generic fragments, bias[NP]) | output layer
namespace {

// Wavefronts per tile of the tuned 16-trajectory tile that serves width N (the fragment stream is laid out per wavefront); false: none.
bool tile_shape(int N, int *G) {
  const ionode::Variant *v = find_variant(IONODE_MODEL_NNF, 0, ionode::Net::Tile, ionode::Lean::General, 16, 0, np_of(N) / 16);
  if (!v) return false;
  *G = v->G;
  return true;
}

// widths without a tuned tile: the image of the run-time-width tile (ionode_mlp_gen.hpp MlpGen)
bool generic_width(int N) {
  int G;
  const int NT = np_of(N) / 16;
  return N >= 1 && !tile_shape(N, &G) && NT >= 2 && NT <= ionode::MlpGen::NT_MAX;
}

// 1 KiB fragments per wavefront per hidden layer: F per step, + R on the steps s % G == 0 (K-slices of the remainder tiles)
size_t frags_per_wave(int NT, int G) {
  const int F = NT / G, R = NT - G * F, NOWN = (NT + G - 1) / G;
  return (size_t)NT * F + (size_t)NOWN * R;
}

// the reference's flat state dict: W0[N][2], b0[N], L x (W[N][N], b[N]), wl[N], bl
struct FlatNet {
  const float *w;
  int L, N;
  const float *W0() const { return w; }
  const float *b0() const { return w + (size_t)2 * N; }
  const float *W(int l) const { return w + (size_t)3 * N + (size_t)l * ((size_t)N * N + N); }
  const float *b(int l) const { return W(l) + (size_t)N * N; }
  const float *wl() const { return W(L); }
};

// element (row, k) of a hidden layer, zero in the padding
inline float wpad(const float *W, int N, int row, int k) { return (row < N && k < N) ? W[(size_t)row * N + k] : 0.0f; }

// layer 0: rows {b0, w00, w01, 0}
size_t layer0_floats(int NP) { return 4 * (size_t)NP; }
void pack_layer0(const FlatNet &n, float *out) {
  for (int r = 0; r < n.N; ++r) {
    out[4 * r + 0] = n.b0()[r];
    out[4 * r + 1] = n.W0()[2 * r + 0];
    out[4 * r + 2] = n.W0()[2 * r + 1];
  }
}

// output layer: wl[NP], bl, 3 pad
size_t output_floats(int NP) { return (size_t)NP + 4; }
void pack_output(const FlatNet &n, int NP, float *out) {
  for (int k = 0; k < n.N; ++k) out[k] = n.wl()[k];
  out[NP] = n.wl()[n.N];
}

// one hidden layer of the 16-column fragment stream, then its bias[NP]
size_t stream_layer_floats(int NT, int G) { return (size_t)G * frags_per_wave(NT, G) * 256 + (size_t)16 * NT; }
void pack_stream_layer(const float *W, const float *b, int N, int NT, int G, float *dst) {
  const int F = NT / G, Rm = NT - G * F;
  const size_t FR = frags_per_wave(NT, G);
  // A operand of v_mfma_f32_16x16x4_f32: lane = 16q + m supplies row 16*rt + m, k = 16*kt + 4*q + r.
  // Stream order: wavefront wv | step s, k-tile kt = (s + wv) mod NT | fragments | lane.  F fragments hold the full
  // row tiles wv + i*G k-step-major (element e = r*F + i -> fragment e/4, component e%4); steps with s % G == 0 add
  // one fragment per remainder tile G*F + j (component = k-step r), zero when the step wraps (s + wv >= NT).
  for (int wv = 0; wv < G; ++wv) {
    size_t pos = 0;  // fragment index inside this wavefront's layer stream
    for (int st = 0; st < NT; ++st) {
      const int kt = (st + wv) % NT;
      for (int lane = 0; lane < 64; ++lane) {
        const int m = lane & 15, q = lane >> 4;
        float *f0 = dst + (((size_t)wv * FR + pos) * 64 + lane) * 4;
        // the asm tile's short form of the half-padded k-tile 12 (N <= 200, ionode_mlp_tile.hpp IONODE_KT12_SHORT): MFMA r = 0 takes
        // k = 192, 196, 193, 197 from the lane groups q = 0..3, MFMA r = 1 takes 194, 198, 195, 199; r = 2, 3 are not executed
        const bool short12 = IONODE_KT12_SHORT && NT == 13 && G == 4 && N <= 200 && kt == 12;
        auto kof = [&](int r) { return short12 ? (r < 2 ? 192 + 4 * (q & 1) + (q >> 1) + 2 * r : N) : 16 * kt + 4 * q + r; };
        for (int e = 0; e < 4 * F; ++e) {
          const int r = e / F, i = e % F, rt = wv + i * G;
          f0[(size_t)(e / 4) * 256 + e % 4] = wpad(W, N, 16 * rt + m, kof(r));
        }
        if (Rm > 0 && st % G == 0)
          for (int j = 0; j < Rm; ++j)
            for (int r = 0; r < 4; ++r)
              f0[(size_t)(F + j) * 256 + r] = (st + wv < NT) ? wpad(W, N, 16 * (G * F + j) + m, kof(r)) : 0.0f;
      }
      pos += F + ((Rm > 0 && st % G == 0) ? Rm : 0);
    }
  }
  float *bias = dst + (size_t)G * FR * 256;
  for (int r = 0; r < N; ++r) bias[r] = b[r];
}

// one hidden layer of the generic layout (MlpGen): [rt][kt][lane = 16 q + m] float4 over r of W[16 rt + m][16 kt + 4 q + r], then bias[NP]
void pack_generic_layer(const float *W, const float *b, int N, int NT, float *dst) {
  for (int rt = 0; rt < NT; ++rt)
    for (int kt = 0; kt < NT; ++kt)
      for (int lane = 0; lane < 64; ++lane) {
        const int m = lane & 15, q = lane >> 4;
        float *f = dst + (((size_t)rt * NT + kt) * 64 + lane) * 4;
        for (int r = 0; r < 4; ++r) f[r] = wpad(W, N, 16 * rt + m, 16 * kt + 4 * q + r);
      }
  float *bias = dst + (size_t)NT * NT * 256;
  for (int r = 0; r < N; ++r) bias[r] = b[r];
}

// one layer of the 4-trajectory tile's section (ionode_mlp_tile4.hpp MlpTile4), round-5 lane layout: wavefronts 0..2: [w][step s][q][lane = 4 b + i]
// float4 over r of W[row][16 kt + 4 q + r], block b = 4 g + u: row 16 (4 w + g) + 4 u + i, kt = (s + g) mod 13; wavefront 3 (partial chains of
// the remainder rows): [step j][q][lane] float4 over r of W[192 + 4 u + i][16 (c + 4 j) + 4 q + r] with c = g, -0.0f where c + 4 j > 12; then per
// (wavefront, lane) the accumulator start float4 {bias of rows i = 0..3 of the lane's block} (chains c > 0: 0)
void pack_tile4_layer(const float *W, const float *b, int N, float *lay) {
  for (int wv = 0; wv < 3; ++wv)
    for (int st = 0; st < 13; ++st)
      for (int q = 0; q < 4; ++q)
        for (int lane = 0; lane < 64; ++lane) {
          const int i = lane & 3, bb = lane >> 2, g = bb >> 2, u = bb & 3;
          float *f = lay + ((((size_t)wv * 13 + st) * 4 + q) * 64 + lane) * 4;
          const int row = 16 * (4 * wv + g) + 4 * u + i, kt = (st + g) % 13;
          for (int r = 0; r < 4; ++r) f[r] = wpad(W, N, row, 16 * kt + 4 * q + r);
        }
  float *rem = lay + (size_t)3 * 13 * 4 * 256;
  for (int jj = 0; jj < 4; ++jj)
    for (int q = 0; q < 4; ++q)
      for (int lane = 0; lane < 64; ++lane) {
        const int i = lane & 3, bb = lane >> 2, c = bb >> 2, u = bb & 3;
        float *f = rem + (((size_t)jj * 4 + q) * 64 + lane) * 4;
        const int row = 192 + 4 * u + i, kt = c + 4 * jj;
        for (int r = 0; r < 4; ++r) f[r] = (kt >= 13) ? -0.0f : wpad(W, N, row, 16 * kt + 4 * q + r);
      }
  float *bias = rem + (size_t)4 * 4 * 256;
  for (int wv = 0; wv < 4; ++wv)
    for (int lane = 0; lane < 64; ++lane) {
      const int bb = lane >> 2, g = bb >> 2, u = bb & 3;
      for (int i = 0; i < 4; ++i) {
        const int row = (wv < 3) ? 16 * (4 * wv + g) + 4 * u + i : 192 + 4 * u + i;
        bias[((size_t)wv * 64 + lane) * 4 + i] = (row < N && (wv < 3 || g == 0)) ? b[row] : 0.0f;
      }
    }
}

// one layer of the one-trajectory tile's section (ionode_mlp_row1.hpp MlpRow1): wavefronts 0..2: [w][step s][r][lane] float4 over q of
// W[64 w + lane][16 ((s + lane / 16) mod 13) + 4 q + r]; wavefront 3 (partial chains of the remainder rows): [step j][r][lane = 16 c + i]
// float4 over q of W[192 + i][16 (c + 4 j) + 4 q + r], -0.0f where c + 4 j > 12; then per (wavefront, lane) the accumulator start (the
// row's bias; chains c > 0: 0)
void pack_row1_layer(const float *W, const float *b, int N, float *lay) {
  for (int wv = 0; wv < 3; ++wv)
    for (int st = 0; st < 13; ++st)
      for (int r = 0; r < 4; ++r)
        for (int lane = 0; lane < 64; ++lane) {
          float *f = lay + ((((size_t)wv * 13 + st) * 4 + r) * 64 + lane) * 4;
          const int row = 64 * wv + lane, kt = (st + (lane >> 4)) % 13;
          for (int q = 0; q < 4; ++q) f[q] = wpad(W, N, row, 16 * kt + 4 * q + r);
        }
  float *rem = lay + (size_t)3 * 13 * 4 * 256;
  for (int j = 0; j < 4; ++j)
    for (int r = 0; r < 4; ++r)
      for (int lane = 0; lane < 64; ++lane) {
        float *f = rem + (((size_t)j * 4 + r) * 64 + lane) * 4;
        const int row = 192 + (lane & 15), kt = (lane >> 4) + 4 * j;
        for (int q = 0; q < 4; ++q) f[q] = (kt >= 13) ? -0.0f : wpad(W, N, row, 16 * kt + 4 * q + r);
      }
  float *bias = rem + (size_t)4 * 4 * 256;
  for (int wv = 0; wv < 4; ++wv)
    for (int lane = 0; lane < 64; ++lane) {
      const int row = (wv < 3) ? 64 * wv + lane : 192 + (lane & 15);
      bias[wv * 64 + lane] = (row < N && (wv < 3 || lane < 16)) ? b[row] : 0.0f;
    }
}

// scalar section (ionode_mlp_lane.hpp MlpLane), in row PAIRS (2 m, 2 m + 1) -- the two halves of a v_pk_fma_f32; an odd N's last
// pair has a zero second row.  Layer 0: {b0, b0'} {w00, w00'} {w01, w01'} {0, 0}.  Hidden layer l, pair m: {W[2m][k], W[2m+1][k]}
// for k = 4 q + r < N in the order r-major / q-minor (the order in which the 16 x 16 x 4 MFMA tile accumulates them), then the
// biases as bias + 0.0f (a -0 bias becomes +0: see MlpLane), pad to a multiple of 4 floats.
int scalar_pairs(int N) { return (N + 1) / 2; }
int scalar_block(int N) { return (2 * (N + 1) + 3) & ~3; }
size_t scalar_floats(int L, int N) { return (size_t)scalar_pairs(N) * 8 + (size_t)L * scalar_pairs(N) * scalar_block(N); }
void pack_scalar(const FlatNet &n, float *sc) {
  const int N = n.N, NPAIR = scalar_pairs(N), PB = scalar_block(N);
  float *sh = sc + NPAIR * 8;
  for (int j = 0; j < N; ++j) {
    const int m = j / 2, e = j % 2;
    sc[m * 8 + 0 + e] = n.b0()[j];
    sc[m * 8 + 2 + e] = n.W0()[2 * j + 0];
    sc[m * 8 + 4 + e] = n.W0()[2 * j + 1];
    for (int l = 0; l < n.L; ++l) {
      float *blk = sh + ((size_t)l * NPAIR + m) * PB;
      int pos = 0;
      for (int r = 0; r < 4; ++r)
        for (int q = 0; q < 4; ++q)
          if (4 * q + r < N) blk[2 * (pos++) + e] = n.W(l)[(size_t)j * N + 4 * q + r];
      blk[2 * N + e] = (N < 16) ? n.b(l)[j] + 0.0f : n.b(l)[j];
    }
  }
}

// where the sections of the image of an (L, N) net start; total == 0: no kernel serves the width
struct ImageLayout {
  bool generic = false;
  int G = 0, NP = 0, NT = 0;
  size_t layer = 0;   // floats per hidden layer of the main stream
  size_t hidden = 0, output = 0, scalar = 0, tile4 = 0, row1 = 0, total = 0;
};
ImageLayout image_layout(int L, int N) {
  ImageLayout y;
  if (L < 0 || N < 1) return y;
  y.generic = generic_width(N);
  if (!y.generic && !tile_shape(N, &y.G)) return y;
  y.NP = np_of(N); y.NT = y.NP / 16;
  y.layer = y.generic ? ionode::MlpGen::layer_floats(y.NT) : stream_layer_floats(y.NT, y.G);
  y.hidden = layer0_floats(y.NP);
  y.output = y.hidden + (size_t)L * y.layer;
  y.scalar = y.output + output_floats(y.NP);
  y.tile4 = y.scalar + ((!y.generic && y.NT == 1) ? scalar_floats(L, N) : 0);                       // N <= 16: the per-lane net's section
  y.row1 = y.tile4 + ((!y.generic && y.NT == 13) ? (size_t)L * ionode::MlpTile4::layer_floats() : 0);   // N = 200: the 4-trajectory tile's ...
  y.total = y.row1 + ((!y.generic && y.NT == 13) ? (size_t)L * ionode::MlpRow1::layer_floats() : 0);    // ... and the one-trajectory tile's
  return y;
}

}  // namespace

extern "C" {

int32_t ionode_abi_version(void) { return IONODE_ABI_VERSION; }

const char *ionode_last_error(void) { return g_err; }

size_t ionode_mlp_packed_floats(int32_t L, int32_t N) { return image_layout(L, N).total; }

int ionode_mlp_pack(const float *w, int32_t L, int32_t N, float *out) {
  if (!w || !out || L < 0 || N < 1) { set_err("ionode_mlp_pack: bad argument"); return IONODE_ERR_ARG; }
  const ImageLayout y = image_layout(L, N);
  if (y.total == 0) { set_err("ionode_mlp_pack: MLP width outside the supported range (1 <= N <= 512)"); return IONODE_ERR_UNSUPPORTED; }
  const FlatNet n = {w, L, N};
  memset(out, 0, y.total * sizeof(float));
  pack_layer0(n, out);
  for (int l = 0; l < L; ++l) {
    float *dst = out + y.hidden + (size_t)l * y.layer;
    if (y.generic) pack_generic_layer(n.W(l), n.b(l), N, y.NT, dst);
    else pack_stream_layer(n.W(l), n.b(l), N, y.NT, y.G, dst);
  }
  pack_output(n, y.NP, out + y.output);
  if (y.tile4 > y.scalar) pack_scalar(n, out + y.scalar);
  for (int l = 0; l < L && y.row1 > y.tile4; ++l) pack_tile4_layer(n.W(l), n.b(l), N, out + y.tile4 + (size_t)l * ionode::MlpTile4::layer_floats());
  for (int l = 0; l < L && y.total > y.row1; ++l) pack_row1_layer(n.W(l), n.b(l), N, out + y.row1 + (size_t)l * ionode::MlpRow1::layer_floats());
  return IONODE_OK;
}

int ionode_launch_geometry(const ionode_desc *d, int32_t out[4]) {
  Plan pl;
  const int rc = make_plan(d, &pl);
  if (rc != IONODE_OK) return rc;
  out[0] = (int32_t)pl.grid;
  out[1] = (int32_t)pl.block;
  out[2] = (int32_t)pl.lds;
  out[3] = pl.v->G;
  return IONODE_OK;
}

const char *ionode_kernel_name(const ionode_desc *d) {
  Plan pl;
  // the descriptor does not say whether i_out will be passed: a table or a fused objective implies the epilogue
  if (make_plan(d, &pl, d && (d->sse_out != nullptr || d->v_at_outputs != nullptr)) != IONODE_OK) return "";
  return pl.v->name;
}

const char *ionode_last_kernel_name(void) { return g_last_kernel; }

int32_t ionode_lane_wise_from(int32_t model, int32_t mlp_width) { return lane_wise_from(model, mlp_width); }

int ionode_dense_defer_plan(const ionode_desc *d, int32_t want_current, int64_t out[2]) {
  Plan pl;
  const int rc = make_plan(d, &pl, want_current != 0 || (d && d->sse_out != nullptr));
  if (rc != IONODE_OK) return rc;
  const DeferPlan dp = plan_defer(d, pl, want_current != 0);
  out[0] = dp.cap;
  out[1] = dp.bytes;
  return IONODE_OK;
}

int ionode_dense_tail_plan(const ionode_desc *d, int32_t want_current, int64_t out[2]) {
  Plan pl;
  const int rc = make_plan(d, &pl, want_current != 0 || (d && d->sse_out != nullptr));
  if (rc != IONODE_OK) return rc;
  const TailPlan tp = plan_tail(pl, plan_defer(d, pl, want_current != 0));
  out[0] = tp.rank;
  out[1] = tp.fill;
  return IONODE_OK;
}


int ionode_compose_tail_plan(const ionode_desc *d, int32_t want_current, int32_t cost_source, int64_t out[2]) {
  Plan pl;
  const int rc = make_plan(d, &pl, want_current != 0 || (d && d->sse_out != nullptr));
  if (rc != IONODE_OK) return rc;
  if (cost_source < 0 || cost_source > 2) { set_err("cost_source: 0 (not composed), 1 (pilot) or 2 (counts)"); return IONODE_ERR_ARG; }
  const TailPlan tp = plan_tail(pl, plan_defer(d, pl, want_current != 0), d->launch_order ? cost_source : 0);
  out[0] = tp.rank;
  out[1] = tp.fill;
  return IONODE_OK;
}

int ionode_compose_plan(const ionode_desc *d, int32_t want_current, int32_t out[2]) {
  Plan pl;
  const int rc = make_plan(d, &pl, want_current != 0 || (d && d->sse_out != nullptr));
  if (rc != IONODE_OK) return rc;
  const ComposeSource src = compose_source();
  out[0] = (src != kComposeOff && plan_compose(d, pl)) ? 1 : 0;
  out[1] = (int32_t)src;
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
    if (ea != hipSuccess) { set_err("kernel launch failed: %s", hipGetErrorString(ea)); return IONODE_ERR_LAUNCH; }
  }
  hipLaunchKernelGGL(kern, dim3(1), dim3(ionode::kComposeThreads), lds, reinterpret_cast<hipStream_t>(stream), cost, (long long)cost_stride,
                     (int)n_traj, order);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) { set_err("kernel launch failed: %s", hipGetErrorString(e)); return IONODE_ERR_LAUNCH; }
  return IONODE_OK;
}

}  // extern "C"

namespace {

// ionode_dopri5 and ionode_dopri5_deferred: the solve and, when the plan defers the dense output into `workspace`, its expansion
int dopri5_impl(const ionode_desc *d, const float *mlp_packed, const double *params, const double *prot_v,
                const double *prot_t, const int32_t *prot_of_traj, const void *y0, const double *t_eval,
                void *y_out, double *i_out, int32_t *status, int64_t *stats, void *stream, void *workspace, int64_t workspace_bytes,
                int cost_source = 0, int objective = IONODE_OBJECTIVE_SSE) {
  Plan pl;
  const int rc = make_plan(d, &pl, i_out != nullptr || d->sse_out != nullptr, prot_t != nullptr, objective == IONODE_OBJECTIVE_SAE);
  if (rc != IONODE_OK) return rc;
  const bool mlp = d->model == IONODE_MODEL_NNF || d->model == IONODE_MODEL_NND;
  if (!params || !prot_v || !y0 || !t_eval || (!y_out && !d->sse_out) || !status || (mlp && !mlp_packed)) {
    set_err("ionode_dopri5: required buffer is NULL");
    return IONODE_ERR_ARG;
  }
  if (d->sse_out && (!d->sse_ref || !(d->t_eval_dt_hint > 0.0) || d->n_out < 2)) {
    set_err("fused objective: sse_out needs sse_ref and the output-grid hint (t_eval_dt_hint > 0)");
    return IONODE_ERR_ARG;
  }
  ionode::KArgs a;
  memset(&a, 0, sizeof a);
  a.mlp = mlp_packed; a.params = params; a.prot_v = prot_v; a.prot_t = prot_t; a.prot_of_traj = prot_of_traj;
  a.y0 = y0; a.t_eval = t_eval; a.y_out = y_out; a.i_out = i_out; a.status = status; a.stats = stats;
  a.B = d->n_traj; a.Nt = d->n_out; a.P = d->n_prot; a.Np = d->prot_n; a.n_params = d->n_params;
  if (mlp) { a.L = d->mlp_layers; a.N = d->mlp_width; a.NP = np_of(d->mlp_width); a.NT = a.NP / 16; }
  a.max_steps = d->max_steps > 0 ? d->max_steps : (int64_t)2147483647;  // torchdiffeq max_num_steps default 2**31 - 1
  a.max_total = d->max_total_steps > 0 ? d->max_total_steps
                                       : (d->max_total_steps == 0 ? (int64_t)IONODE_DEFAULT_MAX_TOTAL_STEPS : INT64_MAX);
  a.ckpt = d->ckpt; a.ckpt_cap = d->ckpt ? d->ckpt_cap : 0;
  if (d->ckpt && d->ckpt_cap < 1) { set_err("ckpt given with ckpt_cap < 1"); return IONODE_ERR_ARG; }
  a.prot_rdt = 1.0 / d->prot_dt;  // correctly rounded: the kernels divide by prot_dt through div_by()
  a.dt_max = d->max_step > 0.0 ? d->max_step : __builtin_inf();
  a.prot_t0 = d->prot_t0; a.prot_dt = d->prot_dt; a.v_oob = d->v_oob; a.rtol = d->rtol; a.atol = d->atol;
  a.obs_g = d->obs_g; a.obs_e = d->obs_e; a.obs_open = d->obs_open_state_only;
  a.step_log = d->step_log; a.step_log_cap = d->step_log ? d->step_log_cap : 0;
  a.sse_ref = d->sse_ref; a.sse_out = d->sse_out; a.v_tab = d->v_at_outputs;
  a.obj_abs = objective == IONODE_OBJECTIVE_SAE ? 1 : 0;
  if (mlp && d->traj_per_image > 0) { a.mlp_stride = d->mlp_image_stride; a.traj_per_img = d->traj_per_image; }  // checked in make_plan
  if (d->launch_order) {
    if (a.traj_per_img > 0) { set_err("launch_order cannot be combined with traj_per_image (tiles of an image must stay together)"); return IONODE_ERR_ARG; }
    a.order = d->launch_order;
  }
  a.lw_bytes = (int32_t)pl.lw_bytes;
  a.te_t0 = d->t_eval_t0_hint; a.te_dt = (d->t_eval_dt_hint > 0.0 && d->n_out > 1) ? d->t_eval_dt_hint : 0.0;
  a.te_rdt = a.te_dt > 0.0 ? 1.0 / a.te_dt : 0.0;
  a.te_exact = (a.te_dt > 0.0 && d->t_eval_exact) ? 1 : 0;
  a.tile_shrink = pl.tile_shrink ? 1 : 0;
  // deferred dense output: the plan's capacity again (with what this call really asks for); a workspace it does not use is ignored
  DeferPlan dp;
  if (workspace != nullptr && prot_t == nullptr && y_out != nullptr) dp = plan_defer(d, pl, i_out != nullptr);
  if (dp.cap > 0) {
    if (workspace_bytes < dp.bytes || (reinterpret_cast<uintptr_t>(workspace) & 15) != 0) {
      set_err("ionode_dopri5_deferred: workspace smaller than ionode_dense_defer_plan() asks for, or not 16-byte aligned");
      return IONODE_ERR_ARG;
    }
    a.defer_count = static_cast<int32_t *>(workspace);
    a.defer_rec = reinterpret_cast<double *>(static_cast<unsigned char *>(workspace) + ionode::DenseRecord<2>::records_offset(d->n_traj));
    a.defer_cap = (int32_t)dp.cap;
    const TailPlan tp = plan_tail(pl, dp, d->launch_order ? cost_source : 0);
    a.defer_fill = (int32_t)tp.fill;
    a.defer_tail_rank = (int32_t)tp.rank;
    if (tp.rank > 0) {
      // the tail block: the last record slot (no trajectory fills it), zeroed in stream order ahead of the solve
      a.defer_tail = reinterpret_cast<int32_t *>(a.defer_rec + ((size_t)d->n_traj * (size_t)dp.cap - 1) * ionode::DenseRecord<2>::ROW);
      const hipError_t em = hipMemsetAsync(a.defer_tail, 0, ionode::DenseRecord<2>::BYTES, reinterpret_cast<hipStream_t>(stream));
      if (em != hipSuccess) { set_err("hipMemsetAsync failed: %s", hipGetErrorString(em)); return IONODE_ERR_LAUNCH; }
    }
  }
  hipError_t e = pl.v->fn(a, pl.grid, pl.lds, reinterpret_cast<hipStream_t>(stream));
  if (e != hipSuccess) { set_err("kernel launch failed: %s", hipGetErrorString(e)); return IONODE_ERR_LAUNCH; }
  if (dp.cap > 0) {
    const int64_t blocks = std::min<int64_t>((dp.cap + ionode::kExpandRecordsPerWg - 1) / ionode::kExpandRecordsPerWg, ionode::kExpandMaxBlocks);
    const dim3 grid((unsigned)std::min<int64_t>((int64_t)d->n_traj * blocks, ionode::kExpandGrid));
    if (d->state_f32) hipLaunchKernelGGL((ionode::ionode_dense_expand_kernel<float, 2>), grid, dim3(256), 0, reinterpret_cast<hipStream_t>(stream), a);
    else hipLaunchKernelGGL((ionode::ionode_dense_expand_kernel<double, 2>), grid, dim3(256), 0, reinterpret_cast<hipStream_t>(stream), a);
    e = hipGetLastError();
    if (e != hipSuccess) { set_err("kernel launch failed: %s", hipGetErrorString(e)); return IONODE_ERR_LAUNCH; }
  }
  g_last_kernel = pl.v->name;
  return IONODE_OK;
}

}  // namespace

extern "C" {

int ionode_dopri5(const ionode_desc *d, const float *mlp_packed, const double *params, const double *prot_v,
                  const double *prot_t, const int32_t *prot_of_traj, const void *y0, const double *t_eval,
                  void *y_out, double *i_out, int32_t *status, int64_t *stats, void *stream) {
  return dopri5_impl(d, mlp_packed, params, prot_v, prot_t, prot_of_traj, y0, t_eval, y_out, i_out, status, stats, stream, nullptr, 0);
}

int ionode_dopri5_deferred(const ionode_desc *d, const float *mlp_packed, const double *params, const double *prot_v,
                           const double *prot_t, const int32_t *prot_of_traj, const void *y0, const double *t_eval,
                           void *y_out, double *i_out, int32_t *status, int64_t *stats, void *stream, void *workspace,
                           int64_t workspace_bytes) {
  return dopri5_impl(d, mlp_packed, params, prot_v, prot_t, prot_of_traj, y0, t_eval, y_out, i_out, status, stats, stream, workspace,
                     workspace_bytes);
}

int ionode_dopri5_composed(const ionode_desc *d, const float *mlp_packed, const double *params, const double *prot_v,
                           const double *prot_t, const int32_t *prot_of_traj, const void *y0, const double *t_eval,
                           void *y_out, double *i_out, int32_t *status, int64_t *stats, void *stream, void *workspace,
                           int64_t workspace_bytes, int32_t cost_source) {
  if (cost_source < 0 || cost_source > 2) { set_err("cost_source: 0 (not composed), 1 (pilot) or 2 (counts)"); return IONODE_ERR_ARG; }
  return dopri5_impl(d, mlp_packed, params, prot_v, prot_t, prot_of_traj, y0, t_eval, y_out, i_out, status, stats, stream, workspace,
                     workspace_bytes, cost_source);
}

int ionode_dopri5_objective(const ionode_desc *d, const float *mlp_packed, const double *params, const double *prot_v,
                            const double *prot_t, const int32_t *prot_of_traj, const void *y0, const double *t_eval,
                            void *y_out, double *i_out, int32_t *status, int64_t *stats, void *stream, void *workspace,
                            int64_t workspace_bytes, int32_t cost_source, int32_t objective) {
  // the kind first: whatever else is wrong with the call, an unknown kind or absolute values without a fused objective is what it reports
  if (objective != IONODE_OBJECTIVE_SSE && objective != IONODE_OBJECTIVE_SAE) {
    set_err("ionode_dopri5_objective: objective must be IONODE_OBJECTIVE_SSE (0) or IONODE_OBJECTIVE_SAE (1)");
    return IONODE_ERR_ARG;
  }
  if (objective == IONODE_OBJECTIVE_SAE && (d == nullptr || d->sse_out == nullptr)) {
    set_err("ionode_dopri5_objective: IONODE_OBJECTIVE_SAE needs the fused objective's output, d->sse_out");
    return IONODE_ERR_ARG;
  }
  if (objective == IONODE_OBJECTIVE_SSE) {
    return ionode_dopri5_composed(d, mlp_packed, params, prot_v, prot_t, prot_of_traj, y0, t_eval, y_out, i_out, status, stats, stream,
                                  workspace, workspace_bytes, cost_source);
  }
  if (cost_source < 0 || cost_source > 2) { set_err("cost_source: 0 (not composed), 1 (pilot) or 2 (counts)"); return IONODE_ERR_ARG; }
  return dopri5_impl(d, mlp_packed, params, prot_v, prot_t, prot_of_traj, y0, t_eval, y_out, i_out, status, stats, stream, workspace,
                     workspace_bytes, cost_source, objective);
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
  if (e != hipSuccess) { set_err("kernel launch failed: %s", hipGetErrorString(e)); return IONODE_ERR_LAUNCH; }
  return IONODE_OK;
}

}  // extern "C"
