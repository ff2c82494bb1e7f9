// ionode_form.hpp -- KernelForm: the ONE decoder of the kernel template's parameter slots.
//
// ionode_dopri5_kernel<MODEL, S, G, RT, NT, PD, TAIL> encodes its variant in slots that mean different things per family (the
// kernel names are asserted by tests and recorded in every profile, so the encoding stays):
//   closed-form models   G = 1, RT = trajectories per wavefront (0 -> 64, 16: lanes replicated 4x), NT = PD = 0,
//                        TAIL 0 general / 1 lean (states only) / 2 table (epilogue through v_at_outputs)
//   N <= 16 nets         G = 1, NT = 1; RT slot 64: one trajectory per lane, then PD slot 10: the per-lane net (MlpLane), TAIL 1: lean
//   MLP tiles            G wavefronts, RT row-tile slots per wavefront, NT k-tiles (slot 0: the run-time-width tile), PD ring depth,
//                        TAIL bits: 4 two column sets, 8 lean, 16 four trajectories per tile, 32 one per tile, 64 its deep-stack form
// The kernel, its launch bounds, the launcher and the host's variant table read the NAMES below; nothing else tests a slot.
// Host- and device-constexpr; nothing of HIP's device side is needed here.
#pragma once

#include <type_traits>

#include "../../include/ionode.h"

#ifndef IONODE_LEAN
#define IONODE_LEAN 1   // 0: A/B build without the contract folding of the lean variants
#endif
#ifndef IONODE_T64_WAVES
#define IONODE_T64_WAVES 1
#endif
// Lane-wise kernels: a workgroup carries FOUR independent one-wavefront tiles (see the kernel)
#define IONODE_LW_TILES_PER_WG 4

namespace ionode {

template <int MODEL> struct ModelTraits {
  static constexpr int D = (MODEL == IONODE_MODEL_MARKOV6) ? 6 : 2;
  static constexpr int NPAR = (MODEL == IONODE_MODEL_MARKOV6) ? 12 : 8;
  static constexpr bool MLP = (MODEL == IONODE_MODEL_NNF || MODEL == IONODE_MODEL_NND);
};

// the net structs (ionode_mlp_*.hpp, ionode_rhs.hpp)
template <int G, int RT, int NT, int PD, int NSETS> struct MlpTile;
struct MlpTile4;
template <int MRES_> struct MlpRow1T;
using MlpRow1 = MlpRow1T<2>;       // nets of at most MlpRow1::max_layers() = 6 hidden layers: two steps per row wavefront resident in LDS
using MlpRow1Deep = MlpRow1T<0>;   // deeper stacks: every step streamed
template <int N> struct MlpLane;
struct MlpGen;
struct NoMlp;

enum class Net { None, Tile, Tile4, Row1, Row1Deep, Lane, Gen };
// the contract a variant is compiled under (ionode_capi.hip selects it only when the contract holds):
//   States  lane-wise kernels: uniform protocol grid, VERIFIED uniform output grid, states only, no step log, no checkpoints
//   Table   closed-form kernels: uniform protocol grid, no step log, no checkpoints; the epilogue reads V(t_k) from v_at_outputs
//   Tile    MLP tiles: uniform protocol grid, VERIFIED uniform output grid, no step log, no checkpoints
enum class Lean { General, States, Table, Tile };

template <int MODEL, int G, int RT, int NT, int PD, int TAIL> struct KernelForm {
  static constexpr bool mlp = ModelTraits<MODEL>::MLP;
  // one trajectory per lane: the closed-form models, and the N <= 16 nets at 64 per wavefront
  static constexpr bool t64 = mlp && RT == 64;
  static constexpr bool lane_wise = !mlp || t64;
  // two 16-trajectory column sets per workgroup (MlpTile::NSETS): wavefronts [0, G / 2) integrate set 0, the others set 1
  static constexpr int nsets = (mlp && G > 1 && (TAIL & 4)) ? 2 : 1;
  static constexpr Net net = !mlp                                      ? Net::None
                             : (t64 && PD > 1)                         ? Net::Lane
                             : (G == 4 && NT == 13 && (TAIL & 32))     ? ((TAIL & 64) ? Net::Row1Deep : Net::Row1)
                             : (G == 4 && NT == 13 && (TAIL & 16))     ? Net::Tile4
                             : (G == 4 && NT == 0)                     ? Net::Gen
                                                                       : Net::Tile;
  static constexpr Lean lean = lane_wise ? (TAIL == 1 ? Lean::States : ((!mlp && TAIL == 2) ? Lean::Table : Lean::General))
                                         : ((G > 1 && (TAIL & 8)) ? Lean::Tile : Lean::General);
  // trajectories of a tile (one workgroup; lane-wise kernels: one wavefront), and the lanes of a wavefront that hold distinct ones
  static constexpr int lanes_per_set = !mlp ? (RT > 0 ? RT : 64) : t64 ? 64 : (net == Net::Row1 || net == Net::Row1Deep) ? 1 : net == Net::Tile4 ? 4 : 16;
  static constexpr int traj_per_tile = lanes_per_set * nsets;
  // the variant key of the lane-wise kernels' LDS layout (LwLds): 0 general, 1 lean, 2 table
  static constexpr int lds_key = lean == Lean::States ? 1 : (lean == Lean::Table ? 2 : 0);
  static constexpr int block_threads = 64 * (lane_wise ? IONODE_LW_TILES_PER_WG : G);
  // Wavefronts per SIMD asked of hipcc (__launch_bounds__).  2-state closed-form kernels: TWO -- a 256-register budget, of which hipcc
  // uses 118 (lean variant: FOUR resident per SIMD), 125-131 (table variant) or 150-158 (general: three per SIMD) -- round 4: constants
  // as scalar operands, lane- and parameter-derived invariants kept out of the attempt loop, plain work-list emission; asked for three,
  // hipcc's scheduler fills the 168 and spills 2-6 registers to scratch.  6-state: ONE (the whole register file; the lean variant
  // comes out at 232 -- two resident per SIMD): asked for two, the general variant spilled 48 dwords into scratch inside the stage loop
  // and ran 1.6x (65 536 trajectories) to 2x (16 384) slower.  MLP tiles: 1 per SIMD.
  static constexpr int waves_per_simd = t64 ? IONODE_T64_WAVES : (MODEL == IONODE_MODEL_HH2 ? 2 : 1);
  // the lean N = 200 16-tile finishes on the 4-trajectory net once <= 4 of its trajectories are live (MlpShrink4)
  static constexpr bool shrink = net == Net::Tile && G == 4 && NT == 13 && PD == 13 && TAIL == 8;
  // ... and, given a record workspace, leaves the dense output of its accepted steps to ionode_dense_expand_kernel: a step writes one
  // record (ionode_dense_expand.hpp DenseRecord) instead of evaluating and storing its samples between two evaluations of the net
  static constexpr bool defer = shrink;
  // ... and knows the fused objective's squares alone (KArgs::obj_abs is not read): these four kernels fill the register file -- NN-d
  // fp64 all 512 registers without a spill -- and a flag in their emission, in whatever form, made that one spill 4 to 8 vector
  // registers.  The host sends a sum of absolute residuals on the 16-tile to the general variant (ionode_capi.hip plan_mlp).
  static constexpr bool objective_kinds = !shrink;

  using Tile = MlpTile<G, (t64 ? 1 : (RT > 0 ? RT : 1)), (NT > 0 ? NT : 1), ((PD > 0 && net != Net::Lane) ? PD : 1), nsets>;
  using Mlp = std::conditional_t<net == Net::None, NoMlp,
              std::conditional_t<net == Net::Lane, MlpLane<(net == Net::Lane ? PD : 10)>,
              std::conditional_t<net == Net::Row1, MlpRow1,
              std::conditional_t<net == Net::Row1Deep, MlpRow1Deep,
              std::conditional_t<net == Net::Tile4, MlpTile4,
              std::conditional_t<net == Net::Gen, MlpGen, Tile>>>>>>;

  static_assert(mlp || G == 1, "closed-form models use one wavefront per tile");
  static_assert(!t64 || (G == 1 && NT == 1), "64 trajectories per wavefront is the resident-weights (N <= 16) path");
  static_assert(nsets == 1 || net == Net::Tile, "the 4- and one-trajectory tiles have one column set");
};

}  // namespace ionode
