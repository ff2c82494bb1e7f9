// ionode_grad_launch.hpp -- launchers of the backward sweep, shared by the translation units that instantiate it
// (ionode_grad_capi.hip: N = 10 / 100 / 200; inst_grad32.hip: N = 500).
#pragma once
#include "ionode_grad.hpp"
#include "ionode_grad_gc.hpp"
#include "ionode_regress.hpp"

namespace ionode {

__host__ __device__ constexpr size_t grad_walk_lds_bytes() { return (size_t)16 * GRAD_PACKET * 8; }   // the step's 16 packets

// the one-phase sweep (everything inside the walk); closed-form models: NT = 1 and grad_closed_lds_bytes
template <int MODEL, typename S, int NT>
void launch_sweep(const GArgs &a, unsigned grid, size_t lds, hipStream_t s) {
  auto kern = ionode_dopri5_backward_kernel<MODEL, S, NT>;
  raise_lds_limit(kern, lds);
  hipLaunchKernelGGL(kern, dim3(grid), dim3(256), lds, s, a);
}
// phase A of the two-phase sweep: every (tile, step) of the chunk at once
template <int MODEL, typename S, int NT>
void launch_recompute(const GArgs &a, unsigned grid, size_t lds, hipStream_t s) {
  auto kern = ionode_grad_recompute_kernel<MODEL, S, NT>;
  raise_lds_limit(kern, lds);
  const unsigned nb = (unsigned)((a.it_end - a.it_begin + GRAD_RECOMPUTE_IB - 1) / GRAD_RECOMPUTE_IB);
  hipLaunchKernelGGL(kern, dim3(grid, nb), dim3(256), lds, s, a);
}
// phase B: one wavefront per tile, whatever the width (`lds` is the sweep's and unused)
template <int MODEL, typename S>
void launch_walk(const GArgs &a, unsigned grid, size_t, hipStream_t s) {
  hipLaunchKernelGGL((ionode_grad_walk_kernel<MODEL, S>), dim3(grid), dim3(64), grad_walk_lds_bytes(), s, a);
}
// the fused sum-of-squares sweep of the closed-form models (ionode_dopri5_backward_sse)
template <int MODEL, typename S>
void launch_sweep_sse(const GArgs &a, unsigned grid, size_t lds, hipStream_t s) {
  hipLaunchKernelGGL((ionode_dopri5_backward_sse_kernel<MODEL, S>), dim3(grid), dim3(256), lds, s, a);
}
// G_c and the sample-0 term of the fused objective for the two-phase sweep (NN-f / NN-d): one wavefront per (trajectory, iteration);
// grid.y = ceil(iterations / 4) <= 65535 for every chunk the recompute kernel accepts.  `grid` (tiles) and `lds` are unused.
template <typename S>
void launch_sse_gc(const GArgs &a, unsigned, size_t, hipStream_t s) {
  const unsigned nb = (unsigned)((a.it_end - a.it_begin + GRAD_GC_WAVES - 1) / GRAD_GC_WAVES);
  hipLaunchKernelGGL((ionode_grad_sse_gc_kernel<S>), dim3((unsigned)a.k.B, nb), dim3(64 * GRAD_GC_WAVES), 0, s, a);
}

using SweepFn = void (*)(const GArgs &, unsigned grid, size_t lds, hipStream_t);
enum class Sweep { OnePhase, Recompute, Walk, ClosedSse, SseGc };   // the launchers above, in their order

// the launcher of an NN model's one-phase sweep or recompute kernel at width NT (the walk has no width: ionode_grad_capi.hip picks it)
template <int MODEL, typename S, int NT> SweepFn pick_sweep(bool recompute) {
  return recompute ? &launch_recompute<MODEL, S, NT> : &launch_sweep<MODEL, S, NT>;
}
template <int NT> SweepFn pick_sweep(bool recompute, int model, int f32) {
  if (model == IONODE_MODEL_NNF) return f32 ? pick_sweep<IONODE_MODEL_NNF, float, NT>(recompute) : pick_sweep<IONODE_MODEL_NNF, double, NT>(recompute);
  return f32 ? pick_sweep<IONODE_MODEL_NND, float, NT>(recompute) : pick_sweep<IONODE_MODEL_NND, double, NT>(recompute);
}

// inst_grad32.hip
SweepFn pick_sweep32(bool recompute, int model, int f32);
void launch_regress32(const RArgs &a, unsigned grid, hipStream_t s);

}  // namespace ionode
