// Training through the solve (ionode_train.hpp): the three kernels of the update -- gradient cast with its norm partials, the guarded
// and clipped Adam step, the refresh of both weight images -- and the host mirrors: the same functions, lane after lane.  A unit of its
// own, compiled with the step units' flags (Makefile), so that every other unit compiles to the code it had.
#define IONODE_TRAIN_KERNELS
#include "ionode_train.hpp"
namespace ionode {
void launch_train_grad_norm(const TrNormArgs &g, hipStream_t s) {
  hipLaunchKernelGGL(ionode_train_grad_norm_kernel, dim3((unsigned)((g.n + kTrChunk - 1) / kTrChunk)), dim3(kTrLanes), 0, s, g);
}
void train_grad_norm_host(const TrNormArgs &g) {
  for (int wg = 0; wg < (g.n + kTrChunk - 1) / kTrChunk; ++wg) tr_norm_wg_host(g, wg);
}
void launch_train_apply(const TrApplyArgs &g, hipStream_t s) {
  hipLaunchKernelGGL(ionode_train_apply_kernel, dim3((unsigned)((g.n + kTrLanes - 1) / kTrLanes)), dim3(kTrLanes), 0, s, g);
}
void train_apply_host(const TrApplyArgs &g) { tr_apply_host(g); }
void launch_train_refresh(const TrRefreshArgs &g, hipStream_t s) {
  hipLaunchKernelGGL(ionode_train_refresh_kernel, dim3((unsigned)((g.n_fwd + g.n_grad + kTrLanes - 1) / kTrLanes)), dim3(kTrLanes), 0, s, g);
}
void train_refresh_host(const TrRefreshArgs &g) { tr_refresh_host(g); }
}  // namespace ionode
