// Tangent (forward-mode) walk of NN-f / NN-d over the recompute kernel's packets (ionode_tangent_nn.hpp), both state dtypes.  A unit of its
// own, compiled with inst_tangent.hip's flags (Makefile), so that every other unit compiles to the code it had.
#include "ionode_tangent_nn.hpp"
namespace ionode {
template <int MODEL, typename S> static void launch(const TArgs &a, hipStream_t s) {
  hipLaunchKernelGGL((ionode_tangent_walk_kernel<MODEL, S>), dim3((unsigned)((a.g.k.B + 7) / 8)), dim3(64), 0, s, a);
}
void launch_tangent_nn(int model, int f32, const TArgs &a, hipStream_t s) {
  if (model == IONODE_MODEL_NNF) {
    if (f32) launch<IONODE_MODEL_NNF, float>(a, s); else launch<IONODE_MODEL_NNF, double>(a, s);
  } else {
    if (f32) launch<IONODE_MODEL_NND, float>(a, s); else launch<IONODE_MODEL_NND, double>(a, s);
  }
}
}  // namespace ionode
