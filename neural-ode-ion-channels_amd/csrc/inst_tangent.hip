// Tangent (forward-mode) sweep of the closed-form models (ionode_tangent.hpp): HH 2-state and 6-state Markov, both state dtypes.  A unit
// of its own, compiled with the closed-form kernels' flags (Makefile), so that every other unit compiles to the code it had.
#include "ionode_tangent.hpp"
namespace ionode {
template <int MODEL, typename S> static void launch(const TArgs &a, hipStream_t s) {
  constexpr int TPW = TangentMap<MODEL>::TPW;
  hipLaunchKernelGGL((ionode_tangent_sweep_kernel<MODEL, S>), dim3((unsigned)((a.g.k.B + TPW - 1) / TPW)), dim3(64), 0, s, a);
}
void launch_tangent(int model, int f32, const TArgs &a, hipStream_t s) {
  if (model == IONODE_MODEL_MARKOV6) {
    if (f32) launch<IONODE_MODEL_MARKOV6, float>(a, s); else launch<IONODE_MODEL_MARKOV6, double>(a, s);
  } else {
    if (f32) launch<IONODE_MODEL_HH2, float>(a, s); else launch<IONODE_MODEL_HH2, double>(a, s);
  }
}
}  // namespace ionode
