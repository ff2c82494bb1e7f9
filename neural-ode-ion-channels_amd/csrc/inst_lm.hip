// Levenberg-Marquardt step of a population (ionode_lm.hpp): the kernel for every number of free parameters 1 .. 12, and the host
// mirror -- the same lm_candidate<NF>, looped over the slots.  A unit of its own, compiled with the closed-form kernels' flags
// (Makefile), so that every other unit compiles to the code it had.
#include "ionode_lm.hpp"
namespace ionode {
template <int NF> static void launch(const LmArgs &a, hipStream_t s) {
  hipLaunchKernelGGL((ionode_lm_step_kernel<NF>), dim3((unsigned)((a.n_active + 63) / 64)), dim3(64), 0, s, a);
}
template <int NF> static void host(const LmArgs &a) {
  for (int slot = 0; slot < a.n_active; ++slot) lm_candidate<NF>(a, slot);
}
#define IONODE_LM_EACH_NF(X) X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8) X(9) X(10) X(11) X(12)
void launch_lm_step(const LmArgs &a, hipStream_t s) {
  switch (a.nf) {
#define X(n) case n: launch<n>(a, s); break;
    IONODE_LM_EACH_NF(X)
#undef X
  }
}
void lm_step_host(const LmArgs &a) {
  switch (a.nf) {
#define X(n) case n: host<n>(a); break;
    IONODE_LM_EACH_NF(X)
#undef X
  }
}
}  // namespace ionode
