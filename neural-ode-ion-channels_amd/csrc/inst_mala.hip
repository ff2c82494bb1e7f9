// Manifold-MALA step of many chains (ionode_mala.hpp): the kernel for every number of coordinates 1 .. 13 -- one lane per launch
// slot -- and the host mirror: the same ma_chain<N>, looped over the slots.  A unit of its own, compiled with the Levenberg-Marquardt
// step's flags (Makefile), so that every other unit compiles to the code it had.
#include "ionode_mala.hpp"
namespace ionode {
template <int N> static void launch(const MaArgs &a, hipStream_t s) {
  hipLaunchKernelGGL((ionode_mala_step_kernel<N>), dim3((unsigned)((a.n_active + 63) / 64)), dim3(64), 0, s, a);
}
template <int N> static void host(const MaArgs &a) {
  for (int slot = 0; slot < a.n_active; ++slot) ma_chain<N>(a, slot);
}
#define IONODE_MALA_EACH_N(X) X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8) X(9) X(10) X(11) X(12) X(13)
void launch_mala_step(const MaArgs &a, hipStream_t s) {
  switch (a.n) {
#define X(n) case n: launch<n>(a, s); break;
    IONODE_MALA_EACH_N(X)
#undef X
  }
}
void mala_step_host(const MaArgs &a) {
  switch (a.n) {
#define X(n) case n: host<n>(a); break;
    IONODE_MALA_EACH_N(X)
#undef X
  }
}
}  // namespace ionode
