// CMA-ES step of many runs (ionode_cmaes.hpp): the kernel for every number of search variables 1 .. 12 -- one 64-lane workgroup per
// launch slot -- and the host mirror: the same cm_run<N>, its phases looped over the lanes.  A unit of its own, compiled with the
// Levenberg-Marquardt step's flags (Makefile), so that every other unit compiles to the code it had.
#include "ionode_cmaes.hpp"
namespace ionode {
template <int N> static void launch(const CmArgs &a, hipStream_t s) {
  hipLaunchKernelGGL((ionode_cmaes_step_kernel<N>), dim3((unsigned)a.n_active), dim3(64), 0, s, a);
}
template <int N> static void host(const CmArgs &a) {
  for (int slot = 0; slot < a.n_active; ++slot) cm_run_host<N>(a, slot);
}
#define IONODE_CMAES_EACH_N(X) X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8) X(9) X(10) X(11) X(12)
void launch_cmaes_step(const CmArgs &a, hipStream_t s) {
  switch (a.n) {
#define X(n) case n: launch<n>(a, s); break;
    IONODE_CMAES_EACH_N(X)
#undef X
  }
}
void cmaes_step_host(const CmArgs &a) {
  switch (a.n) {
#define X(n) case n: host<n>(a); break;
    IONODE_CMAES_EACH_N(X)
#undef X
  }
}
}  // namespace ionode
