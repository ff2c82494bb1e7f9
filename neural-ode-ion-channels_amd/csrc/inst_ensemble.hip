// Affine-invariant ensemble step (ionode_ensemble.hpp): the kernel for every number of coordinates 1 .. 13 -- one workgroup per
// ensemble -- and the host mirror: the same en_ensemble<N>, run as one lane, looped over the ensembles.  A unit of its own, compiled
// with the Levenberg-Marquardt step's flags (Makefile), so that every other unit compiles to the code it had.
#include "ionode_ensemble.hpp"
namespace ionode {
template <int N> static void launch(const EnArgs &a, hipStream_t s) {
  hipLaunchKernelGGL((ionode_ensemble_step_kernel<N>), dim3((unsigned)a.E), dim3(kEnLanes), 0, s, a);
}
template <int N> static void host(const EnArgs &a) {
  int bad = 0;
  for (int e = 0; e < a.E; ++e) en_ensemble<N>(a, e, 0, 1, &bad);
}
#define IONODE_ENSEMBLE_EACH_N(X) X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8) X(9) X(10) X(11) X(12) X(13)
void launch_ensemble_step(const EnArgs &a, hipStream_t s) {
  switch (a.n) {
#define X(n) case n: launch<n>(a, s); break;
    IONODE_ENSEMBLE_EACH_N(X)
#undef X
  }
}
void ensemble_step_host(const EnArgs &a) {
  switch (a.n) {
#define X(n) case n: host<n>(a); break;
    IONODE_ENSEMBLE_EACH_N(X)
#undef X
  }
}
}  // namespace ionode
