// N = 500 (architectures s06-s08) backward sweep, recompute and regression kernels: the N = 500 instantiations of the gradient
// templates in a unit of their own, so that they compile beside ionode_grad_capi.hip's (same flags: the Makefile's GRADFLAGS; no
// scratch: tests/test_kernel_resources.py).
#define IONODE_GRAD_TEMPLATES_ONLY
#include "ionode_grad_launch.hpp"
namespace ionode {
SweepFn pick_sweep32(bool recompute, int model, int f32) { return pick_sweep<32>(recompute, model, f32); }
void launch_regress32(const RArgs &a, unsigned grid, hipStream_t s) { launch_regress<32>(a, grid, s); }
}  // namespace ionode
