// The run-time-width regression kernels (GradMlpGen, ionode_regress_gen_kernel, ionode_grad_reduce_gen_kernel) in a unit of their own:
// the tuned units compile to the code they compiled to before (same flags: the Makefile's GRADFLAGS; no scratch:
// tests/test_kernel_resources.py).
#define IONODE_GRAD_TEMPLATES_ONLY
#include "ionode_grad_gen.hpp"
