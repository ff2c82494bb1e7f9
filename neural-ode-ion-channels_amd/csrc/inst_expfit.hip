// Multi-exponential fit objective and evaluation (ionode_expfit.hpp): the kernels for the tri- and the bi-exponential -- one 256-lane
// workgroup per trial row, one lane per sample of a full grid -- and the host mirrors: the same functions, lane after lane.  A unit of
// its own, compiled with the step units' flags (Makefile), so that every other unit compiles to the code it had.
#include "ionode_expfit.hpp"
// The host mirrors spend their time in lm_exp's fused multiply-adds, which the baseline x86-64 host pass turns into calls of libm's
// fma().  Where the processor has the instruction, a clone of the mirror uses it (resolved when the library is loaded); an fma is
// correctly rounded either way, so the two clones compute the same bits.  flatten: lm_exp is inlined into the clone.
#if defined(__x86_64__) && !defined(__HIP_DEVICE_COMPILE__)
#define IONODE_EF_HOST_MIRROR __attribute__((target_clones("fma", "default"), flatten))
#else
#define IONODE_EF_HOST_MIRROR
#endif
namespace ionode {
void launch_multi_exp_objective(const EfArgs &g, hipStream_t s) {
  const dim3 grid((unsigned)((int64_t)g.n_active * g.lam)), block(kEfLanes);
  if (g.npar == 7) hipLaunchKernelGGL((ionode_multi_exp_objective_kernel<3>), grid, block, 0, s, g);
  else hipLaunchKernelGGL((ionode_multi_exp_objective_kernel<2>), grid, block, 0, s, g);
}
IONODE_EF_HOST_MIRROR void multi_exp_objective_host(const EfArgs &g) {
  const int64_t rows = (int64_t)g.n_active * g.lam;
  for (int64_t row = 0; row < rows; ++row) {
    if (g.npar == 7) ef_row_host<3>(g, row);
    else ef_row_host<2>(g, row);
  }
}
void launch_multi_exp_eval(const EfEvalArgs &g, hipStream_t s) {
  const dim3 grid((unsigned)g.n_seg, kEfEvalChunks), block(kEfLanes);
  if (g.npar == 7) hipLaunchKernelGGL((ionode_multi_exp_eval_kernel<3>), grid, block, 0, s, g);
  else hipLaunchKernelGGL((ionode_multi_exp_eval_kernel<2>), grid, block, 0, s, g);
}
IONODE_EF_HOST_MIRROR void multi_exp_eval_host(const EfEvalArgs &g) {
  if (g.npar == 7) ef_eval_host<3>(g);
  else ef_eval_host<2>(g);
}
}  // namespace ionode
