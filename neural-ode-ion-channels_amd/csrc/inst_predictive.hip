// Posterior predictive bands (ionode_predictive.hpp): the accumulate pass with its count launch, the quantile kernel for every sort
// length 2^1 .. 2^14, and the host mirrors -- the same element routines, looped over the elements in the written order.  A unit of
// its own, compiled with the Levenberg-Marquardt step's flags (Makefile), so that every other unit compiles to the code it had.
#include <algorithm>
#include <vector>

#include "ionode_predictive.hpp"
namespace ionode {

int pr_sort_log2(int s_cap) {
  int L = 1;
  while ((1 << L) < s_cap) ++L;
  return L;
}

__global__ void __launch_bounds__(64) ionode_predictive_count_kernel(const PrArgs a) {
  const int p = blockIdx.x * 64 + threadIdx.x;
  if (p < a.P) pr_count(a, p);
}

void launch_predictive_accumulate(const PrArgs &a, hipStream_t s) {
  const dim3 grid((unsigned)((a.Nt + kPrTileK - 1) / kPrTileK), (unsigned)a.P);
  if (a.cols) hipLaunchKernelGGL((ionode_predictive_accumulate_kernel<true>), grid, dim3(kPrTileK), 0, s, a);
  else hipLaunchKernelGGL((ionode_predictive_accumulate_kernel<false>), grid, dim3(kPrTileK), 0, s, a);
  hipLaunchKernelGGL(ionode_predictive_count_kernel, dim3((unsigned)((a.P + 63) / 64)), dim3(64), 0, s, a);
}

void predictive_accumulate_host(const PrArgs &a) {
  for (int p = 0; p < a.P; ++p) {
    for (int k = 0; k < a.Nt; ++k) {
      const size_t e = (size_t)p * a.Nt + k;
      PrMoments m{a.mean[e], a.m2[e], a.mn[e], a.mx[e], a.count[p]};
      for (int c = 0; c < a.n_draw; ++c) {
        const size_t row = (size_t)c * a.P + p;
        double x = lm_inf();
        if (a.status[row] == 0) {
          x = pr_value(a, a.trace[row * a.Nt + k], a.draw_base + c, p, k);
          pr_welford(m, x);
        }
        if (a.cols) a.cols[e * a.S_cap + a.draw_base + c] = x;
      }
      a.mean[e] = m.mean;
      a.m2[e] = m.m2;
      a.mn[e] = m.mn;
      a.mx[e] = m.mx;
    }
  }
  for (int p = 0; p < a.P; ++p) pr_count(a, p);
}

template <int L> static void launch_q(const PrQuantArgs &a, hipStream_t s) {
  const int half = (1 << L) / 2;
  const int threads = half < 64 ? 64 : (half > 1024 ? 1024 : half);
  hipLaunchKernelGGL((ionode_predictive_quantiles_kernel<L>), dim3((unsigned)(a.P * a.Nt)), dim3(threads), 0, s, a);
}

#define IONODE_PREDICTIVE_EACH_L(X) X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8) X(9) X(10) X(11) X(12) X(13) X(14)
void launch_predictive_quantiles(const PrQuantArgs &a, hipStream_t s) {
  switch (pr_sort_log2(a.S_cap)) {
#define X(l) case l: launch_q<l>(a, s); break;
    IONODE_PREDICTIVE_EACH_L(X)
#undef X
  }
}

void predictive_quantiles_host(const PrQuantArgs &a) {
  std::vector<uint64_t> keys((size_t)a.S_cap);
  for (int p = 0; p < a.P; ++p) {
    const int64_t m = a.count[p] < a.S_cap ? a.count[p] : (int64_t)a.S_cap;
    for (int k = 0; k < a.Nt; ++k) {
      const double *src = a.cols + ((size_t)p * a.Nt + k) * a.S_cap;
      for (int i = 0; i < a.S_cap; ++i) keys[i] = pr_key(src[i]);
      std::sort(keys.begin(), keys.end());   // (a total order on the keys: every correct sort gives the kernel's sequence)
      for (int qi = 0; qi < a.Q; ++qi) a.quant[((size_t)p * a.Q + qi) * a.Nt + k] = pr_quantile(keys, m, a.q[qi]);
    }
  }
}

}  // namespace ionode
