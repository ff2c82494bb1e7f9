// ionode_grad_gen_plan.hpp -- host side of the run-time-width regression kernels (ionode_grad_gen.hpp): which (L, N) they serve, their
// LDS and workgroup plans, and the launchers that inst_grad_gen.hip defines.  It declares no device code of its own (it includes the
// gradient headers for for_width, RArgs and the layouts, as ionode_grad_capi.hip does anyway).
#pragma once

#include <cstdlib>

#include "ionode_regress.hpp"

namespace ionode {

constexpr size_t GRAD_LDS_LIMIT = (size_t)160 * 1024;   // one compute unit's LDS (gfx950)
constexpr int GRAD_MAX_LAYERS = 15;                      // GradMlp::MAXL: sign words for layers 0..15

// GradMlpGen's LDS: GradMlp's budget (grad_lds_bytes) without the contiguous copy of the input layer's second column --
// two activation buffers + two gradient buffers + the remainder tiles' partial sums (ping-pong) + {b0, w00, w01, 0} rows | biases, output weights | fp64 scratch
__host__ __device__ constexpr size_t grad_gen_lds_bytes(int L, int NT) {
  return ((size_t)4 * NT * 64 + (size_t)2 * (NT % 4) * 4 * 64 + 16 * NT) * 16 + ((size_t)L * 16 * NT + 16 * NT + 4) * 4 + 16 * 10 * 8;
}
// the regress kernel's launch bound; what is resident is decided by the LDS of the shape
constexpr int GRAD_GEN_WG_PER_CU = 4;
inline int grad_gen_wg_per_cu(int L, int NT) {
  const size_t n = GRAD_LDS_LIMIT / grad_gen_lds_bytes(L, NT);
  return n < 1 ? 1 : (n > (size_t)GRAD_GEN_WG_PER_CU ? GRAD_GEN_WG_PER_CU : (int)n);
}

// run-time-width reduce kernel: a heavy job is (layer, column block of CB column tiles, row block of RB row tiles); its register tile is
// RB / 4 row tiles x CB column tiles per wavefront (128 accumulator registers), whatever NT is
constexpr int GRAD_GEN_RB = 16, GRAD_GEN_CB = 8;
constexpr int GRAD_GEN_REDUCE_WG_PER_CU = 2;
__host__ __device__ constexpr int grad_gen_reduce_nrb(int NT) { return (NT + GRAD_GEN_RB - 1) / GRAD_GEN_RB; }
__host__ __device__ constexpr int grad_gen_reduce_ncb(int NT) { return (NT + GRAD_GEN_CB - 1) / GRAD_GEN_CB; }
__host__ __device__ constexpr size_t grad_gen_reduce_lds_bytes() { return (size_t)2 * (GRAD_GEN_RB + GRAD_GEN_CB) * 64 * 16 + 128; }   // tile buffers + the staged seeds
// slabs that make ONE round of workgroups on `cus` compute units; at least four records per slab (grad_reduce_slabs' rule)
inline int grad_gen_reduce_slabs(int L, int NT, int cus, int64_t n_records) {
  const int64_t slots = (int64_t)cus * GRAD_GEN_REDUCE_WG_PER_CU;
  const int64_t per_slab = (int64_t)L * grad_gen_reduce_ncb(NT) * grad_gen_reduce_nrb(NT) + 1;
  int64_t n = slots / per_slab;
  if (n > n_records / 4) n = n_records / 4;
  return n < 1 ? 1 : (int)n;
}

// IONODE_GRAD_GENERIC=1 (read on every call): the run-time-width kernels at EVERY width -- the A/B switch against the tuned ones
inline bool grad_generic_forced() {
  const char *e = getenv("IONODE_GRAD_GENERIC");
  return e && e[0] && !(e[0] == '0' && !e[1]);
}
// true: the run-time-width kernels run for this width (no tuned instantiation, or forced)
inline bool grad_use_gen(int NT) { return grad_generic_forced() || !for_width(NT, [](auto) {}, [] {}); }

// inst_grad_gen.hip
void launch_regress_gen(const RArgs &a, unsigned grid, hipStream_t s);
hipError_t launch_grad_reduce_gen(int L, int NT, const float *records, int64_t n_records, int n_slabs, float *partials, hipStream_t s,
                                  int unit_seed);

}  // namespace ionode
