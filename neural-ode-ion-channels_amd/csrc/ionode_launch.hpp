// ionode_launch.hpp -- host-side table of compiled kernel instantiations.
#pragma once
#include "ionode_device.hpp"

namespace ionode {

using LaunchFn = hipError_t (*)(const KArgs &, unsigned grid, size_t lds, hipStream_t);

// What the planner (ionode_capi.hip) needs to know of a compiled instantiation: the decoded facts of its KernelForm, never the slots.
struct Variant {
  int model, f32;
  int G;               // wavefronts per tile
  int NT;              // k-tiles (16 * NT = padded MLP width); 0: closed-form models and the run-time-width tile
  Net net;
  Lean lean;
  int traj_per_tile;   // trajectories of one tile (a workgroup; lane-wise kernels: a wavefront)
  int lds_key;         // lane-wise kernels: the variant key of their LDS layout (LwLds)
  bool lane_wise, shrink;
  bool defer;          // leaves its dense output to ionode_dense_expand_kernel when given a record workspace (KernelForm::defer)
  size_t (*lds_bytes)(int L, int NT);   // LDS bytes of the variant's net for L hidden layers (NT: the run-time-width tile's k-tiles)
  LaunchFn fn;
  const char *name;  // as rocprofv3 --kernel-trace prints it
};

// the LDS region of a variant's net, from the struct the kernel instantiates
template <typename F> size_t net_lds_bytes(int L, int NT) {
  if constexpr (F::net == Net::None) return 0;
  else if constexpr (F::net == Net::Gen) return F::Mlp::lds_bytes(L, NT);
  else if constexpr (F::net == Net::Tile) return F::Mlp::lds_total(L);   // + the asm stream's scratch slot and input exchange
  else return F::Mlp::lds_bytes(L);
}

template <int MODEL, typename S, int G, int RT, int NT, int PD, int TAIL>
hipError_t launch(const KArgs &a, unsigned grid, size_t lds, hipStream_t s) {
  using F = KernelForm<MODEL, G, RT, NT, PD, TAIL>;
  auto kern = ionode_dopri5_kernel<MODEL, S, G, RT, NT, PD, TAIL>;
  // the lane-wise kernels' LDS region is laid out from the SAME template constants the kernel uses: a plan that reserved less
  // (a host / device layout mismatch) is refused here instead of becoming an out-of-bounds LDS access on the device
  if constexpr (F::lane_wise) {
    const size_t need = (size_t)LwLds::bytes(ModelTraits<MODEL>::D, F::lds_key);
    if ((size_t)a.lw_bytes < need || (a.lw_bytes & 15) || lds < (size_t)IONODE_LW_TILES_PER_WG * (size_t)a.lw_bytes) return hipErrorInvalidValue;
  }
  if (lds > 64 * 1024) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kern),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(kern, dim3(grid), dim3(F::block_threads), lds, s, a);
  return hipGetLastError();
}

template <int MODEL, typename S, int F32, int G, int RT, int NT, int PD, int TAIL>
constexpr Variant make_variant(const char *name) {
  using F = KernelForm<MODEL, G, RT, NT, PD, TAIL>;
  return Variant{MODEL, F32, G, NT, F::net, F::lean, F::traj_per_tile, F::lds_key, F::lane_wise, F::shrink, F::defer, &net_lds_bytes<F>,
                 &launch<MODEL, S, G, RT, NT, PD, TAIL>, name};
}

#define IONODE_VARIANT(MODEL, S, F32, G, RT, NT, PD, TAIL) IONODE_VARIANT_(MODEL, S, F32, G, RT, NT, PD, TAIL)
#define IONODE_VARIANT_(MODEL, S, F32, G, RT, NT, PD, TAIL) \
  make_variant<MODEL, S, F32, G, RT, NT, PD, TAIL>("ionode_dopri5_kernel<" #MODEL ", " #S ", " #G ", " #RT ", " #NT ", " #PD ", " #TAIL ">")
// the MLP shapes of the reference's architectures/s00-s11.py: N = 10, 100, 200, 500
#define IONODE_MLP_VARIANTS(MODEL, S, F32)                                                      \
  IONODE_VARIANT(MODEL, S, F32, 1, 1, 1, 1, 0), IONODE_VARIANT(MODEL, S, F32, 4, 4, 7, 7, 0),        \
      /* N <= 16 at 64 trajectories per wavefront (RT slot 64), general and lean (TAIL 1) */ \
      IONODE_VARIANT(MODEL, S, F32, 1, 64, 1, 1, 0), IONODE_VARIANT(MODEL, S, F32, 1, 64, 1, 1, 1),      \
      /* ... and N = 10 with the net evaluated per lane on the vector ALU (PD slot 10: MlpLane) */      \
      IONODE_VARIANT(MODEL, S, F32, 1, 64, 1, 10, 0), IONODE_VARIANT(MODEL, S, F32, 1, 64, 1, 10, 1),    \
      IONODE_VARIANT(MODEL, S, F32, 4, 4, 13, 13, 0), IONODE_VARIANT(MODEL, S, F32, 4, 8, 32, 4, 0),     \
      /* N = 200 with two column sets per tile (TAIL slot 4: 32 trajectories per workgroup), launches of >= 512 such tiles' worth */ \
      IONODE_VARIANT(MODEL, S, F32, 4, 4, 13, 13, 4),                                                     \
      /* ... and both N = 200 tiles as LEAN variants (TAIL bit 8: uniform protocol grid, verified output grid, no step log / checkpoints) */ \
      IONODE_VARIANT(MODEL, S, F32, 4, 4, 13, 13, 8), IONODE_VARIANT(MODEL, S, F32, 4, 4, 13, 13, 12),    \
      /* N = 200 at FOUR trajectories per tile (TAIL bit 16: MlpTile4, small batches / single calls), general and lean */ \
      IONODE_VARIANT(MODEL, S, F32, 4, 4, 13, 13, 16), IONODE_VARIANT(MODEL, S, F32, 4, 4, 13, 13, 24),   \
      /* N = 200 at ONE trajectory per tile (TAIL bit 32: MlpRow1, the reference's own odeint(func, y0, t) call shape), general and lean */ \
      IONODE_VARIANT(MODEL, S, F32, 4, 4, 13, 13, 32), IONODE_VARIANT(MODEL, S, F32, 4, 4, 13, 13, 40),   \
      /* ... and for stacks of 7 .. 15 hidden layers without LDS-resident steps (TAIL bit 64: MlpRow1Deep) */ \
      IONODE_VARIANT(MODEL, S, F32, 4, 4, 13, 13, 96), IONODE_VARIANT(MODEL, S, F32, 4, 4, 13, 13, 104),  \
      /* lean variants of the N = 100 and N = 500 tiles */                                              \
      IONODE_VARIANT(MODEL, S, F32, 4, 4, 7, 7, 8), IONODE_VARIANT(MODEL, S, F32, 4, 8, 32, 4, 8),        \
      /* any other width up to 512 (NT slot 0: MlpGen, the k-tile count is a run-time value), general and lean */ \
      IONODE_VARIANT(MODEL, S, F32, 4, 1, 0, 1, 0), IONODE_VARIANT(MODEL, S, F32, 4, 1, 0, 1, 8)

// one table per translation unit (they compile in parallel)
const Variant *variants_closed(int *n);
const Variant *variants_nnf_f64(int *n);
const Variant *variants_nnf_f32(int *n);
const Variant *variants_nnd_f64(int *n);
const Variant *variants_nnd_f32(int *n);

}  // namespace ionode
