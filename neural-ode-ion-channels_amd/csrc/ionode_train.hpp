// ionode_train.hpp -- the update of training THROUGH the solve (include/ionode.h "Training through the solve"): the three launches
// that follow grad._sweep in an iteration of train.ThroughSolve, and their host mirrors.  The functions below are shared WORD FOR WORD
// by the gfx950 kernels (inst_train.hip) and the mirrors (ionode_train_*_host).
//
//   ionode_train_grad_norm_kernel   grad[i] = (float)acc[padmap[i]] (the cast of grad._backward) and one fp64 partial of sum grad[i]^2
//                                   per workgroup of kTrLanes lanes x kTrPerLane elements: the grid is ceil(n / kTrChunk), a function of n
//   ionode_train_apply_kernel       every workgroup folds the partials in index order, decides the step from them, the loss and the
//                                   state block it READS (state_in), and runs torch.optim.Adam on its elements; workgroup 0 writes the
//                                   state block of the next call (state_out != state_in: no workgroup reads what another writes)
//   ionode_train_refresh_kernel     forward image and grad image of the updated weights from their index maps, one launch
//
// Bit-for-bit agreement of the two builds is a property of this file, as it is for the step units: -ffp-contract=off -fno-fast-math
// on both passes, fp32 and fp64 + - * / and sqrt correctly rounded on both, no fma, no libm / ocml call, every sum in one written order.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ionode.h"
#include "ionode_step_math.hpp"

namespace ionode {

constexpr int kTrLanes = 256;                       // lanes of a workgroup: four wavefronts
constexpr int kTrPerLane = 16;                      // elements a lane of the norm kernel sums: i = base + lane, + 256, ...
constexpr int kTrChunk = kTrLanes * kTrPerLane;     // elements per norm partial

struct TrNormArgs {
  int32_t n;
  int64_t n_acc;             // doubles of acc: ionode_grad_partial_floats()
  const double *acc;         // padded partial gradient
  const int32_t *padmap;     // [n] flat index -> padded index
  float *grad;               // [n]
  double *norm_part;         // [ceil(n / kTrChunk)]
};

struct TrApplyArgs {
  int32_t n, n_part;
  const float *grad;         // [n]
  const double *norm_part;   // [n_part]
  const double *loss;        // [1]
  const double *state_in;    // [IONODE_TRAIN_STATE_DOUBLES]
  double *state_out;         // [IONODE_TRAIN_STATE_DOUBLES], another block than state_in
  float *w, *m, *v;          // [n]
  float lr, eps;
  double beta1, beta2;       // the products advance by these; the element-wise operations use their fp32 roundings
  double max_norm;
};

struct TrRefreshArgs {
  int32_t n;
  int64_t n_fwd, n_grad;     // floats of the two images (n_grad = 0: no grad image)
  const int32_t *fwd_map, *grad_map;
  const float *w;
  float *fwd_image, *grad_image;
};

// lane `lane` of workgroup `wg`: the cast of its elements and their squares' sum, ascending
__host__ __device__ inline double tr_lane_sum(const TrNormArgs &g, int wg, int lane) {
  double s = 0.0;
  for (int j = 0; j < kTrPerLane; ++j) {
    const int64_t i = (int64_t)wg * kTrChunk + (int64_t)j * kTrLanes + lane;
    if (i >= g.n) break;
    const int64_t p = g.padmap[i];
    const float x = (p >= 0 && p < g.n_acc) ? (float)g.acc[p] : 0.0f;   // (a map entry that names no word of acc gives 0)
    g.grad[i] = x;
    s = s + (double)x * (double)x;
  }
  return s;
}

#ifdef IONODE_TRAIN_KERNELS   // (inst_train.hip alone defines the kernels; ionode_train_capi.hip reads the rest)
__global__ void __launch_bounds__(kTrLanes) ionode_train_grad_norm_kernel(const TrNormArgs g) {
  __shared__ double w[kTrLanes / 64];
  const int lane = threadIdx.x;
  double v = tr_lane_sum(g, blockIdx.x, lane);
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) v = v + __shfl_xor(v, s, 64);
  if ((lane & 63) == 0) w[lane >> 6] = v;
  __syncthreads();
  if (lane == 0) g.norm_part[blockIdx.x] = (w[0] + w[1]) + (w[2] + w[3]);
}
#endif

// the same workgroup on the host: the 256 lanes one after the other, the butterfly on an array
inline void tr_norm_wg_host(const TrNormArgs &g, int wg) {
  double w[kTrLanes / 64];
  for (int wave = 0; wave < kTrLanes / 64; ++wave) {
    double v[64], u[64];
    for (int l = 0; l < 64; ++l) v[l] = tr_lane_sum(g, wg, 64 * wave + l);
    for (int s = 32; s >= 1; s >>= 1) {
      for (int l = 0; l < 64; ++l) u[l] = v[l] + v[l ^ s];
      for (int l = 0; l < 64; ++l) v[l] = u[l];
    }
    w[wave] = v[0];
  }
  g.norm_part[wg] = (w[0] + w[1]) + (w[2] + w[3]);
}

// What a call decides, from the partials, the loss and the state it reads: the same words in every workgroup and in the mirror.
struct TrDecision {
  bool apply;
  double t, b1p, b2p, skipped, norm, scale;   // the NEXT state's count, products and skipped count; this call's norm and clip scale
  float scale_f, bc1, bc2_sqrt;
};
__host__ __device__ inline TrDecision tr_decide(const TrApplyArgs &g) {
  TrDecision d;
  double ss = 0.0;
  for (int k = 0; k < g.n_part; ++k) ss = ss + g.norm_part[k];
  d.norm = __builtin_sqrt(ss);
  d.apply = lm_finite(d.norm) && lm_finite(g.loss[0]);
  d.t = g.state_in[IONODE_TRAIN_STATE_T];
  d.b1p = g.state_in[IONODE_TRAIN_STATE_BETA1_T];
  d.b2p = g.state_in[IONODE_TRAIN_STATE_BETA2_T];
  d.skipped = g.state_in[IONODE_TRAIN_STATE_SKIPPED];
  d.scale = 1.0;
  if (d.apply) {
    d.t = d.t + 1.0;
    d.b1p = d.b1p * g.beta1;         // one multiplication per applied step: beta^t with no pow
    d.b2p = d.b2p * g.beta2;
    if (g.max_norm > 0.0) {            // torch.nn.utils.clip_grad_norm_: min(1, max_norm / (norm + 1e-6))
      const double c = g.max_norm / (d.norm + 1e-6);
      d.scale = c < 1.0 ? c : 1.0;
    }
  } else {
    d.skipped = d.skipped + 1.0;
    d.scale = 0.0;
  }
  d.scale_f = (float)d.scale;
  d.bc1 = (float)(1.0 - d.b1p);
  d.bc2_sqrt = (float)__builtin_sqrt(1.0 - d.b2p);
  return d;
}

__host__ __device__ inline void tr_write_state(const TrApplyArgs &g, const TrDecision &d) {
  g.state_out[IONODE_TRAIN_STATE_T] = d.t;
  g.state_out[IONODE_TRAIN_STATE_BETA1_T] = d.b1p;
  g.state_out[IONODE_TRAIN_STATE_BETA2_T] = d.b2p;
  g.state_out[IONODE_TRAIN_STATE_SKIPPED] = d.skipped;
  g.state_out[IONODE_TRAIN_STATE_LOSS] = g.loss[0];
  g.state_out[IONODE_TRAIN_STATE_NORM] = d.norm;
  g.state_out[IONODE_TRAIN_STATE_SCALE] = d.scale;
  g.state_out[IONODE_TRAIN_STATE_APPLIED] = d.apply ? 1.0 : 0.0;
}

// torch.optim.Adam on element i with the clipped gradient: ionode_adam_kernel's operations in its order (ionode_regress.hpp)
__host__ __device__ inline void tr_adam_element(const TrApplyArgs &g, const TrDecision &d, int64_t i) {
  const float gi = g.grad[i] * d.scale_f;
  // (the scalars as torch hands them to its fp32 kernels: beta and 1 - beta formed in fp64, each rounded once)
  const float beta2 = (float)g.beta2, omb1 = (float)(1.0 - g.beta1), omb2 = (float)(1.0 - g.beta2);
  float mi = g.m[i], vi = g.v[i];
  mi = mi + (gi - mi) * omb1;
  vi = vi * beta2 + (gi * gi) * omb2;
  const float denom = __builtin_sqrtf(vi) / d.bc2_sqrt + g.eps;
  g.w[i] = g.w[i] - (g.lr / d.bc1) * (mi / denom);
  g.m[i] = mi;
  g.v[i] = vi;
}

#ifdef IONODE_TRAIN_KERNELS   // (inst_train.hip alone defines the kernels; ionode_train_capi.hip reads the rest)
__global__ void __launch_bounds__(kTrLanes) ionode_train_apply_kernel(const TrApplyArgs g) {
  const TrDecision d = tr_decide(g);   // (uniform over the grid: every lane reads the same words)
  if (blockIdx.x == 0 && threadIdx.x == 0) tr_write_state(g, d);
  if (!d.apply) return;
  const int64_t i = (int64_t)blockIdx.x * kTrLanes + threadIdx.x;
  if (i < g.n) tr_adam_element(g, d, i);
}
#endif

inline void tr_apply_host(const TrApplyArgs &g) {
  const TrDecision d = tr_decide(g);
  tr_write_state(g, d);
  if (!d.apply) return;
  for (int64_t i = 0; i < g.n; ++i) tr_adam_element(g, d, i);
}

// One element of an image from its map code: s > 0: w[s - 1]; 0: padding, +0.0f; IONODE_TRAIN_MAP_NEG_ZERO: the -0.0f fill of the
// 4-trajectory and one-trajectory sections; s <= IONODE_TRAIN_MAP_PLUS_ZERO: w[IONODE_TRAIN_MAP_PLUS_ZERO - s] + 0.0f, the scalar
// section's hidden biases.  A code that names no weight gives +0.0f.
__host__ __device__ inline float tr_image_element(int32_t s, const float *w, int32_t n) {
  if (s > 0) return s <= n ? w[s - 1] : 0.0f;
  if (s == 0) return 0.0f;
  if (s == IONODE_TRAIN_MAP_NEG_ZERO) return -0.0f;
  const int64_t idx = (int64_t)IONODE_TRAIN_MAP_PLUS_ZERO - s;
  return idx < n ? w[idx] + 0.0f : 0.0f;
}

__host__ __device__ inline void tr_refresh_element(const TrRefreshArgs &g, int64_t k) {
  if (k < g.n_fwd) g.fwd_image[k] = tr_image_element(g.fwd_map[k], g.w, g.n);
  else g.grad_image[k - g.n_fwd] = tr_image_element(g.grad_map[k - g.n_fwd], g.w, g.n);
}

#ifdef IONODE_TRAIN_KERNELS   // (inst_train.hip alone defines the kernels; ionode_train_capi.hip reads the rest)
__global__ void __launch_bounds__(kTrLanes) ionode_train_refresh_kernel(const TrRefreshArgs g) {
  const int64_t k = (int64_t)blockIdx.x * kTrLanes + threadIdx.x;
  if (k < g.n_fwd + g.n_grad) tr_refresh_element(g, k);
}
#endif

inline void tr_refresh_host(const TrRefreshArgs &g) {
  for (int64_t k = 0; k < g.n_fwd + g.n_grad; ++k) tr_refresh_element(g, k);
}

// inst_train.hip
void launch_train_grad_norm(const TrNormArgs &g, hipStream_t s);
void train_grad_norm_host(const TrNormArgs &g);
void launch_train_apply(const TrApplyArgs &g, hipStream_t s);
void train_apply_host(const TrApplyArgs &g);
void launch_train_refresh(const TrRefreshArgs &g, hipStream_t s);
void train_refresh_host(const TrRefreshArgs &g);

}  // namespace ionode
