// ionode_expfit.hpp -- the curve-fit objective of the real-data route (include/ionode.h "Multi-exponential fits"): the RMSE of a
// tri- or bi-exponential against the samples of one constant-voltage segment, one value per row of a CMA-ES trial tensor, and the
// fitted curve with its first and second time derivative on a segment's full grid.  The functions below are shared WORD FOR WORD by
// the gfx950 kernels (inst_expfit.hip) and the host mirrors (ionode_multi_exp_objective_host, ionode_multi_exp_eval_host).
//
// Reference: train-r1.py:427-451 (tri_exp / bi_exp and their derivatives), :487-494 (f = sqrt(mean((model - a)^2)) minimised per
// segment), :553-555 / :641 (the segments handed to PINTS' CMA-ES).  x = (A_1, b_1, ..., A_NT, b_NT, c), NT = 3 or 2:
//   m(t) = ((A_1 e_1 + A_2 e_2) + A_3 e_3) + c,  e_j = lm_exp((-b_j) t)
// summed from the first term, the offset last (preprocess.multi_exp's order).
//
// Execution model of the objective: ONE 256-LANE WORKGROUP PER ROW of the trial tensor.  Lane l sums the squared residuals of the
// samples k = l, l + 256, l + 512, ... in ascending order (ef_lane_sum).  The 256 partial sums are combined in one written order:
// inside each of the four wavefronts an xor-butterfly, v_l <- v_l + v_(l xor s) for s = 32, 16, 8, 4, 2, 1 (an addition is
// commutative, so after each stage both partners hold the same bits and after the last all 64 lanes hold the wavefront's sum w);
// then (w_0 + w_1) + (w_2 + w_3) through LDS.  value = sqrt(sum / n).  No atomics, no scratch; the host mirror walks the same lanes
// and the same butterfly on an array (ef_row_host).
//
// Bit-for-bit agreement of the two builds is a property of this file, as it is for the step units: -ffp-contract=off -fno-fast-math
// on both passes, fp64 + - * / and sqrt correctly rounded on both, fma only inside lm_exp, no libm / ocml call.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ionode.h"
#include "ionode_step_math.hpp"

namespace ionode {

constexpr int kEfLanes = 256;        // lanes of an objective workgroup: four wavefronts
constexpr int kEfEvalChunks = 32;    // workgroups striding over one segment's full grid in the eval kernel

struct EfArgs {
  int32_t n_run, n_active, lam, npar;
  const int32_t *active;       // [n_active] or NULL (slot s is run s)
  const int32_t *seg_of_run;   // [n_run]
  const int64_t *seg_off;      // [segments + 1]
  const double *t_rel, *a;     // [seg_off[segments]]
  const double *trial;         // [n_active * lam][npar]
  double *value;               // [n_active * lam]
  int32_t *status;             // [n_active * lam]
};

struct EfEvalArgs {
  int32_t n_seg, npar;
  const double *x;             // [n_seg][npar]
  const int64_t *full_off;     // [n_seg + 1]
  const double *t_full;        // [full_off[n_seg]]
  double *a_fit, *dadt, *d2adt2;
};

// m(t): the terms in index order, the offset last
template <int NT>
__host__ __device__ inline double ef_model(const double (&x)[2 * NT + 1], double t) {
  double m = x[0] * lm_exp((-x[1]) * t);
#pragma unroll
  for (int j = 1; j < NT; ++j) m = m + x[2 * j] * lm_exp((-x[2 * j + 1]) * t);
  return m + x[2 * NT];
}

// lane `lane`'s partial sum of squared residuals over the n samples at t / a: k = lane, lane + 256, ... ascending
template <int NT>
__host__ __device__ inline double ef_lane_sum(const double (&x)[2 * NT + 1], const double *t, const double *a, int64_t n, int lane) {
  double s = 0.0;
  for (int64_t k = lane; k < n; k += kEfLanes) {
    const double r = ef_model<NT>(x, t[k]) - a[k];
    s = s + r * r;
  }
  return s;
}

// what row `row` fits: its run's segment as (first sample, samples); false when the slot names no run (nothing of the row is touched)
__host__ __device__ inline bool ef_row_segment(const EfArgs &g, int64_t row, int64_t &first, int64_t &n) {
  const int slot = (int)(row / g.lam);
  const int c = g.active ? g.active[slot] : slot;
  if (c < 0 || c >= g.n_run) return false;
  const int seg = g.seg_of_run[c];
  first = 0;
  n = 0;
  if (seg < 0) return true;   // (no segment: an empty one)
  first = g.seg_off[seg];
  n = g.seg_off[seg + 1] - first;
  return true;
}

template <int NT>
__host__ __device__ inline void ef_load_row(const EfArgs &g, int64_t row, double (&x)[2 * NT + 1]) {
#pragma unroll
  for (int i = 0; i < 2 * NT + 1; ++i) x[i] = g.trial[row * (2 * NT + 1) + i];
}

__host__ __device__ inline double ef_rmse(double w0, double w1, double w2, double w3, int64_t n) {
  return __builtin_sqrt(((w0 + w1) + (w2 + w3)) / (double)n);
}

template <int NT>
__global__ void __launch_bounds__(kEfLanes) ionode_multi_exp_objective_kernel(const EfArgs g) {
  __shared__ double w[kEfLanes / 64];
  const int64_t row = blockIdx.x;
  const int lane = threadIdx.x;
  int64_t first, n;
  if (!ef_row_segment(g, row, first, n)) return;   // (uniform over the workgroup)
  if (n <= 0) {
    if (lane == 0) {
      g.value[row] = lm_inf();
      g.status[row] = 1;
    }
    return;
  }
  double x[2 * NT + 1];
  ef_load_row<NT>(g, row, x);
  double v = ef_lane_sum<NT>(x, g.t_rel + first, g.a + first, n, lane);
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) v = v + __shfl_xor(v, s, 64);
  if ((lane & 63) == 0) w[lane >> 6] = v;
  __syncthreads();
  if (lane == 0) {
    g.value[row] = ef_rmse(w[0], w[1], w[2], w[3], n);
    g.status[row] = 0;
  }
}

// the same row on the host: the 256 lanes one after the other, the butterfly on an array
template <int NT>
inline void ef_row_host(const EfArgs &g, int64_t row) {
  int64_t first, n;
  if (!ef_row_segment(g, row, first, n)) return;
  if (n <= 0) {
    g.value[row] = lm_inf();
    g.status[row] = 1;
    return;
  }
  double x[2 * NT + 1];
  ef_load_row<NT>(g, row, x);
  double w[kEfLanes / 64];
  for (int wave = 0; wave < kEfLanes / 64; ++wave) {
    double v[64], u[64];
    for (int l = 0; l < 64; ++l) v[l] = ef_lane_sum<NT>(x, g.t_rel + first, g.a + first, n, 64 * wave + l);
    for (int s = 32; s >= 1; s >>= 1) {
      for (int l = 0; l < 64; ++l) u[l] = v[l] + v[l ^ s];
      for (int l = 0; l < 64; ++l) v[l] = u[l];
    }
    w[wave] = v[0];
  }
  g.value[row] = ef_rmse(w[0], w[1], w[2], w[3], n);
  g.status[row] = 0;
}

// sample k of segment `seg`'s full grid: the curve and its derivatives.  The term of order q is ((-b_j)^q A_j) e_j with the
// coefficient formed first ((-b)^2 written b b), the sum starts from the first term, the offset enters the curve only.
template <int NT>
__host__ __device__ inline void ef_eval_sample(const EfEvalArgs &g, int seg, int64_t k) {
  const double *x = g.x + (size_t)seg * (2 * NT + 1);
  const double t = g.t_full[k];
  double m = 0.0, d1 = 0.0, d2 = 0.0;
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    const double A = x[2 * j], b = x[2 * j + 1];
    const double e = lm_exp((-b) * t);
    const double t0 = A * e, t1 = ((-b) * A) * e, t2 = ((b * b) * A) * e;
    m = j == 0 ? t0 : m + t0;
    d1 = j == 0 ? t1 : d1 + t1;
    d2 = j == 0 ? t2 : d2 + t2;
  }
  g.a_fit[k] = m + x[2 * NT];
  g.dadt[k] = d1;
  g.d2adt2[k] = d2;
}

// one lane per sample: workgroup (seg, chunk) strides over the segment's grid with its kEfEvalChunks - 1 siblings
template <int NT>
__global__ void __launch_bounds__(kEfLanes) ionode_multi_exp_eval_kernel(const EfEvalArgs g) {
  const int seg = blockIdx.x;
  const int64_t first = g.full_off[seg], end = g.full_off[seg + 1];
  for (int64_t k = first + (int64_t)blockIdx.y * kEfLanes + threadIdx.x; k < end; k += (int64_t)kEfEvalChunks * kEfLanes)
    ef_eval_sample<NT>(g, seg, k);
}

template <int NT>
inline void ef_eval_host(const EfEvalArgs &g) {
  for (int seg = 0; seg < g.n_seg; ++seg)
    for (int64_t k = g.full_off[seg]; k < g.full_off[seg + 1]; ++k) ef_eval_sample<NT>(g, seg, k);
}

// inst_expfit.hip
void launch_multi_exp_objective(const EfArgs &g, hipStream_t s);
void multi_exp_objective_host(const EfArgs &g);
void launch_multi_exp_eval(const EfEvalArgs &g, hipStream_t s);
void multi_exp_eval_host(const EfEvalArgs &g);

}  // namespace ionode
