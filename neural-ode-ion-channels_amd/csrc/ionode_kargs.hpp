// ionode_kargs.hpp -- the kernel argument block of the integrator and the protocol lookup: what the forward kernels
// (ionode_device.hpp) and the backward sweep (ionode_grad.hpp, which embeds KArgs in its own arguments) share, without the nets.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ionode.h"
#include "ionode_form.hpp"
#include "ionode_math.hpp"

namespace ionode {

struct KArgs {
  const float *mlp;  // packed image (ionode_mlp_pack)
  const double *params;
  const double *prot_v;
  const double *prot_t;
  const int32_t *prot_of_traj;
  const void *y0;
  const double *t_eval;
  void *y_out;
  double *i_out;
  int32_t *status;
  int64_t *stats;
  int32_t B, Nt, P, Np, n_params, L, N, NP, NT;
  int64_t max_steps;   // attempts allowed between two emitted outputs (torchdiffeq's max_num_steps: _advance resets its counter)
  int64_t max_total;   // attempts allowed over the whole solve (runaway bound; the reference uses a 600 s SIGALRM, train-d0.py:309-318)
  double *ckpt;        // optional [B][ckpt_cap][CkptRecord<D>::WIDTH] fp64: one record per ACCEPTED step, for the backward sweep (ionode_grad.hpp)
  int32_t ckpt_cap;
  double prot_t0, prot_dt, v_oob, rtol, atol, obs_g, obs_e;
  double prot_rdt;     // 1.0 / prot_dt, correctly rounded (host division): divisions by prot_dt become div_by()
  double dt_max;       // optional cap on the step size (+inf: none -- torchdiffeq 0.2.1 has no such option)
  int32_t obs_open;
  int32_t obj_abs;     // fused objective, the term a residual adds (ionode_interp.hpp residual_term): 0 = its square, 1 = its absolute value;
                       // wave-uniform.  It sits in what was padding, so every other field keeps its offset
  double *step_log;
  int64_t step_log_cap;
  const double *sse_ref;  // fused objective (hint path): reference currents [P][Nt]; per trajectory sum_k (i_k - ref[prot][k])^2 ...
  double *sse_out;        // ... goes to sse_out[B] (inf for failed trajectories); y_out / i_out may then be NULL: no trace leaves the chip
  double te_t0, te_dt;  // hint: t_eval[k] ~ te_t0 + k*te_dt (te_dt <= 0: no hint).  Only ever a guess; see emit.
  double te_rdt;        // 1 / te_dt (for the guess only)
  int32_t te_exact;     // 1: the caller VERIFIED t_eval[k] == te_t0 + (double)k * te_dt bit for bit (fp64 multiply, then add):
                        // closed-form kernels then form output times arithmetically -- no vector load sits behind their stores
  const double *v_tab;  // optional [P][Nt]: protocol voltage AT the output times (ionode_protocol_at_outputs); the closed-form
                        // kernels' current / objective epilogue then loads V(t_k) instead of re-deriving it per trajectory
  int64_t mlp_stride;   // several weight images (an ensemble / a population of nets): floats between consecutive images ...
  int32_t traj_per_img; // ... and how many consecutive trajectories share one (a multiple of the tile size); 0: one image for all
  int32_t lw_bytes;     // lane-wise kernels: LDS bytes of ONE wavefront's region (a workgroup carries four of them, see the kernel)
  const int32_t *order; // optional launch order (a permutation of 0..B-1): launch slot s integrates trajectory order[s]; every
                        // input and output stays at the trajectory's own index -- only the tiling / lane assignment changes
  int32_t tile_shrink;  // lean N = 200 16-tile: 1 = switch to the 4-trajectory net once <= 4 of the tile's trajectories are live (MlpShrink4)
  // deferred dense output (KernelForm::defer; NULL / 0: every step emits its samples itself), indexed by TRAJECTORY, not by launch slot:
  int32_t *defer_count; // [B] records a trajectory wrote (written with its final scalars) ...
  double *defer_rec;    // ... of [B][defer_cap][DenseRecord<D>::ROW] fp64 (ionode_dense_expand.hpp); a trajectory whose records are
  int32_t defer_cap;    // full emits its later steps inline
  int32_t defer_fill;   // records a trajectory may fill, <= defer_cap (the records' stride stays defer_cap)
  // the solve kernel's tail (ionode_device.hpp): a tile that ends with a finish rank below defer_tail_rank expands its own records on
  // its otherwise idle compute unit and leaves -(records + 1) in defer_count; 0: every tile leaves its records to the follow-up kernel
  int32_t defer_tail_rank;
  int32_t *defer_tail;  // the tail block (the workspace's last record slot, which defer_fill keeps free): [0] tiles that have ended
};

// Uniform protocol grid, in two halves so that a caller can issue the two sample loads of several lookups back to back:
// the sample index (false: t outside the protocol), and the interpolation from the two samples.
__device__ __forceinline__ bool protocol_index(const KArgs &a, double t, int &i);
__device__ __forceinline__ double protocol_from(const KArgs &a, double v_lo, double v_hi, int i, double t);

// interp1d(t, v) (linear) with the reference's out-of-range rule (train-s1.py:218-229, :234-237).
// scipy: i = searchsorted(x, t) [left], clipped to [1, n-1]; y = slope*(t - x[i-1]) + y[i-1].
// Uniform grids find i arithmetically (i = ceil((t - t0)/dt)); explicit grids by bisection.
__device__ __forceinline__ bool protocol_index(const KArgs &a, double t, int &i) {
  // branch-free (selects only): several lookups in a row become one block of arithmetic followed by one block of loads; the
  // index is valid (1 .. n-1) whatever t is, so the sample loads need no guard
  const int n = a.Np;
  const double t_last = a.prot_t0 + (double)(n - 1) * a.prot_dt;
  const bool inr = !(t < a.prot_t0 || t > t_last || t != t);
  const double u = div_by(t - a.prot_t0, a.prot_dt, a.prot_rdt);
  double ci = ceil(u);
  ci = (ci < 1.0) ? 1.0 : ci;
  ci = (ci > (double)(n - 1)) ? (double)(n - 1) : ci;
  i = inr ? (int)ci : 1;
  return inr;
}
__device__ __forceinline__ double protocol_from(const KArgs &a, double v_lo, double v_hi, int i, double t) {
  const double x_lo = a.prot_t0 + (double)(i - 1) * a.prot_dt;
  const double slope = div_by(v_hi - v_lo, a.prot_dt, a.prot_rdt);
  return slope * (t - x_lo) + v_lo;
}

__device__ __forceinline__ bool protocol_v(const KArgs &a, const double *__restrict__ pv, double t, double &v) {
  const int n = a.Np;
  if (a.prot_t != nullptr) {
    const double *__restrict__ x = a.prot_t;
    if (t < x[0] || t > x[n - 1] || t != t) { v = a.v_oob; return false; }
    int lo = 0, hi = n;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (x[mid] < t) lo = mid + 1; else hi = mid;
    }
    const int i = lo < 1 ? 1 : (lo > n - 1 ? n - 1 : lo);
    const double slope = (pv[i] - pv[i - 1]) / (x[i] - x[i - 1]);
    v = slope * (t - x[i - 1]) + pv[i - 1];
    return true;
  }
  int i;
  if (!protocol_index(a, t, i)) { v = a.v_oob; return false; }
  v = protocol_from(a, pv[i - 1], pv[i], i, t);
  return true;
}

}  // namespace ionode
