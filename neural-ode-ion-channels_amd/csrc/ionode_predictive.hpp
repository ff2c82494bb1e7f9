// ionode_predictive.hpp -- posterior predictive bands of the current (include/ionode.h "Posterior predictive bands"): the reduction
// ACROSS trajectories that nothing else here does.  Two passes, both with a host mirror that runs the same __host__ __device__
// element routines (pr_value, pr_welford, pr_key, pr_quantile) in the same order:
//
//   accumulate   one pass over a chunk of current traces [n_draw * P][Nt] (candidate-major: row = draw * P + protocol).  The element
//                (p, k) belongs to ONE lane, which walks the chunk's draws in ascending index with Welford's update
//                    n <- n + 1;  d = x - mean;  mean <- mean + d / n;  m2 <- m2 + d (x - mean);  min, max by "<" and ">"
//                so the moments are a function of the sequence of surviving draws and of nothing else: cutting the draws into other
//                chunks gives the same bits.  A row with status != 0 is skipped (its slot in the column store gets +inf).  With
//                noise the value is x = i + sigma_s z, z = cm_ppnd16(cm_uniform(w0, w1)) of the Philox words of the counter
//                (draw_offset + draw_base + c, p, k, IONODE_PREDICTIVE_TAG): a function of the draw, not of the chunk or the shard.
//   quantiles    exact order statistics of every column of the store cols [P][Nt][S_cap]: the column as order-preserving 64-bit keys
//                (pr_key: the sign-flip transform, a total order with -0 before +0 and +inf after every finite value), sorted, then
//                for each q: h = q (m - 1), lo = floor(h), g = h - lo, value = x_lo + g (x_hi - x_lo), x_hi = x_min(lo + 1, m - 1),
//                m = count[p]; m = 0 gives NaN.  The m survivors are the first m keys: a failed draw's +inf sorts behind them.
//
// The generator's fourth counter word, the "tag".  In use before this file: pair + 65536 * attempt with pair < 7 and
//   attempt 0 .. kCmResamples   CMA-ES (ionode_cmaes.hpp: the resampling attempts of a candidate)
//   attempt 0                   adaptive Metropolis and manifold MALA (the proposal's pairs; their accept word is (.., 1, 0))
//   attempt 0, 1, 2, 3          the ensemble sampler's roles ask, accept, jitter, spread (ionode_ensemble.hpp)
// IONODE_PREDICTIVE_TAG = 0x70720000 = 65536 * 28786: no step's attempt count comes near it.
//
// accumulate, execution model: one 64-lane workgroup per (protocol, 64 consecutive samples); lane l owns sample k0 + l.  The draws go
// by in tiles of 32: the 32 rows' loads are issued together (each a 512-byte coalesced read along k, 16 KiB in flight per wave) into
// the lane's row of an LDS tile [64 k][33] fp64 -- 32 draws and one word of padding --, the lane folds its row in draw order and leaves
// there what the store wants, and the tile is stored along s: lanes 0 .. 31 write the 32 draws of one sample, 256 contiguous bytes of
// cols (four 64-byte segments; whole ones whenever draw_base and S_cap are multiples of 8), lanes 32 .. 63 the next sample's.  The
// chunk's 32 status words sit beside the tile.
//   LDS banks   the tile's row stride is 33 doubles = 66 dwords.  A lane in its own row (dword 66 l + 2 j): stores (ds_write_b64, lane
//               groups of 16 contiguous lanes, bank = dword address mod 32) -- 66 l mod 32 = 2 l runs over all 32 banks in 16 lanes of
//               two dwords each; loads (ds_read_b64, lane groups of 32, bank = dword address mod 64) -- 66 l mod 64 = 2 l, all 64 banks
//               in 32 lanes: both conflict-free.  The store pass's loads: 32 lanes read 32 consecutive doubles = 64 consecutive dwords
//               -- conflict-free.  Unpadded (stride 64 dwords) a lane's own-row accesses would all meet on one pair of banks.
// No atomics, no scratch; count[p] is advanced by a second, one-workgroup launch on the same stream, after the pass that reads it.
//
// quantiles, execution model: one workgroup per column, the keys in LDS (8 * 2^L bytes, 2^L >= S_cap: 128 KiB at the cap of 16 384),
// read contiguously, the tail filled with the largest key (all ones), a bitonic network of L (L + 1) / 2 passes with one barrier each;
// pass (size, stride): lane t takes the pairs i = 2 t - (t & (stride - 1)), i + stride.  Strides of 16 doubles and more are
// conflict-free; the last four passes of every merge (strides 8 .. 1) are 2-way on ds_read_b64.  L is a template argument, so the
// LDS figure is static and stands in the code object's metadata (tests/test_predictive_kernel_resources.py).
#pragma once

#include "ionode_step_math.hpp"

namespace ionode {

constexpr int kPrMaxDraws = IONODE_PREDICTIVE_MAX_DRAWS;
constexpr int kPrMaxQ = IONODE_PREDICTIVE_MAX_Q;
constexpr int kPrMaxLog2 = 14;   // 2^14 = kPrMaxDraws
constexpr int kPrTileK = 64, kPrTileS = 32, kPrTileStride = kPrTileS + 1;

struct PrArgs {
  int32_t P, Nt, n_draw, S_cap, draw_base, draw_offset, noise;
  uint32_t seed_lo, seed_hi;
  double sigma0;           // the one sigma (sigma == NULL)
  const double *trace;     // [n_draw * P][Nt]
  const int32_t *status;   // [n_draw * P]
  const double *sigma;     // [>= draw_base + n_draw] by global draw index, or NULL
  double *mean, *m2, *mn, *mx;   // [P][Nt]
  int64_t *count;          // [P]
  double *cols;            // [P][Nt][S_cap] or NULL
};

struct PrQuantArgs {
  int32_t P, Nt, S_cap, Q;
  double q[kPrMaxQ];
  const int64_t *count;    // [P]
  const double *cols;      // [P][Nt][S_cap]
  double *quant;           // [P][Q][Nt]
};

// ---- the element routines: one text for the kernel and the mirror ----

// order-preserving key of a double: negative numbers have every bit flipped, the others the sign bit set
__host__ __device__ inline uint64_t pr_key(double x) {
  const uint64_t b = __builtin_bit_cast(uint64_t, x);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__host__ __device__ inline double pr_unkey(uint64_t k) {
  return __builtin_bit_cast(double, (k >> 63) ? (k & 0x7FFFFFFFFFFFFFFFull) : ~k);
}
__host__ __device__ constexpr uint64_t pr_pad_key() { return ~0ull; }

// the value of draw (its index among the caller's draws: the slot of cols and of sigma) at (p, k): the trace's, plus sigma z with noise,
// z a function of the draw's index among ALL draws of the run
__host__ __device__ inline double pr_value(const PrArgs &a, double i, int draw, int p, int k) {
  if (!a.noise) return i;
  uint32_t w[4];
  cm_philox((uint32_t)(a.draw_offset + draw), (uint32_t)p, (uint32_t)k, (uint32_t)IONODE_PREDICTIVE_TAG, a.seed_lo, a.seed_hi, w);
  const double z = cm_ppnd16(cm_uniform(w[0], w[1]));
  const double s = a.sigma ? a.sigma[draw] : a.sigma0;
  return i + s * z;
}

struct PrMoments {
  double mean, m2, mn, mx;
  int64_t n;
};

__host__ __device__ inline void pr_welford(PrMoments &m, double x) {
  m.n = m.n + 1;
  const double d = x - m.mean;
  m.mean = m.mean + d / (double)m.n;
  m.m2 = m.m2 + d * (x - m.mean);
  m.mn = x < m.mn ? x : m.mn;
  m.mx = x > m.mx ? x : m.mx;
}

// the q-quantile of the m smallest of sorted keys
template <class Keys>
__host__ __device__ inline double pr_quantile(const Keys &keys, int64_t m, double q) {
  if (m < 1) return __builtin_bit_cast(double, 0x7FF8000000000000ull);
  const double h = q * (double)(m - 1);
  const double fl = __builtin_floor(h);
  const double g = h - fl;
  const int64_t lo = (int64_t)fl;
  const int64_t hi = lo + 1 < m - 1 ? lo + 1 : m - 1;
  const double xlo = pr_unkey(keys[lo]), xhi = pr_unkey(keys[hi]);
  return xlo + g * (xhi - xlo);
}

// ---- accumulate ----

// COLS: with the column store (without it the tile only stages the loads and nothing is stored along s)
template <bool COLS>
__global__ void __launch_bounds__(kPrTileK) ionode_predictive_accumulate_kernel(const PrArgs a) {
  __shared__ double tile[kPrTileK * kPrTileStride];
  __shared__ int32_t failed[kPrTileS];
  const int lane = threadIdx.x, p = blockIdx.y, k0 = blockIdx.x * kPrTileK, k = k0 + lane;
  const bool live = k < a.Nt;
  const size_t e = (size_t)p * a.Nt + (live ? k : 0);
  double *mine = tile + lane * kPrTileStride;
  PrMoments m{0.0, 0.0, 0.0, 0.0, 0};
  if (live) m = PrMoments{a.mean[e], a.m2[e], a.mn[e], a.mx[e], a.count[p]};
  for (int c0 = 0; c0 < a.n_draw; c0 += kPrTileS) {
#pragma unroll
    for (int j = 0; j < kPrTileS; ++j) {   // the tile's loads, all in flight together, into the lane's row of the tile
      const int c = c0 + j;
      mine[j] = (c < a.n_draw && live) ? a.trace[((size_t)c * a.P + p) * a.Nt + k] : 0.0;
    }
    if (lane < kPrTileS) failed[lane] = c0 + lane < a.n_draw ? a.status[(size_t)(c0 + lane) * a.P + p] : 1;
    __syncthreads();
    for (int j = 0; j < kPrTileS; ++j) {   // ... folded in draw order; the row then holds what the store wants
      double x = lm_inf();
      if (failed[j] == 0 && live) {
        x = pr_value(a, mine[j], a.draw_base + c0 + j, p, k);
        pr_welford(m, x);
      }
      mine[j] = x;
    }
    if (COLS) {
      __syncthreads();
      const int s = lane % kPrTileS, c = c0 + s;
#pragma unroll 4
      for (int r = lane / kPrTileS; r < kPrTileK; r += kPrTileK / kPrTileS) {
        if (k0 + r < a.Nt && c < a.n_draw) a.cols[((size_t)p * a.Nt + k0 + r) * a.S_cap + a.draw_base + c] = tile[r * kPrTileStride + s];
      }
    }
    __syncthreads();
  }
  if (live) {
    a.mean[e] = m.mean;
    a.m2[e] = m.m2;
    a.mn[e] = m.mn;
    a.mx[e] = m.mx;
  }
}

// count[p] <- count[p] + the chunk's surviving draws of protocol p: after the pass above, which reads the old count
__host__ __device__ inline void pr_count(const PrArgs &a, int p) {
  int64_t n = a.count[p];
  for (int c = 0; c < a.n_draw; ++c) n = n + (a.status[(size_t)c * a.P + p] == 0 ? 1 : 0);
  a.count[p] = n;
}

// ---- quantiles ----

template <int L>
__global__ void __launch_bounds__(1024) ionode_predictive_quantiles_kernel(const PrQuantArgs a) {
  constexpr int N2 = 1 << L;
  __shared__ uint64_t keys[N2];
  const int col = blockIdx.x, p = col / a.Nt, k = col - p * a.Nt;
  const int t = threadIdx.x, T = blockDim.x;
  const double *src = a.cols + (size_t)col * a.S_cap;
  for (int i = t; i < N2; i += T) keys[i] = i < a.S_cap ? pr_key(src[i]) : pr_pad_key();
  __syncthreads();
  for (int size = 2; size <= N2; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int u = t; u < N2 / 2; u += T) {
        const int i = 2 * u - (u & (stride - 1)), j = i + stride;
        const uint64_t x = keys[i], y = keys[j];
        const bool up = (i & size) == 0;   // (size == N2: always ascending)
        if ((x > y) == up) {
          keys[i] = y;
          keys[j] = x;
        }
      }
      __syncthreads();
    }
  }
  if (t < a.Q) {
    double q = 0.0;
#pragma unroll
    for (int i = 0; i < kPrMaxQ; ++i)   // (constant indices into the by-value arguments)
      if (i == t) q = a.q[i];
    const int64_t m = a.count[p];
    a.quant[((size_t)p * a.Q + t) * a.Nt + k] = pr_quantile(keys, m < a.S_cap ? m : (int64_t)a.S_cap, q);
  }
}

// inst_predictive.hip
int pr_sort_log2(int s_cap);   // L: the smallest with 2^L >= max(s_cap, 2)
void launch_predictive_accumulate(const PrArgs &a, hipStream_t s);
void predictive_accumulate_host(const PrArgs &a);
void launch_predictive_quantiles(const PrQuantArgs &a, hipStream_t s);
void predictive_quantiles_host(const PrQuantArgs &a);

}  // namespace ionode
