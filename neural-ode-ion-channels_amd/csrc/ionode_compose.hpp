// ionode_compose.hpp -- shrink-aware tile composition of the lean N = 200 16-tile: which trajectories share a tile
// when the launch has at most one tile per compute unit.
//
// A tile steps its 16 slots in lock step and hands its region to the 4-trajectory net once <= 4 of them are live (MlpShrink4), so
//     T_tile = A5 * 6 e16 + (A1 - A5) * 6 e4        A1, A5: largest, fifth-largest attempt count of the tile's trajectories
// and the launch lasts as long as its slowest tile.  A tile is slow when its FIFTH trajectory is slow.  THE RULE (written here once;
// the device kernel below and the host mirror ionode_compose_order_host() both apply compose_slot() to the same total order):
//   - sort by cost, descending, ties by index; a non-finite or negative cost counts as 0;
//   - tile k takes sorted entries 4 k .. 4 k + 3 as its heavy slots 0 .. 3 (kComposeHeavy = the shrink threshold);
//   - its other 12 slots come from the light end, lightest first: tile 0 gets the 4 heaviest and the 12 lightest, and so on;
//   - only the last tile may be ragged: it gets the lightest heavies (as many as it has slots, at most 4) and the lights that remain;
//   - equal costs everywhere (nothing to compose) leave index order.
// Any input yields a permutation of [0, B): the order only decides the time, never the results (ionode_desc.launch_order).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ionode {

constexpr int kComposeTile = 16;     // trajectories per tile
constexpr int kComposeHeavy = 4;     // heavy slots per tile: MlpShrink4's threshold
constexpr int kComposeMaxB = 8192;   // the kernel sorts in LDS: 12 bytes per padded entry
constexpr int kComposeThreads = 1024;

// cost as the rule reads it
__host__ __device__ inline double compose_cost(double c) { return (c >= 0.0 && c <= 1.7976931348623157e308) ? c : 0.0; }

// the total order of the sort: heavier first, ties by index
__host__ __device__ inline bool compose_before(double ca, int ia, double cb, int ib) { return ca > cb || (ca == cb && ia < ib); }

// launch slot of the entry at position p of the sorted list of B entries
__host__ __device__ inline int compose_slot(int p, int B) {
  const int NT = (B + kComposeTile - 1) / kComposeTile;                  // tiles
  const int r = B - kComposeTile * (NT - 1);                             // slots of the last tile, 1 .. 16
  const int nH = kComposeHeavy * (NT - 1) + (r < kComposeHeavy ? r : kComposeHeavy);   // heavy entries
  const int LPT = kComposeTile - kComposeHeavy;                          // light slots of a full tile
  if (p < nH) return kComposeTile * (p / kComposeHeavy) + p % kComposeHeavy;
  const int q = B - 1 - p;                                               // rank from the light end
  if (q < LPT * (NT - 1)) return kComposeTile * (q / LPT) + kComposeHeavy + q % LPT;
  return kComposeTile * (NT - 1) + kComposeHeavy + (q - LPT * (NT - 1));  // what remains: the last tile's
}

// next power of two >= B (the bitonic network's size)
__host__ __device__ inline int compose_padded(int B) {
  int n = 1;
  while (n < B) n <<= 1;
  return n;
}
inline size_t compose_lds_bytes(int B) { return (size_t)compose_padded(B) * (sizeof(double) + sizeof(int32_t)); }

// cost[b * stride] as fp64 (I64 = 0) or int64 (I64 = 1: a column of a stats tensor, read in place) -> order[B].  ONE workgroup of
// kComposeThreads threads, bitonic sort in LDS (B <= kComposeMaxB; dynamic LDS = compose_lds_bytes(B)).  Padding entries sort last.
template <int I64>
__global__ void __launch_bounds__(kComposeThreads) ionode_compose_kernel(const void *__restrict__ cost, long long stride, int B,
                                                                         int32_t *__restrict__ order) {
  extern __shared__ __attribute__((aligned(16))) unsigned char compose_smem[];
  const int n = compose_padded(B);
  double *const key = reinterpret_cast<double *>(compose_smem);
  int32_t *const idx = reinterpret_cast<int32_t *>(key + n);
  for (int i = threadIdx.x; i < n; i += kComposeThreads) {
    double c = -1.0;   // padding: below every cost the rule can read
    if (i < B) {
      if constexpr (I64) c = compose_cost((double)static_cast<const long long *>(cost)[(long long)i * stride]);
      else c = compose_cost(static_cast<const double *>(cost)[(long long)i * stride]);
    }
    key[i] = c;
    idx[i] = i;
  }
  __syncthreads();
  for (int k = 2; k <= n; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = threadIdx.x; i < n; i += kComposeThreads) {
        const int l = i ^ j;
        if (l > i) {
          const double ci = key[i], cl = key[l];
          const int ii = idx[i], il = idx[l];
          const bool first = (i & k) == 0;   // this pair ends in the sort's order (else reversed)
          if (first ? compose_before(cl, il, ci, ii) : compose_before(ci, ii, cl, il)) {
            key[i] = cl; key[l] = ci;
            idx[i] = il; idx[l] = ii;
          }
        }
      }
      __syncthreads();
    }
  const bool flat = key[0] == key[B - 1];   // equal costs: index order (idx is then 0 .. B - 1 in place)
  for (int p = threadIdx.x; p < B; p += kComposeThreads) order[flat ? p : compose_slot(p, B)] = idx[p];
}

}  // namespace ionode
