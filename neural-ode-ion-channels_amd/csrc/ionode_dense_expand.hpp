// ionode_dense_expand.hpp -- deferred dense output of the lean N = 200 16-tile (KernelForm::defer): the record an accepted step
// leaves behind, and the streaming kernel that expands the records into y_out / i_out after the solve.
//
// Nothing of a step's dense output feeds the next evaluation of the net -- only the output cursor does.  On the tile every
// instruction between two evaluations extends the launch (one wavefront per SIMD, VALU work does not hide under the fp32 MFMA), so the
// solve kernel keeps the cursor and the fit and writes ONE record per accepted step that covers outputs; the expansion below is bound
// by the stores instead (one wavefront per record, lanes are samples).  Same expressions as the inline emission
// (ionode_attempt_body.hpp), same build flags (-ffp-contract=off): same bits.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ionode_kargs.hpp"
#include "ionode_math.hpp"

namespace ionode {

// One accepted step's interpolant, laid out as the lane-wise kernels' LDS row (LwLds::rowb): ROW = 4 + 5 D doubles,
//   [0] t0   [1] den = t1 - t0   [2] rden = 1 / den   [3] {int32 oi_before, int32 n_out}   [4 + c D + d] coefficient ic[c][d]
// Coefficients are stored as doubles and cast back to the state dtype (exact for fp32).  The workspace holds an int32 count per
// trajectory, then (16-byte aligned) the records [trajectory][cap][ROW].
template <int D> struct DenseRecord {
  static constexpr int ROW = 4 + 5 * D;
  static constexpr int BYTES = ROW * 8;
  static constexpr int CHUNKS = ROW / 2;   // 16-byte chunks: the unit a replica lane of the tile stores
  static constexpr int T0 = 0, DEN = 1, RDEN = 2, CURSOR = 3, COEF = 4;
  static_assert(ROW % 2 == 0, "records are whole 16-byte chunks");
  static __host__ __device__ constexpr size_t records_offset(int64_t B) { return ((size_t)B * 4 + 15) & ~(size_t)15; }
  static __host__ __device__ constexpr size_t workspace_bytes(int64_t B, int64_t cap) { return records_offset(B) + (size_t)B * (size_t)cap * BYTES; }
  static __device__ __forceinline__ double pack_cursor(int oi_before, int n_out) { return __hiloint2double(n_out, oi_before); }
  static __device__ __forceinline__ int cursor_oi(double w) { return __double2loint(w); }
  static __device__ __forceinline__ int cursor_n(double w) { return __double2hiint(w); }
};

// records of one block (a workgroup of 4 wavefronts walks it, one record per wavefront at a time), and the most blocks per trajectory
// a launch starts: the capacity is sized for the worst case, a trajectory's count is known on the device only, and a workgroup that
// finds no block left is pure dispatch cost -- past kExpandMaxBlocks a workgroup strides over the trajectory's blocks instead
constexpr int kExpandRecordsPerWg = 16;
constexpr int kExpandMaxBlocks = 128;

// Grid: x = blocks of kExpandRecordsPerWg records (strided beyond kExpandMaxBlocks), y = trajectories (strided when B exceeds the grid
// limit).  A workgroup past the trajectory's count leaves at once.  No LDS, no scratch.
template <typename S, int D> __global__ void __launch_bounds__(256) ionode_dense_expand_kernel(const KArgs a) {
  using Rec = DenseRecord<D>;
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int Nt = a.Nt;
  auto te_at = [&](int idx) -> double { return a.te_t0 + (double)idx * a.te_dt; };
  const bool want_i = a.i_out != nullptr;
  for (int tr = (int)blockIdx.y; tr < a.B; tr += (int)gridDim.y) {
    int cnt = a.defer_count[tr];
    cnt = cnt < a.defer_cap ? cnt : a.defer_cap;
    if ((int)blockIdx.x * kExpandRecordsPerWg >= cnt) continue;
    const int pj = a.prot_of_traj ? a.prot_of_traj[tr] : (tr % a.P);
    const double *__restrict__ pv = a.prot_v + (size_t)pj * a.Np;
    S *__restrict__ yo = a.y_out ? reinterpret_cast<S *>(a.y_out) + (size_t)tr * Nt * D : nullptr;
    double *__restrict__ io = a.i_out ? a.i_out + (size_t)tr * Nt : nullptr;
    for (int r0 = (int)blockIdx.x * kExpandRecordsPerWg; r0 < cnt; r0 += (int)gridDim.x * kExpandRecordsPerWg) {
    const int r1 = (r0 + kExpandRecordsPerWg < cnt) ? r0 + kExpandRecordsPerWg : cnt;
    for (int ri = r0 + wv; ri < r1; ri += 4) {
      const double *__restrict__ rec = a.defer_rec + ((size_t)tr * (size_t)a.defer_cap + (size_t)ri) * Rec::ROW;
      const double t0b = rec[Rec::T0], denb = rec[Rec::DEN], rdenb = rec[Rec::RDEN];
      const double cur = rec[Rec::CURSOR];
      const int o = Rec::cursor_oi(cur), n = Rec::cursor_n(cur);
      S cb[5][D];
#pragma unroll
      for (int c = 0; c < 5; ++c)
#pragma unroll
        for (int d = 0; d < D; ++d) cb[c][d] = (S)rec[Rec::COEF + c * D + d];
      for (int c0 = 0; c0 < n; c0 += 64) {
        const int idx = o + c0 + lane;
        if (c0 + lane < n && idx < Nt) {
          const double tk = te_at(idx);
          const S x = (S)div_pos(tk - t0b, denb, rdenb);  // _interp_evaluate: x = (t - t0) / (t1 - t0) in fp64, cast; running powers
          S out[D];
          S xp = x;
#pragma unroll
          for (int d = 0; d < D; ++d) out[d] = cb[0][d] + x * cb[1][d];
#pragma unroll
          for (int c = 2; c < 5; ++c) {
            xp = xp * x;
#pragma unroll
            for (int d = 0; d < D; ++d) out[d] = out[d] + xp * cb[c][d];
          }
          if (yo) {
            if constexpr (sizeof(S) == 8) {
#pragma unroll
              for (int d = 0; d < D; d += 2) *reinterpret_cast<double2 *>(yo + (size_t)idx * D + d) = make_double2(out[d], out[d + 1]);
            } else {
#pragma unroll
              for (int d = 0; d < D; d += 2) *reinterpret_cast<float2 *>(yo + (size_t)idx * D + d) = make_float2(out[d], out[d + 1]);
            }
          }
          if (want_i) {
            int ip;
            const bool inr = protocol_index(a, tk, ip);
            const double vk = inr ? protocol_from(a, pv[ip - 1], pv[ip], ip, tk) : a.v_oob;
            S gate;
            if (a.obs_open) gate = out[D - 1]; else gate = out[0] * out[1];
            if (a.obs_g != 1.0) gate = (S)a.obs_g * gate;
            io[idx] = (double)gate * (vk - a.obs_e);
          }
        }
      }
    }
    }
  }
}

}  // namespace ionode
