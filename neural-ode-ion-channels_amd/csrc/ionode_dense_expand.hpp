// ionode_dense_expand.hpp -- deferred dense output of the lean N = 200 16-tile (KernelForm::defer): the record an accepted step
// leaves behind, the routine that expands records into y_out / i_out, and the streaming kernel that runs it after the solve (the
// solve kernel runs it too, for the tiles that end early: ionode_device.hpp).
//
// Nothing of a step's dense output feeds the next evaluation of the net -- only the output cursor does.  On the tile every
// instruction between two evaluations extends the launch (one wavefront per SIMD, VALU work does not hide under the fp32 MFMA), so the
// solve kernel keeps the cursor and the fit and writes ONE record per accepted step that covers outputs; the expansion below is bound
// by memory instead (one wavefront per record, lanes are samples).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ionode_interp.hpp"
#include "ionode_kargs.hpp"
#include "ionode_math.hpp"

namespace ionode {

// One accepted step's interpolant: an InterpRow (ionode_interp.hpp; the lane-wise kernels' LDS row) whose spare slot holds the
// cursor {int32 oi_before, int32 n_out}.  A 16-byte chunk is the unit a replica lane of the tile stores.  The workspace holds an
// int32 count per trajectory, then (16-byte aligned) the records [trajectory][cap][ROW].
template <int D> struct DenseRecord : InterpRow<D> {
  using InterpRow<D>::BYTES;
  static constexpr int CURSOR = InterpRow<D>::SPARE;
  static __host__ __device__ constexpr size_t records_offset(int64_t B) { return ((size_t)B * 4 + 15) & ~(size_t)15; }
  static __host__ __device__ constexpr size_t workspace_bytes(int64_t B, int64_t cap) { return records_offset(B) + (size_t)B * (size_t)cap * BYTES; }
  static __device__ __forceinline__ double pack_cursor(int oi_before, int n_out) { return __hiloint2double(n_out, oi_before); }
  static __device__ __forceinline__ int cursor_oi(double w) { return __double2loint(w); }
  static __device__ __forceinline__ int cursor_n(double w) { return __double2hiint(w); }
};

// records of one block (a workgroup of 4 wavefronts walks it, one record per wavefront at a time), and the workgroups a launch starts:
// the capacity is sized for the worst case and a trajectory's count is known on the device only, so a fixed grid strides over the
// (trajectory, block) pairs -- a pair past the trajectory's count costs one cached load of the count, not a workgroup
#ifndef IONODE_EXPAND_RECORDS_PER_WG
#define IONODE_EXPAND_RECORDS_PER_WG 64   // (a build switch for A/B runs: tools/build_variant.sh)
#endif
constexpr int kExpandRecordsPerWg = IONODE_EXPAND_RECORDS_PER_WG;
constexpr int kExpandMaxBlocks = 128;
constexpr int kExpandGrid = 256 * 8;      // workgroups of the follow-up kernel (eight per compute unit)
// record headers in flight per wavefront (dense_expand_records): the follow-up kernel hides a record's round trip behind its sixteen
// wavefronts per compute unit as well, the solve kernel's tail (one wavefront per SIMD) behind these alone
constexpr int kExpandAheadKernel = 4;
constexpr int kExpandAheadTail = 8;

// THE expansion: records r0, r0 + step, ... < r1 of trajectory tr, by one wavefront (lanes are samples).  Both callers -- the follow-up
// kernel below and the solve kernel's tail (ionode_device.hpp) -- run this routine.  The per-sample expressions are the inline emission's
// (ionode_attempt_body.hpp): both call interp_eval / obs_current, whose single definition is in ionode_interp.hpp.
// A record is wave-uniform: lane e < ROW loads double e of it (ONE vector load per record; a vector load also sees what the workgroup's
// own wavefronts stored before a fence, which the scalar cache would not promise) and the fields are read out of that lane.
// gfx9 counts loads and stores in one in-order vmcnt (ionode_device.hpp "where the dense output goes through"): a load issued behind
// a store waits for the store's acknowledgement.  So K record loads stay in flight, and the protocol samples of record r + 1 (they
// depend on its cursor word alone) are issued BEFORE the stores of record r; only a record's chunks past the first 64 samples load
// behind stores.  Past the wavefront's last record the pipeline re-reads that record (looked up, never emitted): no guard, no branch.
template <typename S, int D, int K>
__device__ __forceinline__ void dense_expand_records(const KArgs &a, int tr, int r0, int r1, int step, int lane) {
  using Rec = DenseRecord<D>;
  static_assert(Rec::ROW <= 64, "one lane per double of a record");
  if (r0 >= r1) return;
  const int Nt = a.Nt;
  const bool want_i = a.i_out != nullptr;
  const int pj = a.prot_of_traj ? a.prot_of_traj[tr] : (tr % a.P);
  const double *__restrict__ pv = a.prot_v + (size_t)pj * a.Np;
  S *__restrict__ yo = a.y_out ? reinterpret_cast<S *>(a.y_out) + (size_t)tr * Nt * D : nullptr;
  double *__restrict__ io = a.i_out ? a.i_out + (size_t)tr * Nt : nullptr;
  const double *__restrict__ recs = a.defer_rec + (size_t)tr * (size_t)a.defer_cap * Rec::ROW + (lane < Rec::ROW ? lane : Rec::ROW - 1);
  const int last = r0 + ((r1 - 1 - r0) / step) * step;   // this wavefront's last record
  auto fetch = [&](int ri) -> double { return recs[(size_t)(ri < last ? ri : last) * Rec::ROW]; };
  struct Head {   // wave-uniform
    Interp<S, D> itp;
    int o, n;
  };
  struct Samples {   // the first lookup of a 64-sample chunk: output time, protocol index and the two protocol samples
    double tk, lo, hi;
    int ip;
    bool inr;
  };
  auto decode = [&](double raw, Head &h) {
    h.itp.from_lane_doubles(raw);
    const double cur = bcast_f64(raw, Rec::CURSOR);
    h.o = Rec::cursor_oi(cur); h.n = Rec::cursor_n(cur);
  };
  auto lookup = [&](const Head &h, int c0, Samples &s) {
    s.tk = a.te_t0 + (double)(h.o + c0 + lane) * a.te_dt;
    s.lo = s.hi = 0.0; s.ip = 1; s.inr = false;
    if (want_i) {
      s.inr = protocol_index(a, s.tk, s.ip);   // (idle lanes: a valid index whatever the time is; their loads are harmless)
      s.lo = pv[s.ip - 1]; s.hi = pv[s.ip];
    }
  };
  auto emit = [&](const Head &h, int c0, const Samples &s) {
    const int idx = h.o + c0 + lane;
    if (c0 + lane < h.n && idx < Nt) {
      const double tk = s.tk;
      S out[D];
      interp_eval<S, D>(h.itp.cb, h.itp.x(tk), out);
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
        const double vk = s.inr ? protocol_from(a, s.lo, s.hi, s.ip, tk) : a.v_oob;
        io[idx] = obs_current<S, D>(a, out, vk);
      }
    }
  };
  double raw[K];
#pragma unroll
  for (int k = 0; k < K; ++k) raw[k] = fetch(r0 + k * step);
  Head hc, hn;
  Samples sc, sn;
  decode(raw[0], hc);
  lookup(hc, 0, sc);
  for (int ri = r0; ri < r1; ri += K * step) {
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int rk = ri + k * step;
      if (rk >= r1) break;
      raw[k] = fetch(rk + K * step);      // (slot k held record rk: decoded one record ago)
      decode(raw[(k + 1) % K], hn);       // record rk + step
      lookup(hn, 0, sn);
      emit(hc, 0, sc);
      for (int c0 = 64; c0 < hc.n; c0 += 64) {
        Samples s;
        lookup(hc, c0, s);
        emit(hc, c0, s);
      }
      hc = hn; sc = sn;
    }
  }
}

// Grid: kExpandGrid workgroups (fewer for a small batch) stride over the pairs (trajectory, block of kExpandRecordsPerWg records); a
// trajectory offers ceil(cap / kExpandRecordsPerWg) blocks, at most kExpandMaxBlocks -- past that a pair strides over the trajectory's
// blocks.  A count <= 0 means nothing is left here: the trajectory wrote no record, or the solve kernel's tail expanded them
// (-(records + 1)).  No LDS, no scratch.
template <typename S, int D> __global__ void __launch_bounds__(256) ionode_dense_expand_kernel(const KArgs a) {
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int nblk = (a.defer_cap + kExpandRecordsPerWg - 1) / kExpandRecordsPerWg;
  const int bpt = nblk < kExpandMaxBlocks ? nblk : kExpandMaxBlocks;   // blocks per trajectory this launch hands out
  const long long pairs = (long long)a.B * bpt;
  for (long long pr = blockIdx.x; pr < pairs; pr += gridDim.x) {
    const int tr = (int)(pr / bpt), b0 = (int)(pr % bpt);
    int cnt = a.defer_count[tr];
    cnt = cnt < a.defer_cap ? cnt : a.defer_cap;
    for (int r0 = b0 * kExpandRecordsPerWg; r0 < cnt; r0 += bpt * kExpandRecordsPerWg) {
      const int r1 = (r0 + kExpandRecordsPerWg < cnt) ? r0 + kExpandRecordsPerWg : cnt;
      dense_expand_records<S, D, kExpandAheadKernel>(a, tr, r0 + wv, r1, 4, lane);
    }
  }
}

}  // namespace ionode
