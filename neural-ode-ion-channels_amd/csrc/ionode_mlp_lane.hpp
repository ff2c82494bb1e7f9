// ionode_mlp_lane.hpp -- MlpLane: the N = 10 net per lane on the vector ALU (included by ionode_device.hpp, behind KArgs).
#pragma once

namespace ionode {

// ---------------------------------------------------------------------------------------------
// N = 10 nets (architectures s03-s05) at one trajectory per lane: the net evaluated PER LANE on the vector ALU, weights as
// SCALAR operands.  The MFMA form of this path (MlpTile::eval_tiny64) spends 80 MFMAs = 2560 cycles per evaluation on 16 x 16
// tiles of a 10 x 10 layer, gathers its inputs across lanes and keeps four accumulator tiles; per lane the net is 530 fmaf + 2 x 60
// LeakyReLU operations with no cross-lane traffic, and ~25 registers instead of ~110.  Every weight is used by all 64
// lanes at once, so it is read through the scalar cache (constant address space: s_load_dwordx8/x16) and enters the FMA as its
// one SGPR operand.  Same canonical order as the oracle / the MFMA tile with NT = 1:
//   hidden row j:  acc = bias; for r = 0..3: for q = 0..3: k = 4 q + r < N: acc = fmaf(W[j][k], h[k], acc)
//   Linear(N, 1):  part_q = 0; for r: k = 4 q + r < N: part_q = fmaf(wl[k], h[k], part_q); out = ((p0 + p1) + (p2 + p3)) + bl
// The padded terms the tile executes (k >= N: fmaf(0, 0, acc)) are skipped: they return acc for every acc except -0, and an
// accumulator can only be -0 if its bias is -0 (x + (-x) rounds to +0; +0 + -0 = +0), which ionode_mlp_pack rules out by writing
// bias + 0.0f into this section (N < 16; the tile's own trailing padded term does the same to its result).
// TWO ROWS PER INSTRUCTION: rows 2 m and 2 m + 1 run the same k sequence on the same inputs, so their chains are the two halves of
// one v_pk_fma_f32 -- weights {W[2m][k], W[2m+1][k]} in an SGPR pair, h[k] broadcast from its half of the activation pair
// (op_sel), accumulators in a VGPR pair: one exact fmaf per half, 4 cycles for both (gfx950's vector fp32 peak IS the packed rate).
// A layer's output pair m = {h[2m], h[2m+1]} is the next layer's input pair.  The LeakyReLU multiply is packed as well.
// Image section (ionode_mlp_pack, behind wl / bl): row pair m of layer 0: {b0, b0'} {w00, w00'} {w01, w01'} {0, 0}; then, per hidden
// layer and row pair, PB floats: {W[2m][k], W[2m+1][k]} in the canonical k order, {bias, bias'}, pad.
// ---------------------------------------------------------------------------------------------
// (GP = 5 row pairs of a hidden layer evaluated together (scalar loads of the group in flight at once, independent chains): 65 536 x 20 001: 15.5 ms at 1, 14.3 at 2, 14.2 at 3, 13.6 at 5; 262 144: 38.4 / 36.6 / 36.6 / 36.0)
// acc + w * h.lo / acc + w * h.hi in both halves (one fused multiply-add each); w: SGPR pair
__device__ __forceinline__ f32x2 pk_fma_lo(f32x2 w, f32x2 h, f32x2 acc) {
  asm("v_pk_fma_f32 %0, %1, %2, %0 op_sel_hi:[1,0,1]" : "+v"(acc) : "s"(w), "v"(h));
  return acc;
}
__device__ __forceinline__ f32x2 pk_fma_hi(f32x2 w, f32x2 h, f32x2 acc) {
  asm("v_pk_fma_f32 %0, %1, %2, %0 op_sel:[0,1,0] op_sel_hi:[1,1,1]" : "+v"(acc) : "s"(w), "v"(h));
  return acc;
}
__device__ __forceinline__ f32x2 lrelu2(f32x2 x) {
  f32x2 t, h;
  const f32x2 c = {0.01f, 0.01f};
  asm("v_pk_mul_f32 %0, %1, %2" : "=v"(t) : "v"(x), "s"(c));
  float h0, h1;
  asm("v_max_f32 %0, %1, %2" : "=v"(h0) : "v"(x.x), "v"(t.x));
  asm("v_max_f32 %0, %1, %2" : "=v"(h1) : "v"(x.y), "v"(t.y));
  h.x = h0; h.y = h1;
  return h;
}
template <int N> struct MlpLane {
  static_assert(N == 10, "the per-lane net is instantiated for N = 10 (architectures s03-s05)");
  static constexpr int GW = 1;
  static constexpr int NP = 16;
  static constexpr int NPAIR = (N + 1) / 2;
  static constexpr int PB = (2 * (N + 1) + 3) & ~3;   // floats per (layer, row pair) block of the scalar section
  typedef const float __attribute__((address_space(4))) cfloat;   // constant address space: uniform loads are scalar loads
  typedef const f32x2 __attribute__((address_space(4))) cfloat2;
  const cfloat *img;   // the tile's packed image
  int L;
#ifdef IONODE_STAMPS
  Stamps *sp;
#endif
  static __host__ __device__ constexpr size_t lds_bytes(int) { return 0; }
  static __host__ __device__ constexpr size_t scalar_floats(int L) { return (size_t)NPAIR * 8 + (size_t)L * NPAIR * PB; }
  __device__ __forceinline__ void init(const KArgs &a, unsigned char *, int, int, int first_traj = 0) {
    L = a.L;
    const float *g = a.mlp + (a.traj_per_img > 0 ? (size_t)(first_traj / a.traj_per_img) * (size_t)a.mlp_stride : (size_t)0);
    img = (const cfloat *)(uintptr_t)g;
  }
  // canonical position of k in a row's chain: r-major, q-minor over k = 4 q + r < N
  static __host__ __device__ constexpr int k_at(int pos) {
    int n = 0;
    for (int r = 0; r < 4; ++r)
      for (int q = 0; q < 4; ++q)
        if (4 * q + r < N) { if (n == pos) return 4 * q + r; ++n; }
    return -1;
  }
#ifndef IONODE_VNET_RELOAD
#define IONODE_VNET_RELOAD 1   // 1: Linear(2, N) and Linear(N, 1) are scalar loads of THIS evaluation (round 5).  0 (rounds 3-4): hipcc hoists
                               // the 62 loop-invariant scalars out of the attempt loop, cannot keep them in scalar registers next to the hidden
                               // layers' 110 and parks them in VGPR lanes: 79 v_readlane per evaluation -- vector-ALU work in a vector-issue-bound kernel
#endif
  __device__ __forceinline__ float eval_tiny64(float x0, float x1) {
    constexpr size_t lstride = (size_t)256 + NP;  // MlpTile<1, 1, 1, 1>::layer_floats(): one fragment + bias[NP]
    const cfloat *im = img;
    if (IONODE_VNET_RELOAD) asm volatile("" : "+s"(im));     // (an opaque copy of the pointer: loads through it stay inside this evaluation)
    const cfloat *wl = im + 4 * NP + (size_t)L * lstride;   // wl[NP], bl, 3 pad
    const cfloat2 *s0 = reinterpret_cast<const cfloat2 *>(wl + NP + 4);   // the scalar section: layer 0 ...
    const cfloat2 *sh = s0 + NPAIR * 4;                                    // ... and the hidden layers
    f32x2 h[NPAIR];
    {
      const f32x2 xx = {x0, x1};
#pragma unroll
      for (int m = 0; m < NPAIR; ++m) h[m] = lrelu2(pk_fma_hi(s0[4 * m + 2], xx, pk_fma_lo(s0[4 * m + 1], xx, s0[4 * m + 0])));
    }
    constexpr int GP = 5;   // row pairs of a hidden layer evaluated together (above)
    for (int l = 0; l < L; ++l) {
      f32x2 g[NPAIR];
#pragma unroll
      for (int m0 = 0; m0 < NPAIR; m0 += GP) {
        // a group's scalar loads are issued together (one wait); its chains are independent of each other (a lone dependent
        // chain stalls a SIMD that holds few wavefronts)
#pragma unroll
        for (int u = 0; u < GP; ++u)
          if (m0 + u < NPAIR) g[m0 + u] = sh[((size_t)l * NPAIR + m0 + u) * (PB / 2) + N];
#ifndef IONODE_VNET_SPLIT
#define IONODE_VNET_SPLIT 5   // > 0: a scheduling barrier after this many k positions: half of the 110 weight scalars of a row-pair group in flight, so that the kernel's own uniform state stays in scalar registers (with IONODE_VNET_RELOAD: 539 -> 49 v_readlane per attempt)
#endif
#pragma unroll
        for (int pos = 0; pos < N; ++pos) {
#pragma unroll
          for (int u = 0; u < GP; ++u)
            if (m0 + u < NPAIR) {
              const f32x2 w = sh[((size_t)l * NPAIR + m0 + u) * (PB / 2) + pos];
              const int k = k_at(pos);
              g[m0 + u] = (k & 1) ? pk_fma_hi(w, h[k >> 1], g[m0 + u]) : pk_fma_lo(w, h[k >> 1], g[m0 + u]);
            }
          if (IONODE_VNET_SPLIT > 0 && pos + 1 == IONODE_VNET_SPLIT) __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int u = 0; u < GP; ++u)
          if (m0 + u < NPAIR) g[m0 + u] = lrelu2(g[m0 + u]);
        __builtin_amdgcn_sched_barrier(0);
      }
#pragma unroll
      for (int m = 0; m < NPAIR; ++m) h[m] = g[m];
    }
    if (IONODE_VNET_RELOAD) asm volatile("" : "+s"(wl));     // (Linear(N, 1)'s scalars are loaded after the hidden stack, not carried through it)
    float part[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      part[q] = 0.0f;
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (4 * q + r < N) part[q] = fmaf(wl[4 * q + r], h[(4 * q + r) >> 1][(4 * q + r) & 1], part[q]);
    }
    return ((part[0] + part[1]) + (part[2] + part[3])) + wl[NP];
  }
  __device__ __forceinline__ float eval(float x0, float x1) { return eval_tiny64(x0, x1); }
};

}  // namespace ionode
