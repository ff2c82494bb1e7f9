// ionode_mlp_tile.hpp -- MlpTile: the stage MLP of one 16-trajectory tile on the fp32 MFMA (included by ionode_device.hpp, behind KArgs).
#pragma once

namespace ionode {

// ---------------------------------------------------------------------------------------------
// Stage MLP of one 16-trajectory tile on the fp32 MFMA.  All G wavefronts of the workgroup call
// eval() together in uniform control flow; it returns net([x0, x1]) for the lane's trajectory.
//
// Work split.  A hidden layer is NT row tiles x NT k-tiles of 16x16x4 MFMAs (4 per tile pair).  Each of the G
// wavefronts owns F = NT/G FULL row tiles (rt = w + i*G: all k-tiles) and a 1/G K-slice (k-tiles kt % G == w) of each
// of the R = NT - G*F REMAINDER row tiles (rt = G*F + j).  For N = 200 (NT = 13, G = 4) that is 3*13 + 13/4 tile
// products per wavefront instead of 4*13 on the critical wavefront.  The K-slices of a remainder tile are
// partial sums; they meet in LDS and every wavefront folds them itself after the layer barrier.
// Wavefront w walks the k-tiles in the rotated order kt = (s + w) mod NT, s = 0..NT-1, so that "this step carries my
// K-slice" is the compile-time predicate s % G == 0 (plus s + w < NT on the last such step) instead of a branch per
// k-step, and the weight stream of a wavefront has a static shape.
//
// Canonical accumulation order (the oracle executes exactly this; DESIGN.md "canonical MLP order"):
//   k index of (k-tile kt, k-step r, lane group q):  k = 16*kt + 4*q + r        (accumulator layout == B operand layout)
//   full tile rows:       acc = bias; for s = 0..NT-1, kt = (s + rt % G) mod NT: for r: for q: acc = fmaf(W[row][k], h[k], acc)
//   remainder tile rows:  p_w = (w == 0 ? bias : 0); for kt with kt % G == w, ascending: for r: for q: p_w = fmaf(...)
//                         acc = (p_0 + p_1) + (p_2 + p_3)                            (G = 4; G = 1 has no remainder)
//   Linear(N, 1):         part_q = 0; for kt: for r: part_q = fmaf(wl[k], h[k], part_q);
//                         out = ((part_0 + part_1) + (part_2 + part_3)) + bl
//
// Weight streaming.  The A fragments of the hidden layers are the only global traffic of the MLP.  Stream order
// (ionode_mlp_pack): layer | wavefront w | step s (k-tile (s + w) mod NT) | fragments | lane.  Every step has F
// fragments holding the full tiles k-step-major (element e = r*F + i -> float4 e/4, component e%4); steps with
// s % G == 0 carry R more, one per remainder tile (components = k-steps r; zeros when s + w >= NT).
// Fragments are consumed from a register ring
// refilled PD k-tiles ahead (PD == NT: a whole layer ahead) with SRSRC buffer loads issued right behind the last
// MFMA that reads them, pinned with sched_barrier so the machine scheduler neither sinks them to the end of the
// layer nor bunches them into an MFMA-free gap.  The stream runs at ~28 B/clk/CU; it is not the limiter (cutting its
// bytes by 17 % changed nothing): the MFMA count and the issue work per k-tile step and per layer boundary are.
// Small vectors (layer-0 rows, biases, last-layer weights) live in LDS for the kernel's lifetime.
// ---------------------------------------------------------------------------------------------
// Hand-scheduled hidden-layer stream (tools/gen_mlp_asm.py -> mlp_asm_nt13.inc): the N = 200 tile <4, 4, 13, 13> runs its
// hidden stack as ONE inline-asm statement with a fixed register map (weight ring in AGPRs a[0:171], working set in
// v[184:255]) and a software-pipelined layer boundary; same canonical accumulation order, same bits.  -DIONODE_NO_ASM_CORE
// builds the compiler-scheduled stream instead (A/B, stamps).
// Round 5: N = 200 pads its contraction index to 208; k-tile 12 holds eight real k and eight padding columns -- two of the four k of each of
// its MFMAs.  Without the padding terms (exact no-ops) the canonical chain through the tile is 192, 196, 193, 197 | 194, 198, 195, 199: the asm
// stream runs it as TWO MFMAs per accumulator (tools/gen_mlp_asm.py "short form"), and ionode_mlp_pack lays the tile's A fragments out for it.
#ifndef IONODE_KT12_SHORT
#if defined(IONODE_NO_ASM_CORE)
#define IONODE_KT12_SHORT 0
#else
#define IONODE_KT12_SHORT 1
#endif
#endif
#if !defined(IONODE_NO_ASM_CORE)
#define IONODE_ASM_CORE 1
#include "mlp_asm_nt13.inc"
#include "mlp_asm_nt13x2.inc"
#else
#define IONODE_ASM_CORE 0
#endif

template <int G, int RT, int NT, int PD, int NSETS_ = 1>
struct MlpTile {
  static constexpr bool ASM = IONODE_ASM_CORE && G == 4 && NT == 13 && PD == 13;
  static constexpr int GW = G;           // wavefronts per tile
  // NSETS == 2: TWO 16-trajectory column sets per tile (32 trajectories per workgroup; launches of >= 2 tiles per compute unit).
  // Every weight fragment then feeds two MFMAs, and wavefronts 0, 1 integrate set 0, wavefronts 2, 3 set 1: the scalar
  // Runge-Kutta work is replicated twice per trajectory instead of four times.  Asm stream only (tools/gen_mlp_asm.py --ns 2).
  static constexpr int NSETS = NSETS_;
  static_assert(NSETS == 1 || NSETS == 2, "one or two column sets");
  static_assert(NSETS == 1 || ASM, "two column sets exist for the asm tile only");
  static constexpr int F = NT / G;       // full row tiles per wavefront
  static constexpr int R = NT - G * F;   // remainder row tiles, K-split over the G wavefronts
  static constexpr int NP = 16 * NT;
  static constexpr int RP = (R > 0 ? R : 1);
  static constexpr int HT = NT + G - 1;  // activation slots per buffer (see Hs)
  static_assert(NT % PD == 0, "ring depth must divide the k-tile count");
  static_assert(RT == F + R, "RT = full + remainder tile slots per wavefront");
  static_assert((4 * RT) % 4 == 0 && (RT == 1 || RT == 2 || RT == 4 || RT == 8), "fragment = RT float4 per k-tile");
  static_assert(R == 0 || G == 4, "the remainder combine tree is written for 4 wavefronts");
  static constexpr int NOWN = (NT + G - 1) / G;      // steps s = 0, G, 2G, ... carry a K-slice of the remainder tiles
  static constexpr int FRAGS = NT * F + NOWN * R;    // 1 KiB fragments per wavefront per layer
  // ring slot of step u (blocked scheme: step kt0 + u): F full fragments (+ R remainder fragments when owned)
  f32x4 ring[PD][F > 0 ? F : 1];
  // N = 100 (NT = 7: one full tile per wavefront + THREE remainder tiles): K-splitting three tiles over the wavefronts costs three
  // partial-sum exchanges and a 60-instruction fold per layer on every wavefront, and the layer barrier waits for it.  OWNREM:
  // wavefront w < R computes remainder tile w WHOLE -- its four canonical partial chains p_0..p_3 (k-tiles kt % 4 == c, ascending)
  // in four accumulators, folded in registers with the canonical tree -- so the layer's activations are complete at the barrier.
  // 56 / 56 / 56 / 28 MFMAs per layer instead of 52 / 52 / 52 / 40, no partial sums in LDS; same chains, same bits.  The chains
  // need the k-tiles in natural order (the full tile walks them rotated), so they read their own B operands, one step behind.
  static constexpr bool OWNREM = (G == 4 && F == 1 && R == 3 && PD == NT);
  f32x4 rrem[(R > 0 && !OWNREM) ? (PD + G - 1) / G : 1][(R > 0 && !OWNREM) ? RP : 1];
  f32x4 rown[OWNREM ? NT : 1];   // fragments of my remainder tile, one per k-tile (a layer ahead, like the ring)
  unsigned voff0;                // per lane: lane * 16 (fragments of another wavefront's stream: frag_of)
  // NT == 1 (N <= 16, architectures s03-s05): the whole hidden stack is LMAX fragments -- it stays in registers
  static constexpr bool TINY = (NT == 1 && G == 1);
  static constexpr int LMAX = 10;
  f32x4 wres[TINY ? LMAX : 1];
  // LDS [2][HT*64] activations after LeakyReLU, accumulator layout.  HT = NT + G - 1 slots: tiles 0..G-2 are stored
  // twice (slot kt and kt + NT) so that wavefront w reads its rotated sequence kt = (s + w) mod NT at the linear
  // address base_w + s -- an immediate offset, no per-step address arithmetic.  Remainder-tile slots are filled by
  // every wavefront itself (identical bits) when it folds the partial sums.
  f32x4 *Hs;
  f32x4 *Ps;          // LDS [2][R][G][64] partial sums of the remainder tiles (pre-activation)
  const f32x4 *W0s;   // LDS [NP] {b0, w00, w01, 0}
  const float *biasS; // LDS [L][NP]
  const float *wlS;   // LDS [NP] + bl
  __amdgpu_buffer_rsrc_t rsrc;  // weight image; one 32-bit VGPR offset per lane + scalar offset per load
  unsigned voff;      // per lane: byte offset of (this wavefront's stream, lane) inside a hidden layer
  unsigned hid0;      // byte offset of hidden layer 0 in the image
  unsigned lbytes;    // bytes per hidden layer in the image
  unsigned lds0;      // LDS byte address of the tile's region (asm stream)
  int bl_bits;        // bias of Linear(N, 1), wave-uniform (asm stream)
  int sw12;           // asm stream: the wavefront's index when k-tile 12 may take its two-MFMA form (N <= 200: k >= 200 is padding), else 99
  int L, wave, lane;
#ifdef IONODE_STAMPS
  Stamps *sp;
#endif

  static __host__ __device__ constexpr size_t layer_floats() { return (size_t)G * FRAGS * 256 + NP; }
  // index of step s's first fragment in a wavefront's layer stream
  static __host__ __device__ constexpr int step_base(int s) { return s * F + R * ((s + G - 1) / G); }
  static __host__ __device__ constexpr size_t lds_bytes(int L) {
    return ((size_t)2 * NSETS * HT * 64 + (size_t)2 * NSETS * R * G * 64 + NP) * 16 + ((size_t)L * NP + NP + 4) * 4;
  }
  // the asm stream parks the stores of a not-yet-existing previous layer in a 1 KiB scratch slot behind the tile's LDS
  // (so that every pass issues the same LDS operations and the wait counts are static); two column sets: + 256 B through
  // which the wavefronts exchange their stage inputs
  static __host__ __device__ constexpr size_t scratch_off(int L) { return (lds_bytes(L) + 15) & ~(size_t)15; }
  static __host__ __device__ constexpr size_t lds_total(int L) { return ASM ? scratch_off(L) + 1024 + (NSETS > 1 ? 256 : 0) : lds_bytes(L); }

  __device__ __forceinline__ void init(const KArgs &a, unsigned char *smem, int wave_, int lane_, int first_traj = 0) {
    L = a.L; wave = wave_; lane = lane_;
    // the tile's weight image: the shared one, or image number first_traj / traj_per_img of an ensemble
    const float *__restrict__ img = a.mlp + (a.traj_per_img > 0 ? (size_t)(first_traj / a.traj_per_img) * (size_t)a.mlp_stride : (size_t)0);
    Hs = reinterpret_cast<f32x4 *>(smem);
    Ps = Hs + 2 * NSETS * HT * 64;
    f32x4 *w0 = Ps + 2 * NSETS * R * G * 64;
    float *bs = reinterpret_cast<float *>(w0 + NP);
    float *ws = bs + (size_t)L * NP;
    constexpr size_t lstride = layer_floats();
    const int tid = wave * 64 + lane;
    const f32x4 *src = reinterpret_cast<const f32x4 *>(img);
    for (int i = tid; i < NP; i += 64 * G) w0[i] = src[i];
    for (int i = tid; i < L * NP; i += 64 * G) bs[i] = img[4 * (size_t)NP + (size_t)(i / NP) * lstride + (lstride - NP) + (i % NP)];
    const float *wl = img + 4 * (size_t)NP + (size_t)L * lstride;
    for (int i = tid; i < NP + 4; i += 64 * G) ws[i] = wl[i];
    W0s = w0; biasS = bs; wlS = ws;
    const size_t img_bytes = (4 * (size_t)NP + (size_t)L * lstride + NP + 4) * 4;
    rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(img), 0, (int)img_bytes, 0x00020000);
    voff = (unsigned)(wave * FRAGS * 1024 + lane * 16);
    voff0 = (unsigned)(lane * 16);
    hid0 = (unsigned)(4 * NP * 4);
    lbytes = (unsigned)(lstride * 4);
    if constexpr (TINY) {
#pragma unroll
      for (int l = 0; l < LMAX; ++l) wres[l] = (l < L) ? frag(hid0 + (unsigned)l * lbytes, 0) : f32x4{0, 0, 0, 0};
    }
    if constexpr (ASM) {
#if IONODE_ASM_CORE
      lds0 = (unsigned)(uintptr_t)smem;
      if (L > 0)
        asm volatile(IONODE_MLPASM_INIT_13
                     :
                     : [voff] "v"(voff), [rsrc] "s"(rsrc), [hid0] "s"(hid0)
                     : "memory", "scc", IONODE_MLPASM_CLOBBER_A_13, IONODE_MLPASM_CLOBBER_S_13);
#endif
      __syncthreads();
      bl_bits = __builtin_amdgcn_readfirstlane(__float_as_int(wlS[NP]));
      sw12 = (IONODE_KT12_SHORT && a.N <= 200) ? wave : 99;
      return;
    }
    // prime the ring with the first PD steps of hidden layer 0
#pragma unroll
    for (int u = 0; u < (TINY ? 0 : PD); ++u) {
#pragma unroll
      for (int j = 0; j < F; ++j) ring[u][j] = frag(hid0, step_base(u) + j);
      if constexpr (R > 0 && !OWNREM) {
        if (u % G == 0) {
#pragma unroll
          for (int j = 0; j < R; ++j) rrem[u / G][j] = frag(hid0, step_base(u) + F + j);
        }
      }
    }
    if constexpr (OWNREM) {
#pragma unroll
      for (int kt = 0; kt < NT; ++kt) rown[kt] = frag_of(hid0, kt);
    }
    __syncthreads();
  }

  // OWNREM: the fragment of remainder tile `wave` for k-tile kt.  It sits in the stream of wavefront kt % G (the K-slice owner of
  // the packed layout, ionode_mlp_pack), at that wavefront's owned step kt - kt % G, behind the step's F full-tile fragments.
  __device__ __forceinline__ f32x4 frag_of(unsigned lbase, int kt) const {
    using u32x4 = __attribute__((ext_vector_type(4))) unsigned;
    const unsigned n = (unsigned)((kt % G) * FRAGS + step_base(kt - kt % G) + F) + (unsigned)(wave < R ? wave : 0);
    const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rsrc, voff0, lbase + n * 1024u, 0);
    return __builtin_bit_cast(f32x4, v);
  }

  // one 1 KiB fragment (64 lanes x float4): fragment n of this wavefront's stream of the layer at byte offset `lbase`
  __device__ __forceinline__ f32x4 frag(unsigned lbase, int n) const {
    using u32x4 = __attribute__((ext_vector_type(4))) unsigned;
    const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rsrc, voff, lbase + (unsigned)n * 1024u, 0);
    return __builtin_bit_cast(f32x4, v);
  }

  // activations of remainder tile j as a B operand / dot-product input: fold the G partial sums (fixed tree)
  __device__ __forceinline__ f32x4 remainder_h(const f32x4 *__restrict__ Pin, int j) const {
    const f32x4 p0 = Pin[(j * G + 0) * 64 + lane], p1 = Pin[(j * G + 1) * 64 + lane];
    const f32x4 p2 = Pin[(j * G + 2) * 64 + lane], p3 = Pin[(j * G + 3) * 64 + lane];
    f32x4 h;
#pragma unroll
    for (int r = 0; r < 4; ++r) h[r] = lrelu((p0[r] + p1[r]) + (p2[r] + p3[r]));
    return h;
  }

  // N <= 16: one wavefront, one 16x16 tile per layer, weights resident, activations never leave the registers
  // (the accumulator tile IS the next B operand).  Same canonical order as the general path with NT = 1.
  __device__ __forceinline__ float eval_tiny(float x0, float x1) {
    const int q = lane >> 4;
    f32x4 h;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const f32x4 w = W0s[4 * q + r];
      h[r] = lrelu(fmaf(w[2], x1, fmaf(w[1], x0, w[0])));
    }
#pragma unroll
    for (int l = 0; l < LMAX; ++l) {
      if (l < L) {
        f32x4 acc = *reinterpret_cast<const f32x4 *>(biasS + l * NP + 4 * q);
#pragma unroll
        for (int r = 0; r < 4; ++r) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(wres[l][r], h[r], acc, 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 4; ++r) h[r] = lrelu(acc[r]);
      }
    }
    const f32x4 w = *reinterpret_cast<const f32x4 *>(wlS + 4 * q);
    float part = 0.0f;
#pragma unroll
    for (int r = 0; r < 4; ++r) part = fmaf(w[r], h[r], part);
    const float pair = part + __shfl_xor(part, 16);
    return (pair + __shfl_xor(pair, 32)) + wlS[NP];
  }

  // N <= 16 at 64 trajectories per wavefront (one per lane, no replicated scalar work): four 16-column tiles share the
  // resident weights.  Tile c holds trajectories 16c..16c+15; its layer-0 inputs are gathered from the owning lanes with
  // ds_bpermute, and its result for column n is the value of lane 16c + n.  Per tile this is eval_tiny() -- same canonical
  // order, same bits -- and the four tiles' MFMA chains are independent, so they fill each other's latency.
  __device__ __forceinline__ float eval_tiny64(float x0, float x1) {
    const int q = lane >> 4, n = lane & 15;
    f32x4 w0[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) w0[r] = W0s[4 * q + r];
    f32x4 h[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const float a0 = __shfl(x0, 16 * c + n), a1 = __shfl(x1, 16 * c + n);
#pragma unroll
      for (int r = 0; r < 4; ++r) h[c][r] = lrelu(fmaf(w0[r][2], a1, fmaf(w0[r][1], a0, w0[r][0])));
    }
#pragma unroll
    for (int l = 0; l < LMAX; ++l) {
      if (l < L) {
        const f32x4 bias = *reinterpret_cast<const f32x4 *>(biasS + l * NP + 4 * q);
        f32x4 acc[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[c] = bias;
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
          for (int c = 0; c < 4; ++c) acc[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(wres[l][r], h[c][r], acc[c], 0, 0, 0);
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
          for (int r = 0; r < 4; ++r) h[c][r] = lrelu(acc[c][r]);
      }
    }
    const f32x4 w = *reinterpret_cast<const f32x4 *>(wlS + 4 * q);
    const float bl = wlS[NP];
    float res = 0.0f;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      float part = 0.0f;
#pragma unroll
      for (int r = 0; r < 4; ++r) part = fmaf(w[r], h[c][r], part);
      const float pair = part + __shfl_xor(part, 16);
      const float out = (pair + __shfl_xor(pair, 32)) + bl;
      if (c == q) res = out;
    }
    return res;
  }

  __device__ __forceinline__ float eval(float x0, float x1) {
    if constexpr (TINY) return eval_tiny(x0, x1);
    const int q = lane >> 4;
    constexpr int tstride = HT * 64;
    constexpr int pstride = R * G * 64;
    MSTAMP(0);  // slot 0: everything outside the MLP (RK scalar work, emission)
#if IONODE_ASM_CORE
    if constexpr (ASM) {
      if (L > 0) {
        // the whole evaluation -- Linear(2, N), the hidden stack, Linear(N, 1) -- is one asm statement (tools/gen_mlp_asm.py).
        // Inputs: per-lane LDS byte addresses of the two activation buffers (b = 0: input of even layers), the partial-sum
        // buffers, this lane's rows of the small vectors, and the wavefront's weight stream.
        constexpr unsigned HB = (unsigned)(NSETS * tstride) * 16u, PB = (unsigned)(NSETS * pstride) * 16u;  // bytes per activation / partial-sum buffer
        const unsigned hw0 = lds0 + (unsigned)(wave * 64 + lane) * 16u, hw1 = hw0 + HB;
        const unsigned fw0 = lds0 + (unsigned)((NT - 1) * 64 + lane) * 16u, fw1 = fw0 + HB;
        const unsigned pl0 = lds0 + 2u * HB + (unsigned)lane * 16u, pl1 = pl0 + PB;
        const unsigned pw0 = pl0 + (unsigned)wave * 1024u, pw1 = pl1 + (unsigned)wave * 1024u;
        const unsigned bias0 = (unsigned)(uintptr_t)biasS, w00 = (unsigned)(uintptr_t)W0s;
        const unsigned bias_a = bias0 + (unsigned)(16 * wave + 4 * q) * 4u, bias_r = bias0 + (unsigned)(16 * (NT - 1) + 4 * q) * 4u;
        const unsigned w0a = w00 + (unsigned)(16 * wave + 4 * q) * 16u, w0r = w00 + (unsigned)(16 * (NT - 1) + 4 * q) * 16u;
        const unsigned wla = (unsigned)(uintptr_t)wlS + (unsigned)q * 16u;
        const unsigned dummy = lds0 + (unsigned)scratch_off(L) + (unsigned)lane * 16u;
        const int nl = __builtin_amdgcn_readfirstlane(L);
        float out;
        if constexpr (NSETS == 1) {
          asm volatile(IONODE_MLPASM_LAYERS_13
                       : [out] "=v"(out)
                       : [hw_in] "v"(hw0), [hw_out] "v"(hw1), [fw_in] "v"(fw0), [fw_out] "v"(fw1), [pl_in] "v"(pl0), [pl_out] "v"(pl1),
                         [pw_in] "v"(pw0), [pw_out] "v"(pw1), [bias_a] "v"(bias_a), [bias_r] "v"(bias_r), [voff] "v"(voff),
                         [dummy] "v"(dummy), [w0a] "v"(w0a), [w0r] "v"(w0r), [wla] "v"(wla), [x0] "v"(x0), [x1] "v"(x1),
                         [rsrc] "s"(rsrc), [nl] "s"(nl), [lbytes] "s"(lbytes), [hid0] "s"(hid0), [wave] "s"(wave), [bl] "s"(bl_bits), [sw] "s"(sw12)
                       : "memory", "scc", "vcc", IONODE_MLPASM_CLOBBER_V_13, IONODE_MLPASM_CLOBBER_A_13, IONODE_MLPASM_CLOBBER_S_13);
        } else {
          // two column sets: this wavefront's stage inputs belong to set `wave / 2`; the stream exchanges them through LDS
          // ([set][16] x {x0, x1} behind the scratch slot) and returns the result of the own set
          const int cset = wave / (G / NSETS);
          const unsigned xch = lds0 + (unsigned)scratch_off(L) + 1024u + (unsigned)(lane & 15) * 8u;
          const unsigned xchw = xch + (unsigned)cset * 128u;
          const int own_h = cset * (int)(tstride * 16), own_p = cset * (int)(pstride * 16);
          asm volatile(IONODE_MLPASM_LAYERS_13x2
                       : [out] "=v"(out)
                       : [hw_in] "v"(hw0), [hw_out] "v"(hw1), [fw_in] "v"(fw0), [fw_out] "v"(fw1), [pl_in] "v"(pl0), [pl_out] "v"(pl1),
                         [pw_in] "v"(pw0), [pw_out] "v"(pw1), [bias_a] "v"(bias_a), [bias_r] "v"(bias_r), [voff] "v"(voff),
                         [dummy] "v"(dummy), [w0a] "v"(w0a), [w0r] "v"(w0r), [wla] "v"(wla), [x0] "v"(x0), [x1] "v"(x1),
                         [xchw] "v"(xchw), [xchr] "v"(xch),
                         [rsrc] "s"(rsrc), [nl] "s"(nl), [lbytes] "s"(lbytes), [hid0] "s"(hid0), [wave] "s"(wave), [bl] "s"(bl_bits), [sw] "s"(sw12),
                         [own_h] "s"(own_h), [own_p] "s"(own_p)
                       : "memory", "scc", "vcc", IONODE_MLPASM_CLOBBER_V_13x2, IONODE_MLPASM_CLOBBER_A_13x2, IONODE_MLPASM_CLOBBER_S_13x2);
        }
        MSTAMP(3);  // slot 3: the whole evaluation (asm stream)
        return out;
      }
    }
#endif

    // layer 0: Linear(2, N) + LeakyReLU on the VALU, written in accumulator layout; row tile rt by wavefront rt % G.
    // hOwn = this wavefront's tile `wave`: the k-tile it consumes at step 0 of the next layer ((0 + w) mod NT).
    // That B operand is taken from registers, which lets the layer barrier sit AFTER step 0: the LDS store -> barrier ->
    // load round trip of the activations and the wait for the slowest wavefront overlap with step 0's MFMAs.
    f32x4 hOwn = f32x4{0, 0, 0, 0};
#pragma unroll
    for (int i = 0; i < RT; ++i) {
      const int rt = wave + i * G;
      if (rt < NT) {
        f32x4 h;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const f32x4 w = W0s[16 * rt + 4 * q + r];
          h[r] = lrelu(fmaf(w[2], x1, fmaf(w[1], x0, w[0])));
        }
        if (i == 0) hOwn = h;
        Hs[rt * 64 + lane] = h;
        if (rt < G - 1) Hs[(rt + NT) * 64 + lane] = h;
      }
    }
    MSTAMP(1);  // slot 1: layer 0

    if constexpr (!ASM)  // (the asm tile comes here only with L == 0)
    for (int l = 0; l < L; ++l) {
      f32x4 *__restrict__ Hin = Hs + (l & 1) * tstride;
      f32x4 *__restrict__ Hout = Hs + ((l + 1) & 1) * tstride;
      const f32x4 *__restrict__ Pin = Ps + (l & 1) * pstride;
      f32x4 *__restrict__ Pout = Ps + ((l + 1) & 1) * pstride;
      const int ln = (l + 1 < L) ? l + 1 : 0;  // the ring runs cyclically over the hidden stack
      // (L == 1 simply re-streams the same layer: a runtime 'resident' branch around the refills would make
      // hipcc's wait-count pass lose the age of the loads and drain them all at every use)
      const unsigned lcur = hid0 + (unsigned)l * lbytes, lnext = hid0 + (unsigned)ln * lbytes;

      // B operands of the remainder k-tiles: layer 0 wrote them as ordinary tiles; hidden layers leave partial sums,
      // which every wavefront folds into the remainder slots of the input buffer itself (identical bits from all
      // wavefronts; each reads after its own write, so no barrier).  The fold is needed first at step G*F - wave;
      // when that is late enough it runs behind the MFMAs of step 0 instead of in the layer prologue.
      constexpr bool LAZY_FOLD = (R > 0) && !OWNREM && (G * F - (G - 1) >= 3);
      f32x4 acc[F > 0 ? F : 1], accr[RP];
#pragma unroll
      for (int i = 0; i < F; ++i)
        acc[i] = *reinterpret_cast<const f32x4 *>(biasS + l * NP + 16 * (wave + i * G) + 4 * q);
      f32x4 pc[OWNREM ? 4 : 1];   // OWNREM: the four partial chains of my remainder tile
      f32x4 bn_nxt = f32x4{0, 0, 0, 0};
      if constexpr (OWNREM) {
        pc[0] = *reinterpret_cast<const f32x4 *>(biasS + l * NP + 16 * (G * F + (wave < R ? wave : 0)) + 4 * q);  // chain 0 carries the bias
        pc[1] = pc[2] = pc[3] = f32x4{0, 0, 0, 0};
      } else {
#pragma unroll
      for (int j = 0; j < R; ++j) {
        const f32x4 bz = *reinterpret_cast<const f32x4 *>(biasS + l * NP + 16 * (G * F + j) + 4 * q);
        accr[j] = (wave == 0) ? bz : f32x4{0, 0, 0, 0};  // partial sum 0 carries the bias
      }
      }
      for (int kt0 = 0; kt0 < NT; kt0 += PD) {
        static_assert(R == 0 || PD == NT, "remainder tiles need the full-layer ring (static step index)");
        const bool same_layer = kt0 + PD < NT;
        // stream position of the refills issued in this block: same layer, PD steps ahead, or the next layer's start
        const unsigned lref = same_layer ? lcur + (unsigned)step_base(kt0 + PD) * 1024u : lnext;
        // this wavefront's k-tile at step kt0 + u is (kt0 + u + wave) mod NT = slot kt0 + u + wave of the buffer
        const f32x4 *__restrict__ Bw = Hin + (kt0 + wave) * 64 + lane;
        f32x4 b_nxt = hOwn;                      // step 0 of the layer: own tile, from registers (before the barrier)
        if (kt0 > 0) b_nxt = Bw[0];
        MSTAMP(8);  // slot 8: layer prologue (bias)
#pragma unroll
        for (int u = 0; u < PD; ++u) {
          if (u == 1) MSTAMP(9);       // slot 9: first k-tile (+ barrier)
          if (u == PD - 1) MSTAMP(3);  // slot 3: k-tiles 1..PD-2
          const f32x4 b = b_nxt;
          // LDS read one step ahead, immediate offset -- except across the layer barrier (after step 0)
          if (u + 1 < PD && !(u == 0 && kt0 == 0)) b_nxt = Bw[(u + 1) * 64];
          // K-slice ownership: static, except that the last owned step wraps past NT for the higher wavefronts
          const bool own_static = (R > 0) && !OWNREM && (u % G == 0);
          // OWNREM: my remainder tile's chain (u - 1) % 4 takes k-tile u - 1 (natural order, one step behind: k-tile 0 is another
          // wavefront's tile and exists only behind the layer barrier, which sits at the end of step 0)
          f32x4 bn = bn_nxt;
          if constexpr (OWNREM) {
            if (u >= 1) bn_nxt = Hin[u * 64 + lane];
          }
          const bool own_always = own_static && (u + G - 1 < NT);
          const bool own = own_static && (own_always || (u + wave < NT));
#pragma unroll
          for (int r = 0; r < 4; ++r) {
#pragma unroll
            for (int i = 0; i < F; ++i) {
              const int e = r * F + i;
              acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(ring[u][e / 4][e % 4], b[r], acc[i], 0, 0, 0);
            }
            if constexpr (!OWNREM) {
            if (own_static) {
              if (own) {
#pragma unroll
                for (int j = 0; j < R; ++j)
                  accr[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(rrem[u / G][j][r], b[r], accr[j], 0, 0, 0);
              }
            }
            } else {
              if (u >= 1) {   // (every wavefront, also the one without a remainder tile: a wave-dependent branch around the
                              // refills makes hipcc drain every load at every use -- 29.8 -> 48.8 ms; it computes tile 0 again, unused)
                pc[(u - 1) % G] = __builtin_amdgcn_mfma_f32_16x16x4f32(rown[u - 1][r], bn[r], pc[(u - 1) % G], 0, 0, 0);
                if (r == 3) rown[u - 1] = frag_of(lref, u - 1);
              }
            }
            // refill every fragment whose last reader was this k-step; pinned here (see header comment)
#pragma unroll
            for (int j = 0; j < F; ++j)
              if ((4 * j + 3) / F == r) ring[u][j] = frag(lref, step_base(u) + j);
            if constexpr (!OWNREM) {
            if (own_static && r == 3) {
#pragma unroll
              for (int j = 0; j < R; ++j) rrem[u / G][j] = frag(lref, step_base(u) + F + j);
            }
            }
            if (LAZY_FOLD && u == 1 && r == 0 && l > 0) {
#pragma unroll
              for (int j = 0; j < R; ++j) Hin[(G * F + j) * 64 + lane] = remainder_h(Pin, j);
            }
            __builtin_amdgcn_sched_barrier(0);
          }
          if (u == 0 && kt0 == 0) {
            // ---- the layer barrier: everybody's activations / partial sums of the previous layer are in LDS ----
            if (G > 1) __syncthreads();
            if (R > 0 && !OWNREM && !LAZY_FOLD && l > 0) {
#pragma unroll
              for (int j = 0; j < R; ++j) Hin[(G * F + j) * 64 + lane] = remainder_h(Pin, j);
            }
            if (PD > 1) b_nxt = Bw[64];
            if constexpr (OWNREM) {
              bn_nxt = Hin[lane];   // k-tile 0 for my remainder chains (step 1)
            }
            __builtin_amdgcn_sched_barrier(0);
          }
        }
      }
      if constexpr (OWNREM) {
        const f32x4 bn = bn_nxt;   // k-tile NT - 1
#pragma unroll
        for (int r = 0; r < 4; ++r) pc[(NT - 1) % G] = __builtin_amdgcn_mfma_f32_16x16x4f32(rown[NT - 1][r], bn[r], pc[(NT - 1) % G], 0, 0, 0);
        rown[NT - 1] = frag_of(lnext, NT - 1);
        f32x4 h;
#pragma unroll
        for (int r = 0; r < 4; ++r) h[r] = lrelu((pc[0][r] + pc[1][r]) + (pc[2][r] + pc[3][r]));  // the canonical combine tree
        if (wave < R) Hout[(G * F + wave) * 64 + lane] = h;
      }
      MSTAMP(10);  // slot 10: last k-tile
#pragma unroll
      for (int i = 0; i < F; ++i) {
        f32x4 h;
#pragma unroll
        for (int r = 0; r < 4; ++r) h[r] = lrelu(acc[i][r]);
        if (i == 0) hOwn = h;
        Hout[(wave + i * G) * 64 + lane] = h;
        if (wave + i * G < G - 1) Hout[(wave + i * G + NT) * 64 + lane] = h;
      }
      if constexpr (!OWNREM) {
#pragma unroll
      for (int j = 0; j < R; ++j) Pout[(j * G + wave) * 64 + lane] = accr[j];
      }
      MSTAMP(4);  // slot 4: LeakyReLU + activation store
    }
    if (G > 1) __syncthreads();  // the last hidden layer's (or layer 0's) activations for the output layer
    MSTAMP(2);

    // Linear(N, 1) on the VALU: four partial fmaf chains (one per lane group q), fixed combine tree
    const f32x4 *__restrict__ Hin = Hs + (L & 1) * tstride;
    const f32x4 *__restrict__ Pin = Ps + (L & 1) * pstride;
    float part = 0.0f;
    // (issuing the LDS reads of several steps together was measured: no change at N = 200 / 100, -2 % at N = 500 -- the four wavefronts
    // run this chain redundantly and its stalls overlap; the 4-trajectory tile, one chain per evaluation on the critical path, does it)
#pragma unroll
    for (int kt = 0; kt < NT; ++kt) {
      const f32x4 w = *reinterpret_cast<const f32x4 *>(wlS + 16 * kt + 4 * q);
      f32x4 h;
      if (R > 0 && !OWNREM && kt >= G * F && L > 0) h = remainder_h(Pin, kt - G * F);
      else h = Hin[kt * 64 + lane];
#pragma unroll
      for (int r = 0; r < 4; ++r) part = fmaf(w[r], h[r], part);
    }
    const float pair = part + __shfl_xor(part, 16);   // (p0 + p1) or (p2 + p3)
    const float out = (pair + __shfl_xor(pair, 32)) + wlS[NP];
    if (G > 1 && (L & 1) == 0) __syncthreads();  // next evaluation's layer 0 rewrites buffer 0
    MSTAMP(5);  // slot 5: last layer
    return out;
  }
};

}  // namespace ionode
