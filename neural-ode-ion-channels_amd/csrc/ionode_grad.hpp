// ionode_grad.hpp -- gfx950 device code of the BACKWARD sweep through a dopri5 solve (BASELINE config 5).
//
// What is differentiated.  The reference never takes this gradient (its --adjoint flag only switches an import,
// train-s1.py:29-32), so there is no reference behaviour to mirror: the sweep is the exact reverse-mode derivative of the
// discretisation the forward kernel executed -- the accepted steps (t0, dt) are constants ("discretise-then-optimise",
// controller frozen), rejected attempts contribute nothing, FSAL (k1 of a step is k7 of its predecessor) and the 4th-order
// dense output are differentiated as written in ionode_device.hpp.  Checker: autograd through a torch restatement replaying
// the same step sequence (tests/grad_check.py); the scalar algebra below is `manual_adjoint()` of that file.
//
// Execution model.  One workgroup = one tile of 16 trajectories, 4 wavefronts, lane = 16q + j holds trajectory j
// (replicated over q and over the wavefronts, as in the forward kernel).  The tile walks its trajectories' ACCEPTED steps
// backwards in lock-step (iteration `it`: trajectory j processes its step nacc_j - 1 - it, then one extra MLP evaluation
// for k1 = f(t[0], y0) of its first step, then idles).  The forward launch left one checkpoint per accepted step
// (ionode_desc.ckpt: t0, dt, output range, y, k1..k7), so every stage input Y_i = y + dt * sum_j beta_ij k_j is rebuilt
// without re-running earlier stages.  Per step: the output gradients of the step's dense-output samples are reduced
// cooperatively into the 5 x D interpolant-coefficient adjoints, then six MLP vector-Jacobian products (stages 6..1) follow.
//
// MLP vector-Jacobian product on the fp32 MFMA.  Forward recompute h_0..h_L (all layers kept in LDS), then
// d_{l-1} = (W_l^T d_l) * lrelu'(h_{l-1}) with the TRANSPOSED weight fragments of the grad image (ionode_grad_pack), same
// 16x16x4 tiles and the same k-permutation as the forward kernel (register r of lane group q of tile kt is k = 16kt+4q+r),
// so accumulator tiles are B operands without a transpose in both directions.
//
// Weight gradients.  dW_l = sum over (trajectory, step, stage) of d_l h_{l-1}^T has 5 x 208 x 208 accumulators per tile
// (865 KB for s00): more than a CU's registers + LDS.  The sweep therefore STREAMS (d_l, h_l) tiles to HBM (160 KB per tile
// evaluation; 288 GB of HBM3E hold tens of thousands of steps per tile, and the host chunks the sweep over iterations when
// it does not fit) and a second kernel (ionode_grad_reduce, whole chip, split-K fp32 MFMA GEMM) contracts them.
#pragma once

#include <type_traits>

#include "ionode_grad_step.hpp"   // GArgs and the layouts of the streams between the launches
#include "ionode_interp.hpp"      // the forward's dense-output interpolant and observation model

namespace ionode {

__host__ __device__ constexpr size_t grad_lds_bytes(int L, int NT) {
  // two activation buffers + two gradient buffers (ping-pong over the layers, whatever L is) + remainder partial sums + small vectors
  // (+ the input layer's second weight column as a contiguous vector: the closing dot product d net / d x1)
  return ((size_t)4 * NT * 64 + (size_t)2 * (NT % 4) * 4 * 64 + 16 * NT) * 16 + ((size_t)L * 16 * NT + 16 * NT + 4) * 4 + 16 * 10 * 8 + (NT <= 13 ? (size_t)16 * NT * 4 : 0);   // (N = 500 with 10 layers fills the 160 KiB without it)
}
// One call per compiled width NT = N padded to 16, 112, 208 or 512 (architectures/s00-s11.py: N = 10, 100, 200, 500):
// f(std::integral_constant<int, NT>) for the units' own widths, f32() for N = 500 (instantiated in inst_grad32.hip); false: no such variant.
template <typename F, typename F32> bool for_width(int NT, F f, F32 f32) {
  switch (NT) {
    case 1: f(std::integral_constant<int, 1>{}); return true;
    case 7: f(std::integral_constant<int, 7>{}); return true;
    case 13: f(std::integral_constant<int, 13>{}); return true;
    case 32: f32(); return true;
    default: return false;
  }
}

template <typename Kern> void raise_lds_limit(Kern kern, size_t lds) {
  if (lds > 64 * 1024)
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
}

// image offsets (floats): rows of layer 0 {b0, w00, w01, 0} | hidden biases | wl, bl | forward fragments | transposed fragments
__host__ __device__ constexpr size_t grad_img_bias(int NT) { return (size_t)4 * 16 * NT; }
__host__ __device__ constexpr size_t grad_img_wl(int L, int NT) { return grad_img_bias(NT) + (size_t)L * 16 * NT; }
__host__ __device__ constexpr size_t grad_img_fwd(int L, int NT) { return grad_img_wl(L, NT) + 16 * NT + 4; }
__host__ __device__ constexpr size_t grad_img_bwd(int L, int NT) { return grad_img_fwd(L, NT) + (size_t)L * NT * NT * 256; }
__host__ __device__ constexpr size_t grad_img_floats(int L, int NT) { return grad_img_bwd(L, NT) + (size_t)L * NT * NT * 256; }

template <int NT>
struct GradMlp {
  static constexpr int G = 4;
  static constexpr int F = NT / G;                // full row tiles per wavefront (rt = wave + 4i, every k-tile)
  static constexpr int R = NT - G * F;            // remainder row tiles (rt = 4F + j): their k-tiles are dealt over the wavefronts
  static constexpr int NOWN = (NT + G - 1) / G;   // k-tiles of a remainder tile one wavefront owns (kt = wave + 4u)
  static constexpr int FP = F > 0 ? F : 1, RP = R > 0 ? R : 1;
  static constexpr int NP = 16 * NT;
  // Work split as in the forward kernel: every wavefront runs F full row tiles over all NT k-tiles and a 1/4 K-slice of each
  // remainder row tile (partial sums meet in LDS, every wavefront folds them itself behind the layer barrier): 172 MFMAs per
  // product on every wavefront for N = 200 instead of 208 on wavefront 0.  Wavefront w walks the k-tiles in the rotated order
  // kt = (s + w) mod NT so that "this step carries my K-slice" is the static predicate s % 4 == 0 (and s + w < NT).
  //
  // Weight fragments are consumed from a register ring one product deep that runs AHEAD of the MFMAs across product boundaries
  // (forward layers 0..L-1, transposed layers L-1..0, then the next evaluation's layer 0): a fragment is re-loaded right behind
  // the MFMAs that read it, so an L2 round trip (~1 us under load, ~5 k-tiles of MFMA time) is covered.  Without the ring every
  // k-tile waited for its own loads: 18 us per product instead of the 6.7k-cycle MFMA floor (measured).
  // N = 500 (NT = 32: 8 full row tiles per wavefront, no remainder) cannot hold a whole product's fragments (1024 registers):
  // there the ring is PD = 4 k-tiles deep and is refilled from the SAME product until its last PD steps (the forward
  // kernel's blocked ring for s06-s08).
  static constexpr int PD = (NT <= 13) ? NT : 4;
  static_assert(R == 0 || PD == NT, "remainder tiles need the full-product ring (static step index)");
  f32x4 ringF[PD][FP];
  f32x4 ringR[NOWN][RP];
  f32x4 *Hs;          // LDS [2][NT*64]     activations after LeakyReLU, accumulator layout, ping-pong over layers (layer l in
                      //                    buffer l & 1); the backward pass needs only their signs, kept as bits in registers
  f32x4 *Ds;          // LDS [2][NT*64]     pre-activation gradients, ping-pong over layers
  f32x4 *Ps;          // LDS [2][R][G][64]  partial sums of the remainder row tiles, ping-pong over products
  const f32x4 *W0s;   // LDS [NP] {b0, w00, w01, 0}
  const float *biasS; // LDS [L][NP]
  const float *wlS;   // LDS [NP] + bl
  const float *w01S;  // LDS [NP]: W0[k][1]
  __amdgpu_buffer_rsrc_t rsrc;
  unsigned fwd0, bwd0;  // byte offsets of the fragment sections
  int L, wave, lane;
  int roff;           // this lane's float offset inside a record tile (rec_store)

  __device__ __forceinline__ void init(const GArgs &a, unsigned char *smem, int wave_, int lane_) {
    L = a.k.L; wave = wave_; lane = lane_;
    roff = 64 * (lane & 3) + 16 * (lane >> 4) + ((lane & 15) >> 2);
    Hs = reinterpret_cast<f32x4 *>(smem);
    Ds = Hs + (size_t)2 * NT * 64;
    Ps = Ds + 2 * NT * 64;
    f32x4 *w0 = Ps + 2 * R * G * 64;
    float *bs = reinterpret_cast<float *>(w0 + NP);
    float *ws = bs + (size_t)L * NP;
    const int tid = wave * 64 + lane;
    const f32x4 *src = reinterpret_cast<const f32x4 *>(a.img);
    for (int i = tid; i < NP; i += 64 * G) w0[i] = src[i];
    for (int i = tid; i < L * NP; i += 64 * G) bs[i] = a.img[grad_img_bias(NT) + i];
    for (int i = tid; i < NP + 4; i += 64 * G) ws[i] = a.img[grad_img_wl(L, NT) + i];
    W0s = w0; biasS = bs; wlS = ws;
    // w01[k] = W0[k][1] contiguous (13 x 16-byte reads in the closing dot product instead of 52 rows of {b0, w00, w01, 0})
    if constexpr (NT <= 13) {
      float *w01 = reinterpret_cast<float *>(reinterpret_cast<double *>(ws + NP + 4) + 16 * 10);
      for (int i = tid; i < NP; i += 64 * G) w01[i] = a.img[4 * i + 2];
      w01S = w01;
    }
    rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(a.img), 0, (int)(grad_img_floats(L, NT) * 4), 0x00020000);
    fwd0 = (unsigned)(grad_img_fwd(L, NT) * 4);
    bwd0 = (unsigned)(grad_img_bwd(L, NT) * 4);
    refill_all(fwd0, 0);  // prime: first product of the first evaluation
    __syncthreads();
  }
  __device__ __forceinline__ int ktile(int s) const { return (s + wave) % NT; }  // wave-uniform (scalar ALU)
  __device__ __forceinline__ int own_kt(int u) const { const int k = wave + G * u; return k < NT ? k : NT - 1; }  // clamped: never read past the layer
  // LeakyReLU'(h) per layer as bits
  static constexpr int MAXL = 15;
  static __device__ __forceinline__ unsigned bits_of(const f32x4 &h) {
    return (h[0] > 0.0f ? 1u : 0u) | (h[1] > 0.0f ? 2u : 0u) | (h[2] > 0.0f ? 4u : 0u) | (h[3] > 0.0f ? 8u : 0u);
  }
  // BITS per layer: 4 per owned full tile, then 4 per remainder tile (16 for N <= 208, 32 for N = 500); layers 0..15
  static constexpr int BITS = (4 * (F + R) <= 16) ? 16 : 32;
  static_assert(4 * (F + R) <= BITS, "sign bits of one layer");
  struct Signs {  // 64-bit words, 64 / BITS layers each; scalar members (no indexed array: that would live in scratch)
    static constexpr int PER = 64 / BITS;
    unsigned long long w0 = 0, w1 = 0, w2 = 0, w3 = 0, w4 = 0, w5 = 0, w6 = 0, w7 = 0;
    // Pure mask arithmetic: a chain of selects over the members is folded by hipcc into ONE load with a selected address, which
    // pins the struct in scratch (72 B per lane in round 2's N = 500 builds; 40 B in the N <= 16 builds once the words are passed
    // by reference); and/or on values cannot be.
    static __device__ __forceinline__ unsigned long long on(int k, int i) { return (k == i) ? ~0ull : 0ull; }
    __device__ __forceinline__ void put(int l, unsigned bits) {
      const int sh = (l % PER) * BITS;
      const unsigned long long full = (BITS == 32) ? 0xffffffffull : 0xffffull;
      const unsigned long long m = ~(full << sh), v = (unsigned long long)bits << sh;
      const int k = l / PER;
      w0 = (w0 & (m | ~on(k, 0))) | (v & on(k, 0));
      w1 = (w1 & (m | ~on(k, 1))) | (v & on(k, 1));
      w2 = (w2 & (m | ~on(k, 2))) | (v & on(k, 2));
      w3 = (w3 & (m | ~on(k, 3))) | (v & on(k, 3));
      if constexpr (PER < 4) {
        w4 = (w4 & (m | ~on(k, 4))) | (v & on(k, 4));
        w5 = (w5 & (m | ~on(k, 5))) | (v & on(k, 5));
        w6 = (w6 & (m | ~on(k, 6))) | (v & on(k, 6));
        w7 = (w7 & (m | ~on(k, 7))) | (v & on(k, 7));
      }
    }
    __device__ __forceinline__ unsigned get(int l) const {
      const int k = l / PER;
      unsigned long long w = (w0 & on(k, 0)) | (w1 & on(k, 1)) | (w2 & on(k, 2)) | (w3 & on(k, 3));
      if constexpr (PER < 4) w |= (w4 & on(k, 4)) | (w5 & on(k, 5)) | (w6 & on(k, 6)) | (w7 & on(k, 7));
      const unsigned long long full = (BITS == 32) ? 0xffffffffull : 0xffffull;
      return (unsigned)((w >> ((l % PER) * BITS)) & full);
    }
  };
  __device__ __forceinline__ void refill_all(unsigned sec, int l) {
#pragma unroll
    for (int s = 0; s < PD; ++s)
#pragma unroll
      for (int i = 0; i < F; ++i) ringF[s][i] = frag(sec, l, wave + G * i, ktile(s));
#pragma unroll
    for (int u = 0; u < NOWN; ++u)
#pragma unroll
      for (int j = 0; j < R; ++j) ringR[u][j] = frag(sec, l, G * F + j, own_kt(u));
  }
  __device__ __forceinline__ double *gs() const {  // LDS [16][10] fp64 scratch behind the small vectors (8-byte aligned)
    return reinterpret_cast<double *>(const_cast<float *>(wlS) + NP + 4);
  }

  __device__ __forceinline__ f32x4 frag(unsigned sec, int l, int rt, int kt) const {
    using u32x4 = __attribute__((ext_vector_type(4))) unsigned;
    const unsigned off = sec + (unsigned)(((l * NT + rt) * NT + kt) * 1024);
    const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rsrc, (unsigned)lane * 16u, off, 0);
    return __builtin_bit_cast(f32x4, v);
  }

  // Record tiles are stored in the A/B-operand layout of ionode_grad_reduce's MFMAs (contraction over the 16 trajectories):
  // G[16*kk + m][c] = X[row 16*rt + m][trajectory 4*c + kk].  This lane holds rows 4q + r of trajectory n = lane & 15.
  // NT: non-temporal (written once, read once by ionode_grad_reduce: the stream then does not evict the weight image from L2) --
  // the regression step and the one-phase sweep; the two-phase kernels store ordinarily (L2 write-back merges the four 16-byte
  // pieces of a sector before they leave: walk 0.470 -> 0.459 s; the regression step loses 1 % with it)
  template <bool NTS = true>
  __device__ __forceinline__ void rec_store(f32x4 *tile, const f32x4 &v) const {
    float *p = reinterpret_cast<float *>(tile) + roff;   // 64 * (n & 3) + 16 * q + (n >> 2), q = lane >> 4, n = lane & 15
    if constexpr (NTS) {
      __builtin_nontemporal_store(v[0], p); __builtin_nontemporal_store(v[1], p + 4);
      __builtin_nontemporal_store(v[2], p + 8); __builtin_nontemporal_store(v[3], p + 12);
    } else {
      p[0] = v[0]; p[4] = v[1]; p[8] = v[2]; p[12] = v[3];
    }
  }

  // accF[i] += A(csec, cl)[row tile wave + 4i][:] . B[:] over all k-tiles; accR[j] += the owned K-slice of remainder tile j.
  // B is read from LDS in accumulator layout.  (nsec, nl): the product that follows -- its fragments replace this one's
  // right behind the MFMAs that read them (PD == NT); with the short ring the steps s + PD < NT of THIS product come first.
  // The workgroup barrier between two products is NOT in front of this one: step 0's B operand is the wavefront's own first
  // tile (k-tile `wave` of the rotated walk), handed over in registers (`own`), and `after0` -- the barrier, then whatever had
  // to wait for it (the fold of the previous product's remainder tile) -- runs BEHIND step 0's MFMAs, so the LDS round trip
  // and the wait for the slowest wavefront overlap with them (the forward kernel's arrangement, ionode_device.hpp).  Widths
  // without a full tile per wavefront (N <= 48) run `after0` first and read every operand from LDS.
  static constexpr bool OWN0 = (F >= 1);
  // SCHED: what may cross the end of a k-tile step in hipcc's scheduler (sched_barrier mask).  0: nothing -- the refills stay where
  // they are issued.  (0xF -- ALU and MFMA may, memory operations may not -- gained 3.5 % where only backward products ran and
  // loses 5.8 % on the regression step: 1.94 -> 2.05 ms.)
  template <int SCHED, typename After0>
  __device__ __forceinline__ void product(unsigned csec, int cl, unsigned nsec, int nl, const f32x4 *__restrict__ B, const f32x4 &own,
                                          After0 after0, f32x4 (&accF)[FP], f32x4 (&accR)[RP]) {
    // the B operand of step s + 1 is read from LDS before the MFMAs of step s (the sched_barrier at the end of a step would
    // otherwise pin every read directly in front of its MFMAs: ~100 cycles of LDS latency per step, 13 steps per product)
    f32x4 b_nxt;
    if constexpr (OWN0) b_nxt = own;
    else { after0(); b_nxt = B[ktile(0) * 64 + lane]; }
#pragma unroll
    for (int s = 0; s < NT; ++s) {
      const int kt = ktile(s);
      const f32x4 b = b_nxt;
      if (s + 1 < NT && !(OWN0 && s == 0)) b_nxt = B[ktile(s + 1) * 64 + lane];
      // k-step outer, row tile inner: consecutive MFMAs go to different accumulators (issue every 32 cycles, result after 40)
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int i = 0; i < F; ++i) accF[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(ringF[s % PD][i][r], b[r], accF[i], 0, 0, 0);
      if (R > 0 && s % G == 0) {
        if (s + G - 1 < NT || s + wave < NT) {  // static for every step but the last owned one (wave-uniform there)
#pragma unroll
          for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int j = 0; j < R; ++j) accR[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(ringR[s / G][j][r], b[r], accR[j], 0, 0, 0);
        }
#pragma unroll
        for (int j = 0; j < R; ++j) ringR[s / G][j] = frag(nsec, nl, G * F + j, own_kt(s / G));
      }
#pragma unroll
      for (int i = 0; i < F; ++i) {
        if constexpr (PD == NT) ringF[s][i] = frag(nsec, nl, wave + G * i, kt);
        else ringF[s % PD][i] = (s + PD < NT) ? frag(csec, cl, wave + G * i, ktile(s + PD)) : frag(nsec, nl, wave + G * i, ktile(s + PD - NT));
      }
      if constexpr (OWN0) {
        if (s == 0) {
          after0();
          if (NT > 1) b_nxt = B[ktile(1) * 64 + lane];
        }
      }
      __builtin_amdgcn_sched_barrier(SCHED);  // keep the refills here (hipcc otherwise sinks them behind the product)
    }
  }

  // fold the four K-slices of remainder tile j (fixed tree)
  __device__ __forceinline__ f32x4 fold(const f32x4 *__restrict__ P, int j) const {
    const f32x4 p0 = P[(j * G + 0) * 64 + lane], p1 = P[(j * G + 1) * 64 + lane];
    const f32x4 p2 = P[(j * G + 2) * 64 + lane], p3 = P[(j * G + 3) * 64 + lane];
    f32x4 z;
#pragma unroll
    for (int r = 0; r < 4; ++r) z[r] = (p0[r] + p1[r]) + (p2[r] + p3[r]);
    return z;
  }

  // One vector-Jacobian product of the net for the 16 trajectories of the tile, all four wavefronts together.
  // x = (V/100, a) as the forward casts them, seed = adjoint of the net output.  Returns seed * d net / d x1.
  // rec != NULL: the (h_l, d_l) tiles and the scalars of this evaluation are streamed there for ionode_grad_reduce.
  template <bool NTS = true>
  __device__ __forceinline__ float vjp(float x0, float x1, float seed, float *__restrict__ rec) {
    auto fn = [seed](float) -> float { return seed; };
    return vjp_from_output<decltype(fn), NTS>(x0, x1, rec, fn);
  }
  // The same product with the seed computed from the net's output: seed = seed_of(net([x0, x1])) per lane (regression:
  // d loss / d net).  The output layer runs only when the functor needs it; a constant functor leaves it out.
  // NTS: non-temporal record stores (rec_store)
  template <typename SeedFn, bool NTS = true>
  __device__ __forceinline__ float vjp_from_output(float x0, float x1, float *__restrict__ rec, SeedFn seed_of) {
    Signs mk;
    const int q = lane >> 4;
    f32x4 *__restrict__ recH = reinterpret_cast<f32x4 *>(rec);
    f32x4 *__restrict__ recD = recH + (size_t)(L + 1) * NT * 64;
    constexpr int pstride = R * G * 64;
    int par = 0;  // partial-sum buffer of the running product
    // ---- forward recompute.  The activations of layer l live in LDS buffer l & 1 (the next layer's B operand) and go to the
    // record stream as they are produced; what the backward pass needs of them afterwards is the sign, kept here ----
    float seed = 0.0f;
    f32x4 own = f32x4{0, 0, 0, 0};   // this wavefront's first tile of the running activation / gradient: B operand of the next product's step 0
    {
    auto layer0 = [&](int rt) {
      f32x4 h;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const f32x4 w = W0s[16 * rt + 4 * q + r];
        h[r] = lrelu(fmaf(w[2], x1, fmaf(w[1], x0, w[0])));
      }
      return h;
    };
    {
      // Layer 0: full-tile slots rt = wave + 4 i by their owner; remainder tiles evaluated by EVERY wavefront (all of them need
      // the signs when they fold d_0), stored by wavefront j
      unsigned b16 = 0u;
#pragma unroll
      for (int i = 0; i < F; ++i) {
        const int rt = wave + G * i;
        const f32x4 h = layer0(rt);
        b16 |= bits_of(h) << (4 * i);
        Hs[rt * 64 + lane] = h;
        if (i == 0) own = h;
        if (rec) rec_store<NTS>(recH + rt * 64, h);
      }
#pragma unroll
      for (int j = 0; j < R; ++j) {
        const int rt = G * F + j;
        const f32x4 h = layer0(rt);
        b16 |= bits_of(h) << (4 * (F + j));
        if (wave == j) {
          Hs[rt * 64 + lane] = h;
          if (rec) rec_store<NTS>(recH + rt * 64, h);
        }
      }
      mk.put(0, b16);
    }
    bool pend = false;     // the previous layer's remainder tiles are still partial sums in Ps (folded behind the next barrier)
    unsigned b16p = 0u;    // ... and the sign bits of that layer's full tiles wait for theirs
    for (int l = 1; l <= L; ++l) {
      f32x4 accF[FP], accR[RP];
#pragma unroll
      for (int i = 0; i < F; ++i) accF[i] = *reinterpret_cast<const f32x4 *>(biasS + (l - 1) * NP + 16 * (wave + G * i) + 4 * q);
#pragma unroll
      for (int j = 0; j < R; ++j) {
        const f32x4 bz = *reinterpret_cast<const f32x4 *>(biasS + (l - 1) * NP + 16 * (G * F + j) + 4 * q);
        accR[j] = (wave == 0) ? bz : f32x4{0, 0, 0, 0};  // partial sum 0 carries the bias
      }
      // (the product behind this one: the next forward layer; behind the last: the first backward product, or -- recompute
      // kernel -- the next evaluation's first forward layer)
      // the layer barrier; behind it every wavefront folds the previous layer's remainder tiles itself and writes the (identical)
      // activations into that layer's slot -- each reads them back only after its own write, so no second barrier; wavefront 0
      // also streams the record
      auto fold_prev = [&](int lp) {   // lp: the layer whose partial sums wait in Ps[par ^ 1]
        __syncthreads();
        if (R > 0 && pend) {
          f32x4 *__restrict__ Hp = Hs + (size_t)(lp & 1) * NT * 64;
          unsigned b16 = b16p;
#pragma unroll
          for (int j = 0; j < R; ++j) {
            const f32x4 z = fold(Ps + (par ^ 1) * pstride, j);
            f32x4 h;
#pragma unroll
            for (int r = 0; r < 4; ++r) h[r] = lrelu(z[r]);
            b16 |= bits_of(h) << (4 * (F + j));
            Hp[(G * F + j) * 64 + lane] = h;
            if (rec && wave == 0) rec_store<NTS>(recH + ((size_t)lp * NT + G * F + j) * 64, h);
          }
          mk.put(lp, b16);
        }
      };
      // (the product behind this one: the next forward layer; behind the last: the first backward product)
      product<0>(fwd0, l - 1, l < L ? fwd0 : bwd0, l < L ? l : L - 1, Hs + (size_t)((l - 1) & 1) * NT * 64,
              own, [&] { fold_prev(l - 1); }, accF, accR);
      f32x4 *__restrict__ Hl = Hs + (size_t)(l & 1) * NT * 64;
      unsigned b16 = 0u;
#pragma unroll
      for (int i = 0; i < F; ++i) {
        const int rt = wave + G * i;
        f32x4 h;
#pragma unroll
        for (int r = 0; r < 4; ++r) h[r] = lrelu(accF[i][r]);
        b16 |= bits_of(h) << (4 * i);
        Hl[rt * 64 + lane] = h;
        if (i == 0) own = h;
        if (rec) rec_store<NTS>(recH + ((size_t)l * NT + rt) * 64, h);
      }
#pragma unroll
      for (int j = 0; j < R; ++j) Ps[par * pstride + (j * G + wave) * 64 + lane] = accR[j];
      if (R > 0) { pend = true; b16p = b16; } else mk.put(l, b16);
      par ^= 1;
      if (l == L) fold_prev(L);   // behind the last layer: nothing to hide the barrier behind
    }
    if (L == 0) __syncthreads();
    // ---- net = wl . h_L + bl (four partial chains, one per lane group, as the forward kernel's last layer), then the seed ----
    {
      float part = 0.0f;
#pragma unroll
      for (int kt = 0; kt < NT; ++kt) {
        const f32x4 w = *reinterpret_cast<const f32x4 *>(wlS + 16 * kt + 4 * q);
        const f32x4 h = Hs[((size_t)(L & 1) * NT + kt) * 64 + lane];
#pragma unroll
        for (int r = 0; r < 4; ++r) part = fmaf(w[r], h[r], part);
      }
      const float pair = part + __shfl_xor(part, 16);
      seed = seed_of((pair + __shfl_xor(pair, 32)) + wlS[NP]);
    }
    }
    // ---- backward: d_L = seed * wl * lrelu'(h_L); d_{l-1} = (W_l^T d_l) * lrelu'(h_{l-1}) ----
    {
      const unsigned sgL = mk.get(L);   // this wavefront's full tiles, then the remainder tiles (== h > 0 of the activations in LDS)
#pragma unroll
    for (int i = 0; i < (NT + G - 1) / G; ++i) {
      const int rt = wave + i * G;
      if (rt < NT) {
        const f32x4 w = *reinterpret_cast<const f32x4 *>(wlS + 16 * rt + 4 * q);
        const int sl = (i < F) ? 4 * i : 4 * (F + rt - G * F);   // bit slot of row tile rt in this wavefront's word
        f32x4 d;
#pragma unroll
        for (int r = 0; r < 4; ++r) d[r] = (seed * w[r]) * (((sgL >> (sl + r)) & 1u) ? 1.0f : 0.01f);
        Ds[((L & 1) * NT + rt) * 64 + lane] = d;
        if (i == 0) own = d;
        if (rec) rec_store<NTS>(recD + ((size_t)L * NT + rt) * 64, d);
      }
    }
    }
    bool pendb = false;   // the previous product's remainder tiles are still partial sums in Ps
    unsigned sgp = 0u;    // ... to be masked with these bits
    if (L == 0) __syncthreads();
    for (int l = L; l >= 1; --l) {
      f32x4 accF[FP], accR[RP];
#pragma unroll
      for (int i = 0; i < F; ++i) accF[i] = f32x4{0, 0, 0, 0};
#pragma unroll
      for (int j = 0; j < R; ++j) accR[j] = f32x4{0, 0, 0, 0};
      auto fold_prev = [&](int lp) {   // lp: the layer whose gradient's remainder tiles wait in Ps[par ^ 1]
        __syncthreads();
        if (R > 0 && pendb) {
#pragma unroll
          for (int j = 0; j < R; ++j) {
            const f32x4 z = fold(Ps + (par ^ 1) * pstride, j);
            f32x4 d;
#pragma unroll
            for (int r = 0; r < 4; ++r) d[r] = z[r] * (((sgp >> (4 * (F + j) + r)) & 1u) ? 1.0f : 0.01f);
            Ds[((lp & 1) * NT + G * F + j) * 64 + lane] = d;
            if (rec && wave == 0) rec_store<NTS>(recD + ((size_t)lp * NT + G * F + j) * 64, d);
          }
        }
      };
      product<0>(bwd0, l - 1, l > 1 ? bwd0 : fwd0, l > 1 ? l - 2 : 0, Ds + (size_t)(l & 1) * NT * 64,
              own, [&] { fold_prev(l); }, accF, accR);
      const unsigned sg = mk.get(l - 1);  // signs of h_{l-1}: this wavefront's full tiles, then the remainder tiles
#pragma unroll
      for (int i = 0; i < F; ++i) {
        const int rt = wave + G * i;
        f32x4 d;
#pragma unroll
        for (int r = 0; r < 4; ++r) d[r] = accF[i][r] * (((sg >> (4 * i + r)) & 1u) ? 1.0f : 0.01f);
        Ds[(((l - 1) & 1) * NT + rt) * 64 + lane] = d;
        if (i == 0) own = d;
        if (rec) rec_store<NTS>(recD + ((size_t)(l - 1) * NT + rt) * 64, d);
      }
#pragma unroll
      for (int j = 0; j < R; ++j) Ps[par * pstride + (j * G + wave) * 64 + lane] = accR[j];
      pendb = R > 0; sgp = sg;
      par ^= 1;
      if (l == 1) fold_prev(0);   // behind the last product: the input-layer dot product below reads every tile
    }
    // ---- d net / d x1 = sum_k W0[k][1] d_0[k]  (x0 is the voltage: a constant of the differentiation) ----
    float part = 0.0f;
#pragma unroll
    for (int kt = 0; kt < NT; ++kt) {
      const f32x4 d = Ds[kt * 64 + lane];
      if constexpr (NT <= 13) {
        const f32x4 w = *reinterpret_cast<const f32x4 *>(w01S + 16 * kt + 4 * q);
#pragma unroll
        for (int r = 0; r < 4; ++r) part = fmaf(w[r], d[r], part);
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r) part = fmaf(W0s[16 * kt + 4 * q + r][2], d[r], part);
      }
    }
    const float pair = part + __shfl_xor(part, 16);
    const float out = pair + __shfl_xor(pair, 32);
    if (rec && wave == 0 && lane < 16) {
      float *sc = rec + IONODE_RECORD_SCALARS(L, NT);
      sc[REC_X0 + lane] = x0; sc[REC_X1 + lane] = x1; sc[REC_SEED + lane] = seed; sc[REC_PAD + lane] = 0.0f;
    }
    __syncthreads();  // the next evaluation's layer 0 rewrites Hs[0] / Ds
    return out;
  }
};

// Observation model of the fused objective (ionode_device.hpp, the forward's current / objective epilogue), the state y in the
// state dtype: i = (double)gate(y) * (V - obs_e), r = i - ref.  Returns r and dr/dy (fp64).
template <typename S, int D>
__device__ __forceinline__ double sse_residual(const GArgs &a, const S (&y)[D], double v, double ref, double (&dr)[D]) {
  const double gdv = a.obs_g * (v - a.obs_e);
#pragma unroll
  for (int d = 0; d < D; ++d) dr[d] = 0.0;
  if (a.obs_open) dr[D - 1] = gdv;
  else { dr[0] = gdv * (double)y[1]; dr[1] = gdv * (double)y[0]; }
  return obs_current<S, D>(a, y, v) - ref;
}

// The dense-output coefficients (e, d, c, b, a) of an accepted step, fitted from its checkpoint (step length, start state, k1..k7) as
// the forward fitted them: interp_fit in the state dtype, the same bits.  y_next: the next accepted step's checkpointed start state
// (this step's y1), or NULL for the trajectory's last step, whose y1 is recomputed in the forward's order.
template <typename S, int D>
__device__ __forceinline__ void sse_fit_step(double dt, const double (&y)[D], const double (&k)[7][D], const double *__restrict__ y_next, S (&cf)[5][D]) {
  const S dts_s = (S)dt;
  S ys[D], y1[D], ks[7][D];
#pragma unroll
  for (int d = 0; d < D; ++d) ys[d] = (S)y[d];
#pragma unroll
  for (int jx = 0; jx < 7; ++jx)
#pragma unroll
    for (int d = 0; d < D; ++d) ks[jx][d] = (S)k[jx][d];
  if (y_next) {
#pragma unroll
    for (int d = 0; d < D; ++d) y1[d] = (S)y_next[d];
  } else interp_y1<S, D>(dts_s, ys, ks, y1);
  interp_fit_all<S, D>(dts_s, ys, y1, ks, cf);
}

// One output sample of the step: y_k from the interpolant at x (state dtype: interp_eval), its residual against `ref` at voltage
// v, and P[c][d] += w_k dr_k/dy_d x^c in fp64, w_k = residual_weight(r_k, g, ABS) with g = dL/dsum[b]: 2 g r_k for the squares,
// g sign(r_k) for the absolute values.  ABS is a constant: the callers branch on KArgs::obj_abs around their sample loops.
template <typename S, int D, int ABS>
__device__ __forceinline__ void sse_sample_term(const GArgs &a, const S (&cf)[5][D], S xs, double v, double ref, double g, double (&P)[5][D]) {
  S out[D];
  interp_eval<S, D>(cf, xs, out);
  double dr[D];
  const double gr = residual_weight(sse_residual<S, D>(a, out, v, ref, dr), g, ABS);
  const double x = (double)xs;
  double xp = 1.0;
#pragma unroll
  for (int c = 0; c < 5; ++c) {
#pragma unroll
    for (int d = 0; d < D; ++d) P[c][d] += (gr * dr[d]) * xp;
    xp *= x;
  }
}

// The sample loop of one step, once per kind: `samples(kind)` runs it with kind() as sse_sample_term's ABS.  One wave-uniform branch
// per step and trajectory (the forward's flag cost the 6-state squares 2.8 % as a per-sample select and nothing as a hoisted branch:
// profiles/objective_kinds.md).
template <typename F> __device__ __forceinline__ void sse_step_samples(int obj_abs, F &&samples) {
  if (__builtin_expect(obj_abs != 0, 0)) samples(std::integral_constant<int, 1>{});
  else samples(std::integral_constant<int, 0>{});
}

// One-phase backward sweep; SSE: the fused sum-of-squares variant (closed-form models only).  Only the source of the output
// gradients differs: instead of reading grad_y [B][Nt][D], the sweep re-evaluates every output sample of the step from the
// step's interpolant (fitted from the checkpoint by the forward's own routines, ionode_interp.hpp, in the state dtype: the same bits as the
// forward's dense output) and forms dL/dy_k = 2 dL/dsse[b] r_k dr_k/dy_k on the sample's lane.
template <int MODEL, typename S, int NT>
__global__ void __launch_bounds__(256) ionode_dopri5_backward_kernel(const GArgs a) {
  constexpr bool SSE = false;
#include "ionode_grad_sweep_body.hpp"
}

template <int MODEL, typename S>
__global__ void __launch_bounds__(256) ionode_dopri5_backward_sse_kernel(const GArgs a) {
  constexpr bool SSE = true;
  constexpr int NT = 1;
#include "ionode_grad_sweep_body.hpp"
}

// ---------------------------------------------------------------------------------------------
// Two-phase sweep (NN-f / NN-d).  The one-phase sweep above walks a tile's accepted steps on one compute unit -- 64 of 256 at
// BASELINE configs[4]'s per-GPU batch -- and does everything inside the walk.  But (1) the stage inputs Y_i, the protocol
// voltages, the rate exponentials and the reduction of the step's output gradients into the interpolant-coefficient adjoints G_c
// depend on the step's CHECKPOINT only; and (2) a stage's vector-Jacobian product is LINEAR in its seed, which is a scalar per
// trajectory: vjp(seed) = seed * vjp(1).  So nothing of the MLP depends on the adjoint except through that scalar.
// Phase A (ionode_grad_recompute_kernel) computes, for every (tile, step) of a chunk at once -- grid = (tiles, blocks of IB
// iterations): the whole chip -- the UNIT-SEED product of all six stages: records with unit-seed D tiles (ionode_grad_reduce scales
// them by the seeds while staging them), and per trajectory and step a 64-double packet (GRAD_PACKET: dts, flags, G_c, and per
// stage V, Y_i, the exponentials, c = d net / d x1 at unit seed).  Phase B (ionode_grad_walk_kernel) is what is sequential: the
// adjoint algebra, one wavefront per tile, one 8 KiB packet burst per step, the stage's seed written into its record.
// Against the one-phase sweep the seed multiplies at the END of the fp32 product instead of at its start: equal to fp32 rounding
// (1e-7 relative per evaluation; tests: 1e-5 on the gradients, the checker's tolerance is 1e-4).
// ---------------------------------------------------------------------------------------------
constexpr int GRAD_RECOMPUTE_IB = 4;   // iterations per workgroup

#ifndef IONODE_RECOMPUTE_WG_PER_CU
#define IONODE_RECOMPUTE_WG_PER_CU 2   // N <= 200: a 256-register build, two workgroups per compute unit (round 5; 1: the 332-register build, one per unit)
#endif
template <int MODEL, typename S, int NT>
__global__ void __launch_bounds__(256, (NT <= 13 ? IONODE_RECOMPUTE_WG_PER_CU : 1)) ionode_grad_recompute_kernel(const GArgs a) {
  constexpr int D = ModelTraits<MODEL>::D, NPAR = ModelTraits<MODEL>::NPAR;
  static_assert(ModelTraits<MODEL>::MLP && D == 2, "NN-f / NN-d");
  constexpr bool NND = MODEL == IONODE_MODEL_NND;
  using R = Real<S>;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int j = lane & 15;
  const int traj_raw = blockIdx.x * 16 + j;
  const bool valid = traj_raw < a.k.B;
  const int traj = valid ? traj_raw : a.k.B - 1;
  GradMlp<NT> mlp;
  mlp.init(a, smem, wave, lane);
  double *__restrict__ Gs = mlp.gs();
  const int pidx = a.k.prot_of_traj ? a.k.prot_of_traj[traj] : (traj % a.k.P);
  const double *__restrict__ pv = a.k.prot_v + (size_t)pidx * a.k.Np;
  const int nst = valid ? a.nacc[traj] : 0;
  using CK = CkptRecord<D>;
  constexpr int RECW = CK::WIDTH;
  const double *__restrict__ ck = a.ckpt + (size_t)traj * a.ckpt_cap * RECW;
  const int Nt = a.k.Nt;
  const bool pk_writer = wave == 0 && lane < 16;
  const int it_lo = a.it_begin + (int)blockIdx.y * GRAD_RECOMPUTE_IB;
  const int it_hi = (it_lo + GRAD_RECOMPUTE_IB < a.it_end) ? it_lo + GRAD_RECOMPUTE_IB : a.it_end;
  // Memory round trips of an iteration (round 5).  An iteration is ~140 us of MFMA work behind a chain of dependent loads from HBM-resident
  // arrays: the step's checkpoint -> its output gradients (four trajectories per wavefront, one after the other) -> six protocol lookups,
  // one in front of every stage's product -- about a dozen exposed round trips.  Now: the NEXT iteration's checkpoint is fetched while this
  // one's products run, the four trajectories' first 64 samples are loaded together, and the stage voltages are looked up ahead of the
  // stages (as the forward kernel does): three round trips.  Same values, same summation order, same bits.
  double crec[RECW];   // the coming iteration's checkpoint record (a clamped, always valid row: what is not wanted is masked below)
  auto fetch_ckpt = [&](int it) {
    const int s = nst - 1 - it;
    const double *rec = ck + (size_t)(s >= 0 ? s : 0) * RECW;
#pragma unroll
    for (int i = 0; i < RECW; ++i) crec[i] = rec[i];
  };
  constexpr bool CKPT_AHEAD = NT > 13 || IONODE_RECOMPUTE_WG_PER_CU < 2;   // (two workgroups per unit: the other one covers the round trip, and the 40 registers are not there)
  if (CKPT_AHEAD && it_lo < it_hi) fetch_ckpt(it_lo);
  for (int it = it_lo; it < it_hi; ++it) {
    if (!CKPT_AHEAD) fetch_ckpt(it);
    // ---- checkpoint of my step: as in ionode_dopri5_backward_kernel ----
    const int s = nst - 1 - it;
    const bool step = s >= 0;
    const bool initev = (s == -1) && nst > 0;
    double t0 = 0.0, dt = 1.0, y[D], k[7][D];
    int oi = 0, nout = 0;
    {
      const bool ld = step || initev;
      if (ld) { t0 = crec[CK::T0]; dt = crec[CK::DT]; }
      if (step) { oi = (int)crec[CK::OI]; nout = (int)crec[CK::NOUT]; }
#pragma unroll
      for (int d = 0; d < D; ++d) y[d] = ld ? crec[CK::Y + d] : 0.0;
#pragma unroll
      for (int jx = 0; jx < 7; ++jx)
#pragma unroll
        for (int d = 0; d < D; ++d) k[jx][d] = step ? crec[CK::K + jx * D + d] : 0.0;
    }
    if (CKPT_AHEAD && it + 1 < it_hi) fetch_ckpt(it + 1);
    const double t1 = t0 + dt;
    const S t0s = (S)t0, dts_s = (S)dt, t1s = (S)t1;
    const double dts = (double)dts_s;
    const size_t tstep = (size_t)blockIdx.x * (a.it_end - a.it_begin) + (it - a.it_begin);
    double *__restrict__ pk = a.packets + (tstep * 16 + j) * GRAD_PACKET;

    // ---- adjoints of the interpolant coefficients: G_c = sum_k gy[k] * x_k^c over the step's output samples ----
    // (a copy of ionode_grad_sweep_body.hpp's reduction: a shared routine compiled to other code -- DESIGN_HISTORY.md, "The backward sweep's step algebra"; correct both)
    // grad_y == NULL (wave-uniform): the fused objective -- ionode_grad_sse_gc_kernel (ionode_grad_gc.hpp) writes the packets' G_c, nothing is reduced here
    if (a.grad_y != nullptr) {
    // (the first 64 samples of the wavefront's four trajectories: all loads in flight before the first is used)
    double tk0[4] = {0.0, 0.0, 0.0, 0.0};
    S gy0[4][D] = {};
#pragma unroll
    for (int u = 0; u < (CKPT_AHEAD ? 4 : 0); ++u) {   // (two workgroups per unit: not ahead -- the other workgroup covers the round trips)
      const int jj = wave + 4 * u;
      const int n = __builtin_amdgcn_readlane(nout, jj);
      const int o = __builtin_amdgcn_readlane(oi, jj);
      const int tr = __builtin_amdgcn_readlane(traj, jj);
      int idx = o + (lane < n ? lane : 0);
      idx = idx < Nt ? (idx < 0 ? 0 : idx) : Nt - 1;   // (n == 0: any valid sample; it is not used)
      tk0[u] = a.k.t_eval[idx];
      const S *__restrict__ gyb = reinterpret_cast<const S *>(a.grad_y) + (size_t)tr * Nt * D;
#pragma unroll
      for (int d = 0; d < D; ++d) gy0[u][d] = gyb[(size_t)idx * D + d];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int jj = wave + 4 * u;
      const int n = __builtin_amdgcn_readlane(nout, jj);
      double P[5][D];
#pragma unroll
      for (int c = 0; c < 5; ++c)
#pragma unroll
        for (int d = 0; d < D; ++d) P[c][d] = 0.0;
      if (n > 0) {
        const int o = __builtin_amdgcn_readlane(oi, jj);
        const int tr = __builtin_amdgcn_readlane(traj, jj);
        const double t0b = bcast_f64(t0, jj), t1b = bcast_f64(t1, jj);
        const S *__restrict__ gyb = reinterpret_cast<const S *>(a.grad_y) + (size_t)tr * Nt * D;
        for (int c0 = 0; c0 < n; c0 += 64) {
          if (c0 + lane < n) {
            const int idx = o + c0 + lane;
            const double tk = (CKPT_AHEAD && c0 == 0) ? tk0[u] : a.k.t_eval[idx];
            const double x = (double)(S)((tk - t0b) / (t1b - t0b));
            double xp = 1.0;
#pragma unroll
            for (int c = 0; c < 5; ++c) {
#pragma unroll
              for (int d = 0; d < D; ++d) P[c][d] += (double)((CKPT_AHEAD && c0 == 0) ? gy0[u][d] : gyb[(size_t)idx * D + d]) * xp;
              xp *= x;
            }
          }
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1)
#pragma unroll
          for (int c = 0; c < 5; ++c)
#pragma unroll
            for (int d = 0; d < D; ++d) P[c][d] += __shfl_xor(P[c][d], m);
      }
      if (lane == 0) {
#pragma unroll
        for (int c = 0; c < 5; ++c)
#pragma unroll
          for (int d = 0; d < D; ++d) Gs[jj * (5 * D) + c * D + d] = P[c][d];
      }
    }
    }
    __syncthreads();
    if (pk_writer) {
      pk[pkt::DTS] = dts; pk[pkt::STEP] = step ? 1.0 : 0.0; pk[pkt::INITEV] = initev ? 1.0 : 0.0; pk[3] = 0.0;
      if (a.grad_y != nullptr) {
#pragma unroll
        for (int c = 0; c < 5; ++c)
#pragma unroll
          for (int d = 0; d < D; ++d) pk[pkt::GC + c * D + d] = Gs[j * (5 * D) + c * D + d];
      }
    }
    // ---- the six stages' scalar work, AHEAD of their products (round 5): stage voltages (pure functions of (t0, dt): the five distinct
    // lookups in flight together -- stage i = 5 shares i = 4's time), stage inputs Y_i, rate exponentials, the packet; what a product needs
    // -- (x0, x1) per trajectory -- waits in LDS (the G_c scratch, read above by the very lanes that write here).  The product loop then
    // carries none of the step's fp64 state (k[7][D], y, p, the checkpoint in flight): registers for the MFMA stream instead.
    float *xs = reinterpret_cast<float *>(Gs);   // [6][16][2]
    {
      double vst[5];
      double p[NPAR];   // (loaded here, per iteration: 16 registers that need not live through the products)
#pragma unroll
      for (int i = 0; i < NPAR; ++i) p[i] = a.k.params[(size_t)traj * a.k.n_params + i];
      const double tq_init = (double)(S)a.k.t_eval[0];
#pragma unroll
      for (int i = 0; i < 5; ++i) {
        const S ti = (i >= 4) ? R::prev_(t1s) : t0s + (S)kAlpha[i] * dts_s;
        protocol_v(a.k, pv, step ? (double)ti : tq_init, vst[i]);
      }
#pragma unroll
      for (int e = 0; e < 6; ++e) {
        const int i = 5 - e;
        double Yi[D];
        if (step) {
#pragma unroll
          for (int d = 0; d < D; ++d) {
            double sacc = 0.0;
#pragma unroll
            for (int jx = 0; jx <= i; ++jx) sacc += k[jx][d] * (kBeta[i][jx] * dts);
            Yi[d] = y[d] + sacc;
          }
        } else {
#pragma unroll
          for (int d = 0; d < D; ++d) Yi[d] = y[d];
        }
        const double v = vst[i < 4 ? i : 4];
        const float x0 = (float)(v / 100.0), x1 = (float)Yi[0];
        const double e3 = det_exp(p[5] * v), e4 = det_exp(-p[7] * v);
        double e1 = 0.0, e2 = 0.0;
        if constexpr (NND) { e1 = det_exp(p[1] * v); e2 = det_exp(-p[3] * v); }
        if (pk_writer) {
          double *q8 = pk + pkt::STAGE + pkt::STAGE_W * e;
          q8[pkt::V] = v; q8[pkt::Y0] = Yi[0]; q8[pkt::Y1] = Yi[1]; q8[pkt::E3] = e3; q8[pkt::E4] = e4; q8[pkt::E1] = e1; q8[pkt::E2] = e2;
          xs[(e * 16 + j) * 2] = x0; xs[(e * 16 + j) * 2 + 1] = x1;
        }
      }
    }
    __syncthreads();
#pragma unroll 1
    for (int e = 0; e < 6; ++e) {
      const f32x2 xx = *reinterpret_cast<const f32x2 *>(xs + (e * 16 + j) * 2);
      // the WHOLE vector-Jacobian product with seed 1 (it is linear in the seed, a scalar per trajectory): record with unit-seed
      // D tiles, and c = d net / d x1 for the walk
      const float c1 = mlp.template vjp<false>(xx[0], xx[1], 1.0f, a.records ? a.records + (tstep * 6 + e) * a.record_floats : nullptr);
      if (pk_writer) pk[pkt::STAGE + pkt::STAGE_W * e + pkt::C] = (double)c1;
    }
  }
}

// Phase B: the sequential walk.  NO MLP work is left in it: the vector-Jacobian product of a stage is seed * (unit-seed product),
// the seed a scalar per trajectory, so the walk multiplies the stage's c = d net / d x1 (packet) by its seed, writes the seed into
// the record's scalar block for ionode_grad_reduce (which scales the unit-seed D tiles while staging them), and does the adjoint
// algebra.  One wavefront per 16-trajectory tile (lanes replicate it 4x); LDS: the step's 16 packets.
template <int MODEL, typename S>
__global__ void __launch_bounds__(64) ionode_grad_walk_kernel(const GArgs a) {
  constexpr int D = ModelTraits<MODEL>::D, NPAR = ModelTraits<MODEL>::NPAR;
  static_assert(ModelTraits<MODEL>::MLP && D == 2, "NN-f / NN-d");
  constexpr bool NND = MODEL == IONODE_MODEL_NND;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int lane = threadIdx.x & 63;
  const int j = lane & 15;
  const int traj_raw = blockIdx.x * 16 + j;
  const bool valid = traj_raw < a.k.B;
  const int traj = valid ? traj_raw : a.k.B - 1;
  const bool writer = valid && lane < 16;
  double *__restrict__ pkl = reinterpret_cast<double *>(smem);   // [16][GRAD_PACKET]

  double p[NPAR];
#pragma unroll
  for (int i = 0; i < NPAR; ++i) p[i] = a.k.params[(size_t)traj * a.k.n_params + i];
  const S *__restrict__ gy = reinterpret_cast<const S *>(a.grad_y) + (size_t)traj * a.k.Nt * D;
  constexpr int STATE = 2 * D + NPAR;
  double lam[D], mu[D], gp[NPAR];
  {
    const double *st = a.state + (size_t)traj * STATE;
#pragma unroll
    for (int d = 0; d < D; ++d) { lam[d] = a.it_begin > 0 ? st[d] : 0.0; mu[d] = a.it_begin > 0 ? st[D + d] : 0.0; }
#pragma unroll
    for (int i = 0; i < NPAR; ++i) gp[i] = a.it_begin > 0 ? st[2 * D + i] : 0.0;
  }
  const size_t sc_off = IONODE_RECORD_SCALARS(a.k.L, a.k.NT) + REC_SEED;   // the seeds inside a record's scalar block
  const double2 *__restrict__ psrc = reinterpret_cast<const double2 *>(a.packets + (size_t)blockIdx.x * (a.it_end - a.it_begin) * 16 * GRAD_PACKET) + 8 * lane;
  for (int it = a.it_begin; it < a.it_end; ++it) {
    const size_t tstep = (size_t)blockIdx.x * (a.it_end - a.it_begin) + (it - a.it_begin);
    __syncthreads();   // (one wavefront: orders the LDS reads of the previous step before these writes)
    {
      const double2 *__restrict__ src = psrc + (size_t)(it - a.it_begin) * (16 * GRAD_PACKET / 2);
      double2 *dst = reinterpret_cast<double2 *>(pkl) + 8 * lane;
#pragma unroll
      for (int u = 0; u < 8; ++u) dst[u] = src[u];
    }
    __syncthreads();
    const double *__restrict__ pk = pkl + j * GRAD_PACKET;
    const double dts = pk[pkt::DTS];
    const bool step = pk[pkt::STEP] != 0.0, initev = pk[pkt::INITEV] != 0.0;
    double Gc[5][D];
#pragma unroll
    for (int c = 0; c < 5; ++c)
#pragma unroll
      for (int d = 0; d < D; ++d) Gc[c][d] = pk[pkt::GC + c * D + d];

    // ---- interpolant adjoint -> (Y0, Y1, k1..k7); FSAL carry ----
    // (a copy of ionode_grad_sweep_body.hpp's: shared, the kernels compiled to other code -- DESIGN_HISTORY.md, "The backward sweep's step algebra"; correct both)
    double aY0[D], aY1[D], ak[7][D];
#pragma unroll
    for (int d = 0; d < D; ++d) {
      const double g0 = Gc[0][d], g1 = Gc[1][d], g2 = Gc[2][d], g3 = Gc[3][d], g4 = Gc[4][d];
      const double aYM = 16.0 * g4 - 32.0 * g3 + 16.0 * g2;
      aY0[d] = g0 - 8.0 * g4 + 18.0 * g3 - 11.0 * g2 + aYM;
      aY1[d] = -8.0 * g4 + 14.0 * g3 - 5.0 * g2 + lam[d];
#pragma unroll
      for (int jx = 0; jx < 7; ++jx) ak[jx][d] = (kCmid[jx] * dts) * aYM;
      ak[0][d] += dts * (-2.0 * g4 + 5.0 * g3 - 4.0 * g2 + g1);
      ak[6][d] += dts * (2.0 * g4 - 3.0 * g3 + g2) + mu[d];
    }
    float *__restrict__ rec_it = a.records ? a.records + tstep * 6 * a.record_floats : nullptr;
    // (six compile-time instances: no collective in here any more, and ak[][] must stay register-indexed)
    auto stage = [&](auto ec) {
      constexpr int e = decltype(ec)::value;
      constexpr int i = 5 - e;
      const double *__restrict__ q8 = pk + pkt::STAGE + pkt::STAGE_W * e;
      const double v = q8[pkt::V], av = q8[pkt::Y0], rv = q8[pkt::Y1], e3 = q8[pkt::E3], e4 = q8[pkt::E4];
      double seed[D];
#pragma unroll
      for (int d = 0; d < D; ++d) seed[d] = step ? ak[i + 1][d] : ((initev && e == 0) ? mu[d] : 0.0);
      const float seedf = (float)(seed[0] / 1000.0);
      if (rec_it && lane < 16) rec_it[(size_t)e * a.record_floats + sc_off + lane] = seedf;
      const float dx1 = seedf * (float)q8[pkt::C];
      // closed-form terms of the RHS and their parameter gradients (copies of ionode_grad_sweep_body.hpp's stage terms and propagation, for the same reason; correct both)
      double w[D];
      const double k3 = p[4] * e3, k4 = p[6] * e4;
      w[0] = (double)dx1;
      w[1] = -seed[1] * (k3 + k4);
      gp[4] += seed[1] * (-e3 * rv);
      gp[5] += seed[1] * (-k3 * v * rv);
      gp[6] += seed[1] * (e4 * (1.0 - rv));
      gp[7] += seed[1] * (-k4 * v * (1.0 - rv));
      if constexpr (NND) {
        const double e1 = q8[pkt::E1], e2 = q8[pkt::E2];
        const double k1 = p[0] * e1, k2 = p[2] * e2;
        w[0] += -seed[0] * (k1 + k2);
        gp[0] += seed[0] * (e1 * (1.0 - av));
        gp[1] += seed[0] * (k1 * v * (1.0 - av));
        gp[2] += seed[0] * (-e2 * av);
        gp[3] += seed[0] * (k2 * v * av);
      }
      if (step) {
#pragma unroll
        for (int d = 0; d < D; ++d) {
          const double wd = (i == 5) ? w[d] + aY1[d] : w[d];
          aY0[d] += wd;
#pragma unroll
          for (int jx = 0; jx <= i; ++jx) ak[jx][d] += (kBeta[i][jx] * dts) * wd;
        }
      } else if (initev && e == 0) {
#pragma unroll
        for (int d = 0; d < D; ++d) lam[d] += w[d];
      }
    };
    stage(std::integral_constant<int, 0>{}); stage(std::integral_constant<int, 1>{}); stage(std::integral_constant<int, 2>{});
    stage(std::integral_constant<int, 3>{}); stage(std::integral_constant<int, 4>{}); stage(std::integral_constant<int, 5>{});
    if (step) {
#pragma unroll
      for (int d = 0; d < D; ++d) { lam[d] = aY0[d]; mu[d] = ak[0][d]; }
    }
  }
  if (writer) {
    double *st = a.state + (size_t)traj * STATE;
#pragma unroll
    for (int d = 0; d < D; ++d) { st[d] = lam[d]; st[D + d] = mu[d]; }
#pragma unroll
    for (int i = 0; i < NPAR; ++i) st[2 * D + i] = gp[i];
    if (a.it_end >= a.n_iter) {
#pragma unroll
      for (int i = 0; i < NPAR; ++i) a.grad_params[(size_t)traj * NPAR + i] = gp[i];
#pragma unroll
      for (int d = 0; d < D; ++d) a.grad_y0[(size_t)traj * D + d] = lam[d] + (a.grad_y != nullptr ? (double)gy[d] : a.sse_y0[(size_t)traj * D + d]);  // solution[0] = y0 (fused objective: its sample-0 term)
    }
  }
}

}  // namespace ionode
