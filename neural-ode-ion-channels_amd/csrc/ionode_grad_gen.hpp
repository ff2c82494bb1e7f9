// ionode_grad_gen.hpp -- the MLP regression step at a RUN-TIME width: GradMlpGen (the vector-Jacobian product of ionode_grad.hpp's
// GradMlp<NT> with NT = ceil(N / 16) in [1, 32] read from the arguments), the regress kernel over it and a run-time-width reduce kernel.
// For the widths without a tuned instantiation (for_width: N pads to 16, 112, 208 or 512); table-s1.py:145-153 builds
// Linear(2, N) ... Linear(N, 1) for any (n_layers, n_nodes), and MlpGen (ionode_mlp_gen.hpp) already integrates such a net.
//
// No performance target, as in MlpGen: weight fragments are read from L2 as they are needed (the next one in flight), no register ring,
// one accumulator tile at a time, a workgroup barrier per product.  SAME grad image, SAME record layout and SAME canonical accumulation
// order as GradMlp: NT = 4 F + R; wavefront w owns the full row tiles w, w + 4, ... < 4 F -- one chain each over
// the k-tiles in the rotated order kt = (s + w) mod NT, r = 0..3 inside a k-tile, seeded with the bias in the forward and with 0 in
// the transposed products -- and partial chain w (k-tiles kt % 4 == w, ascending; chain 0 carries the bias) of each of the R remainder
// row tiles, folded (p0 + p1) + (p2 + p3); Linear(N, 1) and the closing d net / d x1 as four chains by lane group q.  A record written
// here equals GradMlp's bit for bit at the widths both serve (tests/test_gpu_regress_widths.py).
// Included by inst_grad_gen.hip only (ionode_grad_gen_plan.hpp is the host's view).
#pragma once

#include "ionode_grad_gen_plan.hpp"

namespace ionode {

struct GradMlpGen {
  static constexpr int G = 4;
  f32x4 *Hs;          // LDS [2][NT*64]     activations after LeakyReLU, accumulator layout, layer l in buffer l & 1
  f32x4 *Ds;          // LDS [2][NT*64]     pre-activation gradients, layer l in buffer l & 1
  f32x4 *Ps;          // LDS [2][R][G][64]  partial sums of the remainder row tiles, ping-pong over products
  const f32x4 *W0s;   // LDS [NP] {b0, w00, w01, 0}
  const float *biasS; // LDS [L][NP]
  const float *wlS;   // LDS [NP] + bl
  __amdgpu_buffer_rsrc_t rsrc;
  unsigned fwd0, bwd0;  // byte offsets of the fragment sections
  int L, NT, NP, F, F4, R, wave, lane;
  int roff;           // this lane's float offset inside a record tile (rec_store)

  __device__ __forceinline__ void init(const GArgs &a, unsigned char *smem, int wave_, int lane_) {
    L = a.k.L; NT = a.k.NT; NP = 16 * NT; wave = wave_; lane = lane_;
    F = NT / G; F4 = G * F; R = NT - F4;
    roff = 64 * (lane & 3) + 16 * (lane >> 4) + ((lane & 15) >> 2);
    Hs = reinterpret_cast<f32x4 *>(smem);
    Ds = Hs + (size_t)2 * NT * 64;
    Ps = Ds + (size_t)2 * NT * 64;
    f32x4 *w0 = Ps + 2 * R * G * 64;
    float *bs = reinterpret_cast<float *>(w0 + NP);
    float *ws = bs + (size_t)L * NP;
    const int tid = wave * 64 + lane;
    const f32x4 *src = reinterpret_cast<const f32x4 *>(a.img);
    for (int i = tid; i < NP; i += 64 * G) w0[i] = src[i];
    for (int i = tid; i < L * NP; i += 64 * G) bs[i] = a.img[grad_img_bias(NT) + i];
    for (int i = tid; i < NP + 4; i += 64 * G) ws[i] = a.img[grad_img_wl(L, NT) + i];
    W0s = w0; biasS = bs; wlS = ws;
    rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(a.img), 0, (int)(grad_img_floats(L, NT) * 4), 0x00020000);
    fwd0 = (unsigned)(grad_img_fwd(L, NT) * 4);
    bwd0 = (unsigned)(grad_img_bwd(L, NT) * 4);
    __syncthreads();
  }
  __device__ __forceinline__ double *gs() const {  // LDS [16][10] fp64 scratch behind the small vectors (8-byte aligned)
    return reinterpret_cast<double *>(const_cast<float *>(wlS) + NP + 4);
  }

  // LeakyReLU'(h) of a layer as bits: 4 per owned full tile (F <= 8), then 4 per remainder tile (R <= 3) -- up to 44, so one 64-bit
  // word per layer 0..15.  Scalar members and pure mask arithmetic, as GradMlp::Signs (an indexed array, or selects over the members,
  // end in scratch).
  static __device__ __forceinline__ unsigned long long bits_of(const f32x4 &h) {
    return (h[0] > 0.0f ? 1ull : 0ull) | (h[1] > 0.0f ? 2ull : 0ull) | (h[2] > 0.0f ? 4ull : 0ull) | (h[3] > 0.0f ? 8ull : 0ull);
  }
  static __device__ __forceinline__ float slope(unsigned long long sg, int bit) { return ((sg >> bit) & 1ull) ? 1.0f : 0.01f; }
  struct Signs {
    unsigned long long w0 = 0, w1 = 0, w2 = 0, w3 = 0, w4 = 0, w5 = 0, w6 = 0, w7 = 0, w8 = 0, w9 = 0, w10 = 0, w11 = 0, w12 = 0,
                       w13 = 0, w14 = 0, w15 = 0;
    static __device__ __forceinline__ unsigned long long on(int k, int i) { return (k == i) ? ~0ull : 0ull; }
    __device__ __forceinline__ void put(int l, unsigned long long v) {
#define IONODE_SIGN_PUT(i) w##i = (w##i & ~on(l, i)) | (v & on(l, i));
      IONODE_SIGN_PUT(0) IONODE_SIGN_PUT(1) IONODE_SIGN_PUT(2) IONODE_SIGN_PUT(3) IONODE_SIGN_PUT(4) IONODE_SIGN_PUT(5)
      IONODE_SIGN_PUT(6) IONODE_SIGN_PUT(7) IONODE_SIGN_PUT(8) IONODE_SIGN_PUT(9) IONODE_SIGN_PUT(10) IONODE_SIGN_PUT(11)
      IONODE_SIGN_PUT(12) IONODE_SIGN_PUT(13) IONODE_SIGN_PUT(14) IONODE_SIGN_PUT(15)
#undef IONODE_SIGN_PUT
    }
    __device__ __forceinline__ unsigned long long get(int l) const {
      return (w0 & on(l, 0)) | (w1 & on(l, 1)) | (w2 & on(l, 2)) | (w3 & on(l, 3)) | (w4 & on(l, 4)) | (w5 & on(l, 5)) |
             (w6 & on(l, 6)) | (w7 & on(l, 7)) | (w8 & on(l, 8)) | (w9 & on(l, 9)) | (w10 & on(l, 10)) | (w11 & on(l, 11)) |
             (w12 & on(l, 12)) | (w13 & on(l, 13)) | (w14 & on(l, 14)) | (w15 & on(l, 15));
    }
  };

  __device__ __forceinline__ f32x4 frag(unsigned sec, int l, int rt, int kt) const {   // (bounds-checked by the buffer descriptor)
    using u32x4 = __attribute__((ext_vector_type(4))) unsigned;
    const unsigned off = sec + (unsigned)(((l * NT + rt) * NT + kt) * 1024);
    const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rsrc, (unsigned)lane * 16u, off, 0);
    return __builtin_bit_cast(f32x4, v);
  }
  // GradMlp::rec_store: the operand layout of the reduce kernels' MFMAs
  template <bool NTS>
  __device__ __forceinline__ void rec_store(f32x4 *tile, const f32x4 &v) const {
    float *p = reinterpret_cast<float *>(tile) + roff;
    if constexpr (NTS) {
      __builtin_nontemporal_store(v[0], p); __builtin_nontemporal_store(v[1], p + 4);
      __builtin_nontemporal_store(v[2], p + 8); __builtin_nontemporal_store(v[3], p + 12);
    } else {
      p[0] = v[0]; p[4] = v[1]; p[8] = v[2]; p[12] = v[3];
    }
  }

  // acc += A(sec, l)[row tile rt][:] . B[:]: ONE chain over all k-tiles in the rotated order (full row tiles; wave < 4 <= NT there)
  __device__ __forceinline__ void chain_full(unsigned sec, int l, int rt, const f32x4 *__restrict__ B, f32x4 &acc) const {
    int kt = wave;
    f32x4 a_n = frag(sec, l, rt, kt), b_n = B[kt * 64 + lane];
    for (int s = 0; s < NT; ++s) {
      const f32x4 av = a_n, bv = b_n;
      kt = (kt + 1 == NT) ? 0 : kt + 1;
      if (s + 1 < NT) { a_n = frag(sec, l, rt, kt); b_n = B[kt * 64 + lane]; }
#pragma unroll
      for (int r = 0; r < 4; ++r) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[r], bv[r], acc, 0, 0, 0);
    }
  }
  // ... and partial chain `wave` of a remainder row tile: the k-tiles kt % 4 == wave, ascending
  __device__ __forceinline__ void chain_part(unsigned sec, int l, int rt, const f32x4 *__restrict__ B, f32x4 &acc) const {
    if (wave >= NT) return;
    int kt = wave;
    f32x4 a_n = frag(sec, l, rt, kt), b_n = B[kt * 64 + lane];
    while (kt < NT) {
      const f32x4 av = a_n, bv = b_n;
      kt += G;
      if (kt < NT) { a_n = frag(sec, l, rt, kt); b_n = B[kt * 64 + lane]; }
#pragma unroll
      for (int r = 0; r < 4; ++r) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[r], bv[r], acc, 0, 0, 0);
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

  // GradMlp's interface: one vector-Jacobian product of the net for the 16 trajectories of the tile, all four wavefronts together
  template <bool NTS = true>
  __device__ __forceinline__ float vjp(float x0, float x1, float seed, float *__restrict__ rec) {
    auto fn = [seed](float) -> float { return seed; };
    return vjp_from_output<decltype(fn), NTS>(x0, x1, rec, fn);
  }
  template <typename SeedFn, bool NTS = true>
  __device__ __forceinline__ float vjp_from_output(float x0, float x1, float *__restrict__ rec, SeedFn seed_of) {
    Signs mk;
    const int q = lane >> 4;
    f32x4 *__restrict__ recH = reinterpret_cast<f32x4 *>(rec);
    f32x4 *__restrict__ recD = recH + (size_t)(L + 1) * NT * 64;
    const int pstride = R * G * 64;
    int par = 0;  // partial-sum buffer of the running product
    // ---- forward recompute: layer 0 by row tile; remainder tiles evaluated by EVERY wavefront (all of them need the signs), stored by wavefront j ----
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
      unsigned long long bits = 0ull;
      for (int i = 0; i < F; ++i) {
        const int rt = wave + G * i;
        const f32x4 h = layer0(rt);
        bits |= bits_of(h) << (4 * i);
        Hs[rt * 64 + lane] = h;
        if (rec) rec_store<NTS>(recH + rt * 64, h);
      }
      for (int j = 0; j < R; ++j) {
        const int rt = F4 + j;
        const f32x4 h = layer0(rt);
        bits |= bits_of(h) << (4 * (F + j));
        if (wave == j) {
          Hs[rt * 64 + lane] = h;
          if (rec) rec_store<NTS>(recH + rt * 64, h);
        }
      }
      mk.put(0, bits);
    }
    __syncthreads();
    for (int l = 1; l <= L; ++l) {
      const f32x4 *__restrict__ Hin = Hs + (size_t)((l - 1) & 1) * NT * 64;
      f32x4 *__restrict__ Hout = Hs + (size_t)(l & 1) * NT * 64;
      f32x4 *__restrict__ Pl = Ps + par * pstride;
      const float *__restrict__ bl_ = biasS + (l - 1) * NP + 4 * q;
      unsigned long long bits = 0ull;
      for (int i = 0; i < F; ++i) {
        const int rt = wave + G * i;
        f32x4 acc = *reinterpret_cast<const f32x4 *>(bl_ + 16 * rt);
        chain_full(fwd0, l - 1, rt, Hin, acc);
        f32x4 h;
#pragma unroll
        for (int r = 0; r < 4; ++r) h[r] = lrelu(acc[r]);
        bits |= bits_of(h) << (4 * i);
        Hout[rt * 64 + lane] = h;
        if (rec) rec_store<NTS>(recH + ((size_t)l * NT + rt) * 64, h);
      }
      for (int j = 0; j < R; ++j) {
        const int rt = F4 + j;
        f32x4 acc = f32x4{0, 0, 0, 0};
        if (wave == 0) acc = *reinterpret_cast<const f32x4 *>(bl_ + 16 * rt);   // partial sum 0 carries the bias
        chain_part(fwd0, l - 1, rt, Hin, acc);
        Pl[(j * G + wave) * 64 + lane] = acc;
      }
      __syncthreads();
      // every wavefront folds the remainder tiles itself and writes the (identical) activations; each reads them back only after its own
      // write, so no second barrier.  Wavefront 0 streams the record.
      for (int j = 0; j < R; ++j) {
        const f32x4 z = fold(Pl, j);
        f32x4 h;
#pragma unroll
        for (int r = 0; r < 4; ++r) h[r] = lrelu(z[r]);
        bits |= bits_of(h) << (4 * (F + j));
        Hout[(F4 + j) * 64 + lane] = h;
        if (rec && wave == 0) rec_store<NTS>(recH + ((size_t)l * NT + F4 + j) * 64, h);
      }
      mk.put(l, bits);
      par ^= 1;
    }
    // ---- net = wl . h_L + bl (four partial chains, one per lane group), then the seed ----
    float seed;
    {
      const f32x4 *__restrict__ HL = Hs + (size_t)(L & 1) * NT * 64;
      float part = 0.0f;
      for (int kt = 0; kt < NT; ++kt) {
        const f32x4 w = *reinterpret_cast<const f32x4 *>(wlS + 16 * kt + 4 * q);
        const f32x4 h = HL[kt * 64 + lane];
#pragma unroll
        for (int r = 0; r < 4; ++r) part = fmaf(w[r], h[r], part);
      }
      const float pair = part + __shfl_xor(part, 16);
      seed = seed_of((pair + __shfl_xor(pair, 32)) + wlS[NP]);
    }
    // ---- backward: d_L = seed * wl * lrelu'(h_L); d_{l-1} = (W_l^T d_l) * lrelu'(h_{l-1}) ----
    {
      const unsigned long long sgL = mk.get(L);
      for (int rt = wave, i = 0; rt < NT; rt += G, ++i) {
        const f32x4 w = *reinterpret_cast<const f32x4 *>(wlS + 16 * rt + 4 * q);
        const int sl = (rt < F4) ? 4 * i : 4 * (F + rt - F4);   // bit slot of row tile rt in this wavefront's word
        f32x4 d;
#pragma unroll
        for (int r = 0; r < 4; ++r) d[r] = (seed * w[r]) * slope(sgL, sl + r);
        Ds[((size_t)(L & 1) * NT + rt) * 64 + lane] = d;
        if (rec) rec_store<NTS>(recD + ((size_t)L * NT + rt) * 64, d);
      }
    }
    __syncthreads();
    for (int l = L; l >= 1; --l) {
      const f32x4 *__restrict__ Din = Ds + (size_t)(l & 1) * NT * 64;
      f32x4 *__restrict__ Dout = Ds + (size_t)((l - 1) & 1) * NT * 64;
      f32x4 *__restrict__ Pl = Ps + par * pstride;
      const unsigned long long sg = mk.get(l - 1);  // signs of h_{l-1}: this wavefront's full tiles, then the remainder tiles
      for (int i = 0; i < F; ++i) {
        const int rt = wave + G * i;
        f32x4 acc = f32x4{0, 0, 0, 0};
        chain_full(bwd0, l - 1, rt, Din, acc);
        f32x4 d;
#pragma unroll
        for (int r = 0; r < 4; ++r) d[r] = acc[r] * slope(sg, 4 * i + r);
        Dout[rt * 64 + lane] = d;
        if (rec) rec_store<NTS>(recD + ((size_t)(l - 1) * NT + rt) * 64, d);
      }
      for (int j = 0; j < R; ++j) {
        f32x4 acc = f32x4{0, 0, 0, 0};
        chain_part(bwd0, l - 1, F4 + j, Din, acc);
        Pl[(j * G + wave) * 64 + lane] = acc;
      }
      __syncthreads();
      for (int j = 0; j < R; ++j) {
        const f32x4 z = fold(Pl, j);
        f32x4 d;
#pragma unroll
        for (int r = 0; r < 4; ++r) d[r] = z[r] * slope(sg, 4 * (F + j) + r);
        Dout[(F4 + j) * 64 + lane] = d;
        if (rec && wave == 0) rec_store<NTS>(recD + ((size_t)(l - 1) * NT + F4 + j) * 64, d);
      }
      par ^= 1;
    }
    // ---- d net / d x1 = sum_k W0[k][1] d_0[k]  (x0 is the voltage: a constant of the differentiation) ----
    float part = 0.0f;
    for (int kt = 0; kt < NT; ++kt) {
      const f32x4 d = Ds[kt * 64 + lane];
#pragma unroll
      for (int r = 0; r < 4; ++r) part = fmaf(W0s[16 * kt + 4 * q + r][2], d[r], part);
    }
    const float pair = part + __shfl_xor(part, 16);
    const float out = pair + __shfl_xor(pair, 32);
    if (rec && wave == 0 && lane < 16) {
      float *sc = rec + IONODE_RECORD_SCALARS(L, NT);
      sc[REC_X0 + lane] = x0; sc[REC_X1 + lane] = x1; sc[REC_SEED + lane] = seed; sc[REC_PAD + lane] = 0.0f;
    }
    __syncthreads();  // the next evaluation's layer 0 rewrites Hs[0] / Ds / Ps
    return out;
  }
};

// ionode_regress_kernel<NT> (ionode_regress.hpp) over GradMlpGen: the same tile loop, row fetch and loss partials; NT from the arguments.
// (A kernel of its own: a template parameter for the net on ionode_regress_kernel would rename the tuned kernels.  And a COPY of the tile
// loop: moved into one __forceinline__ routine over the net type, called from both kernels, the tuned units compile to other code --
// tried, their code objects differed; DESIGN_HISTORY.md, "the backward sweep's step algebra", met the same.  Correct both.)
__global__ void __launch_bounds__(256, GRAD_GEN_WG_PER_CU) ionode_regress_gen_kernel(const RArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int j = lane & 15;
  GArgs g;  // GradMlpGen::init reads the image pointer and the MLP shape only
  g.img = a.img; g.k.L = a.L; g.k.NT = a.NT;
  GradMlpGen mlp;
  mlp.init(g, smem, wave, lane);
  const int n_tiles = (a.M + 15) / 16;
  double acc = 0.0;
  struct In { float x0, x1, off, yt; };
  auto fetch = [&](int tile) -> In {
    const int row = tile * 16 + j;
    const int r = row < a.M ? row : a.M - 1;
    const f32x2 xx = *reinterpret_cast<const f32x2 *>(a.x + 2 * (size_t)r);
    return In{xx[0], xx[1], a.offset ? a.offset[r] : 0.0f, a.y[r]};
  };
  In nxt = fetch((int)blockIdx.x < n_tiles ? (int)blockIdx.x : 0);   // a tile's inputs are fetched one tile ahead
  for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const bool valid = tile * 16 + j < a.M;
    const In cur = nxt;
    if (tile + (int)gridDim.x < n_tiles) nxt = fetch(tile + (int)gridDim.x);
    const float x0 = cur.x0, x1 = cur.x1, off = cur.off, yt = cur.yt;
    const float ns = a.netscale;
    float resid = 0.0f;
    mlp.vjp_from_output(x0, x1, a.records + (size_t)tile * a.record_floats, [&](float net) -> float {
      // p = net / netscale (+ model_dadt), then MSELoss(sum): d loss / d net = 2 (p - y) / netscale   (all fp32, as torch)
      float p = net / ns;
      if (a.offset) p = p + off;
      resid = valid ? p - yt : 0.0f;
      return valid ? (2.0f * resid) / ns : 0.0f;
    });
    if (wave == 0 && lane < 16) acc += (double)resid * (double)resid;
  }
  // one partial per workgroup (deterministic; the host / Adam kernel sums them)
  if (wave == 0) {
    double t = (lane < 16) ? acc : 0.0;
#pragma unroll
    for (int s = 1; s < 16; s <<= 1) t += __shfl_xor(t, s);
    if (lane == 0) a.loss_part[blockIdx.x] = t;
  }
}

// ionode_grad_reduce_kernel<NT> (ionode_grad_reduce.hpp) at a run-time NT: same records, same partial layout (grad_partial_floats), and
// the same sums -- every output element is ONE chain over the slab's records in record order, trajectory groups c = 0..3 inside a
// record; the bias gradients fold (c0 + c1) + (c2 + c3), then the lane groups by shfl_xor 16, 32.  Only the deal of the elements differs:
// job 0 = both light jobs; a heavy job = (layer, column block of CB column tiles, row block of RB row tiles), row tile rb0 + wave + 4 i
// on wavefront `wave` (no full / remainder distinction: nothing is folded across wavefronts here).  The register tile is
// [RB / 4][CB] whatever NT is; tiles beyond NT are skipped by wave-uniform predicates.
__global__ void __launch_bounds__(256, GRAD_GEN_REDUCE_WG_PER_CU) ionode_grad_reduce_gen_kernel(const float *__restrict__ records, int64_t n_records, int n_slabs,
                                                                   int L, int NT, float *__restrict__ partials, int unit_seed) {
  constexpr int RB = GRAD_GEN_RB, CB = GRAD_GEN_CB, RW = RB / 4;
  constexpr int STE_MAX = (RB + CB) * 64;   // float4 elements staged per record at most: the row block's D_l tiles + the column block's H_{l-1} tiles
  constexpr int STG = STE_MAX / 256;        // float4 loads per thread per record
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  f32x4 *buf = reinterpret_cast<f32x4 *>(smem);  // [2][STE_MAX]

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int NP = 16 * NT;
  const int NRB = grad_gen_reduce_nrb(NT), NCB = grad_gen_reduce_ncb(NT);
  const int NJOB = L * NCB * NRB + 1;
  const int jobx = blockIdx.x % NJOB;
  const int slab = blockIdx.x / NJOB;
  const int64_t r0 = n_records * slab / n_slabs, r1 = n_records * (slab + 1) / n_slabs;
  const int64_t RECF = grad_record_floats(L, NT);
  float *__restrict__ out = partials + (size_t)slab * grad_partial_floats(L, NT);
  const int m = lane & 15, kk = lane >> 4;

  if (jobx == 0) {
    // ---- the two light jobs, four records in flight, 16 row tiles (four per wavefront) per pass over the slab ----
    constexpr int NB = 4;
    for (int lj = 0; lj < 2; ++lj) {
      const bool first = lj == 0;
      for (int p0 = 0; p0 < NT; p0 += RB) {
        float a0[RW], a1[RW], a2[RW];
#pragma unroll
        for (int i = 0; i < RW; ++i) a0[i] = a1[i] = a2[i] = 0.0f;
        float sg = 0.0f;
        for (int64_t rb = r0; rb < r1; rb += NB) {
          f32x4 t[NB][RW];
          float s0[NB][4], s1[NB][4], sd[NB][4], sgl[NB];
#pragma unroll
          for (int u = 0; u < NB; ++u) {
            const int64_t rr = (rb + u < r1) ? rb + u : r1 - 1;   // (past the end: a valid record, its contribution is skipped below)
            const float *rec = records + rr * RECF;
            const f32x4 *tiles = reinterpret_cast<const f32x4 *>(rec) + (size_t)(first ? (L + 1) * NT : L * NT) * 64;  // D_0 | H_L
            const float *sc = rec + IONODE_RECORD_SCALARS(L, NT);
#pragma unroll
            for (int c = 0; c < 4; ++c) {
              s0[u][c] = first ? sc[REC_X0 + 4 * c + kk] : sc[REC_SEED + 4 * c + kk];
              s1[u][c] = first ? sc[REC_X1 + 4 * c + kk] : 0.0f;
              sd[u][c] = sc[REC_SEED + 4 * c + kk];
            }
            sgl[u] = (lane < 16) ? sc[REC_SEED + lane] : 0.0f;
#pragma unroll
            for (int i = 0; i < RW; ++i) {
              const int rt = p0 + wave + 4 * i;
              t[u][i] = (rt < NT) ? tiles[rt * 64 + lane] : f32x4{0, 0, 0, 0};
            }
          }
#pragma unroll
          for (int u = 0; u < NB; ++u) {
            if (rb + u < r1) {
              if (!first && p0 == 0 && wave == 0 && lane < 16) sg += sgl[u];
#pragma unroll
              for (int i = 0; i < RW; ++i) {
                const int rt = p0 + wave + 4 * i;
                if (rt < NT) {
                  f32x4 tt = t[u][i];
                  if (first && unit_seed) {
#pragma unroll
                    for (int c = 0; c < 4; ++c) tt[c] *= sd[u][c];   // D_0 of a unit-seed record
                  }
#pragma unroll
                  for (int c = 0; c < 4; ++c) {
                    a0[i] += first ? tt[c] : tt[c] * s0[u][c];
                    if (first) { a1[i] = fmaf(tt[c], s0[u][c], a1[i]); a2[i] = fmaf(tt[c], s1[u][c], a2[i]); }
                  }
                }
              }
            }
          }
        }
#pragma unroll
        for (int i = 0; i < RW; ++i) {
          const int rt = p0 + wave + 4 * i;
          float v0 = a0[i], v1 = a1[i], v2 = a2[i];
          v0 += __shfl_xor(v0, 16); v0 += __shfl_xor(v0, 32);
          v1 += __shfl_xor(v1, 16); v1 += __shfl_xor(v1, 32);
          v2 += __shfl_xor(v2, 16); v2 += __shfl_xor(v2, 32);
          if (rt < NT && lane < 16) {
            if (first) {
              float *o = out + (size_t)(16 * rt + m) * 4;
              o[0] = v0; o[1] = v1; o[2] = v2; o[3] = 0.0f;
            } else {
              out[(size_t)4 * NP + (size_t)L * ((size_t)NP * NP + NP) + 16 * rt + m] = v0;
            }
          }
        }
        if (!first && p0 == 0 && wave == 0) {
          float tsum = (lane < 16) ? sg : 0.0f;
#pragma unroll
          for (int sft = 1; sft < 16; sft <<= 1) tsum += __shfl_xor(tsum, sft);
          if (lane == 0) {
            float *o = out + (size_t)4 * NP + (size_t)L * ((size_t)NP * NP + NP) + NP;
            o[0] = tsum; o[1] = o[2] = o[3] = 0.0f;
          }
        }
      }
    }
    return;
  }

  // ---- heavy job (l, cb0, rb0): dW_l[row block][column block] += D_l . H_{l-1}^T over this slab's records ----
  const int hj = jobx - 1;
  const int l = 1 + hj / (NCB * NRB);
  const int cb0 = ((hj / NRB) % NCB) * CB, rb0 = (hj % NRB) * RB;
  const int nrow = (NT - rb0 < RB) ? NT - rb0 : RB, ncol = (NT - cb0 < CB) ? NT - cb0 : CB;   // tiles of this block (>= 1)
  const int nown = (nrow - wave + 3) / 4;   // row tiles rb0 + wave + 4 i, i < nown, are this wavefront's (0 when wave >= nrow)
  const int STE = (nrow + ncol) * 64;
  f32x4 acc[RW][CB], dba[RW];
#pragma unroll
  for (int i = 0; i < RW; ++i) {
    dba[i] = f32x4{0, 0, 0, 0};
#pragma unroll
    for (int ct = 0; ct < CB; ++ct) acc[i][ct] = f32x4{0, 0, 0, 0};
  }
  // staging: element e = 64 * tile + lane of the record's {D_l tiles of the row block, H_{l-1} tiles of the column block}
  auto src_of = [&](int64_t rr, int e) -> const f32x4 * {
    const f32x4 *base = reinterpret_cast<const f32x4 *>(records + rr * RECF);
    return (e < nrow * 64) ? base + ((size_t)((L + 1) + l) * NT + rb0) * 64 + e                    // D_l
                           : base + ((size_t)(l - 1) * NT + cb0) * 64 + (e - nrow * 64);            // H_{l-1}
  };
  f32x4 stg[STG];
  float *seedbuf = reinterpret_cast<float *>(buf + (size_t)2 * STE_MAX);   // [2][16]: a unit-seed record's seeds, staged with its tiles
  auto seed_src = [&](int64_t rr) -> const float * { return records + rr * RECF + IONODE_RECORD_SCALARS(L, NT) + REC_SEED + (threadIdx.x & 15); };
  float sdg = 1.0f;
  if (r0 < r1) {
#pragma unroll
    for (int u = 0; u < STG; ++u) {
      const int e = threadIdx.x + 256 * u;
      if (e < STE) buf[e] = *src_of(r0, e);
    }
    if (unit_seed && threadIdx.x < 16) seedbuf[threadIdx.x] = *seed_src(r0);
  }
  __syncthreads();
  for (int64_t rr = r0; rr < r1; ++rr) {
    const int cur = (int)((rr - r0) & 1);
    const f32x4 *__restrict__ Db = buf + (size_t)cur * STE_MAX;
    const f32x4 *__restrict__ Hb = Db + nrow * 64;
    const bool more = rr + 1 < r1;
    if (more) {
#pragma unroll
      for (int u = 0; u < STG; ++u) {
        const int e = threadIdx.x + 256 * u;
        if (e < STE) stg[u] = *src_of(rr + 1, e);
      }
      if (unit_seed && threadIdx.x < 16) sdg = *seed_src(rr + 1);
    }
    f32x4 sd = f32x4{1.0f, 1.0f, 1.0f, 1.0f};
    if (unit_seed) {
#pragma unroll
      for (int c = 0; c < 4; ++c) sd[c] = seedbuf[cur * 16 + 4 * c + kk];   // this lane's component c is trajectory 4 c + kk
    }
    f32x4 af[RW];
#pragma unroll
    for (int i = 0; i < RW; ++i) {
      af[i] = f32x4{0, 0, 0, 0};
      if (i < nown) {
        af[i] = Db[(wave + 4 * i) * 64 + lane];
        if (unit_seed) af[i] = af[i] * sd;
        dba[i] += af[i];
      }
    }
#pragma unroll
    for (int ct = 0; ct < CB; ++ct) {
      if (ct < ncol) {   // wave-uniform
        const f32x4 b = Hb[ct * 64 + lane];
        // trajectory group c outer, row tile inner: consecutive MFMAs on different accumulators
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
          for (int i = 0; i < RW; ++i)
            if (i < nown) acc[i][ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[i][c], b[c], acc[i][ct], 0, 0, 0);
      }
    }
    if (more) {
      f32x4 *nb = buf + (size_t)(cur ^ 1) * STE_MAX;
#pragma unroll
      for (int u = 0; u < STG; ++u) {
        const int e = threadIdx.x + 256 * u;
        if (e < STE) nb[e] = stg[u];
      }
      if (unit_seed && threadIdx.x < 16) seedbuf[(cur ^ 1) * 16 + threadIdx.x] = sdg;
    }
    __syncthreads();
  }
  // ---- write the partial: accumulator register r of lane (q = lane >> 4, n' = lane & 15) is dW[16*rt + 4q + r][16*ct + n'] ----
  float *__restrict__ W = out + (size_t)4 * NP + (size_t)(l - 1) * ((size_t)NP * NP + NP);
  float *__restrict__ bvec = W + (size_t)NP * NP;
#pragma unroll
  for (int i = 0; i < RW; ++i) {
    if (i < nown) {
      const int rt = rb0 + wave + 4 * i;
#pragma unroll
      for (int ct = 0; ct < CB; ++ct) {
        if (ct < ncol) {
#pragma unroll
          for (int r = 0; r < 4; ++r) W[(size_t)(16 * rt + 4 * kk + r) * NP + 16 * (cb0 + ct) + m] = acc[i][ct][r];
        }
      }
      float s = (dba[i][0] + dba[i][1]) + (dba[i][2] + dba[i][3]);
      s += __shfl_xor(s, 16); s += __shfl_xor(s, 32);
      if (lane < 16 && cb0 == 0) bvec[16 * rt + m] = s;   // the bias gradient once per layer row (column block 0)
    }
  }
}

void launch_regress_gen(const RArgs &a, unsigned grid, hipStream_t s) {
  const size_t lds = grad_gen_lds_bytes(a.L, a.NT);
  raise_lds_limit(ionode_regress_gen_kernel, lds);
  hipLaunchKernelGGL(ionode_regress_gen_kernel, dim3(grid), dim3(256), lds, s, a);
}

hipError_t launch_grad_reduce_gen(int L, int NT, const float *records, int64_t n_records, int n_slabs, float *partials, hipStream_t s,
                                  int unit_seed) {
  const unsigned grid = (unsigned)(n_slabs * (L * grad_gen_reduce_ncb(NT) * grad_gen_reduce_nrb(NT) + 1));
  hipLaunchKernelGGL(ionode_grad_reduce_gen_kernel, dim3(grid), dim3(256), grad_gen_reduce_lds_bytes(), s, records, n_records, n_slabs, L,
                     NT, partials, unit_seed);
  return hipGetLastError();
}

}  // namespace ionode
