// ionode_mlp_tile4.hpp -- MlpTile4 / MlpShrink4: N = 200 at four trajectories per tile (included by ionode_device.hpp, behind KArgs).
#pragma once

namespace ionode {

// ---------------------------------------------------------------------------------------------
// N = 200 at FOUR trajectories per tile: the small-batch / single-call form (round 4).  The reference's own scripts call
// odeint with ONE trajectory (train-s1.py:319-330, 32 sequential solves at :566-580), and BASELINE configs[4]'s per-GPU share is 1024
// trajectories: at 16 per tile those occupy 64 of 256 compute units and every RHS evaluation still costs a full 16-column MFMA
// pass (36.6 k cycles).  Here a tile is 4 trajectories (256 tiles for 1024 trajectories: the whole chip) and a hidden layer is
// 13 x 16 v_mfma_f32_4x4x1_16B_f32 per wavefront: 16 blocks of (4 rows) x (4 trajectories) x (1 k) -- each block an exact fmaf
// per element, so a block's accumulator runs the SAME chain as a row of the 16-column tile when it is fed the same k sequence.
//   lane = 4 b + i supplies A = W[row(b, i)][k];  lane = 4 b + j supplies B = h[k][trajectory j];  D[i][j] = VGPR i of lane 4 b + j
//   wavefront w, block b = 4 g + u:  g < 3: full row tile w + 4 g, rows 16 (w + 4 g) + 4 u + i -- all three tiles have rt % 4 == w, so
//                                    the whole wavefront walks the k-tiles in ONE rotated order kt = (s + w) mod 13, s = 0 .. 12;
//                                    g == 3: remainder tile 12, rows 192 + 4 u + i, partial chain w (k-tiles kt % 4 == w, ascending):
//                                    exactly the steps s % 4 == 0 with s + w < 13 of that same walk; on the other steps its A operand
//                                    is -0.0f (x + (-0 * h) == x for every x as long as h is finite and the chain is not at -0)
//   within a k-tile:  for r: for q: k = 16 kt + 4 q + r      (the canonical order; one MFMA per (r, q))
// so results are bit-identical to MlpTile<4, 4, 13, 13> and to the oracle.  Activations live in LDS as [k / 4][trajectory] float4
// (a lane reads the 4 x float4 of a k-tile for ITS trajectory; an output block IS one such float4); the remainder tile's four partial
// sums meet in LDS and every lane folds them itself ((p0 + p1) + (p2 + p3), LeakyReLU) when the walk reaches k-tile 12.
// Weights stream from L2 as in the 16-column tile (SRSRC buffer loads into a register ring one layer ahead: 13 steps x 4 float4),
// in their own image section (ionode_mlp_pack): layer | wavefront | step | q | lane -> float4 over r, then the layer's bias float4s.
// ---------------------------------------------------------------------------------------------
struct MlpTile4 {
  static constexpr int GW = 4, NT = 13, NP = 208;
  static constexpr int SLOTS = NT + 3;               // k-tile slots per activation buffer: tiles 0..2 are stored twice (slot kt and kt + 13), so
                                                     // that a block whose row tile rotates from k-tile g reads its walk kt = (s + g) mod 13 at the LINEAR slot s + g
  static constexpr int ACT = SLOTS * 16;             // float4 per activation buffer: [slot][q][trajectory]
  // Round 5: the lane layout of the one-trajectory tile (MlpRow1).  Wavefronts 0..2 hold 64 FULL rows each -- 16 blocks of 4 rows: block
  // b = 4 g + u is rows 16 (4 w + g) + 4 u + i, whose canonical chain rotates from k-tile g (the B operand is read per lane, so the four
  // block groups of a wavefront walk four rotations) -- and wavefront 3 holds the four partial chains of the sixteen remainder rows (block
  // 4 c + u: chain c of rows 192 + 4 u + i; 4 steps instead of 13), folded (p0 + p1) + (p2 + p3) across its lane groups.  172 one-KiB weight
  // loads per layer instead of 208 (round 4: every wavefront 48 rows + a remainder chain): this tile's walk waits on the compute unit's
  // vector-memory path as much as on the 4x4x1 MFMA's dependent issue (without its refills an evaluation takes 8.4 instead of 10.2 us).
  static constexpr int FRAGS_FULL = NT * 4, FRAGS_REM = 4 * 4;   // 1 KiB fragments per layer of a full-row wavefront / of the remainder wavefront
  static constexpr size_t layer_floats() { return (size_t)(3 * FRAGS_FULL + FRAGS_REM) * 256 + (size_t)4 * 256; }   // fragments + accumulator-start float4 per (wave, lane)
  static __host__ __device__ constexpr size_t lds_bytes(int L) {
    return ((size_t)2 * ACT + NP) * 16 + ((size_t)NP + 4) * 4 + (size_t)L * 64 * 16;   // activations x2, W0 rows, wl + bl, accumulator starts [L][wave][block]
  }
  f32x4 ring[NT][4];
  f32x4 w0r[4];    // layer 0: the four rows {b0, w00, w01, 0} of this lane's output block
                   // (round 4 also kept the lane's chain of the output weights resident: 52 registers the two walk forms of round 5 need;
                   // they are read from LDS together with the thirteen activation reads of the output layer -- one round trip)
  f32x4 *Hs;
  const f32x4 *W0s, *B4s;
  const float *wlS;
  __amdgpu_buffer_rsrc_t rsrc;
  unsigned voff, sec0, lbytes;
  int L, wave, lane;
#ifdef IONODE_STAMPS
  Stamps *sp;
#endif
  // offset (floats) of the T4 section inside the packed image of (L, N = 200): behind the 16-column image
  static __host__ __device__ constexpr size_t section_off(int L) {
    return 4 * (size_t)NP + (size_t)L * ((size_t)4 * 43 * 256 + NP) + NP + 4;   // MlpTile<4, 4, 13, 13>: FRAGS = 13 * 3 + 4 = 43 per wavefront
  }
  __device__ __forceinline__ f32x4 frag(unsigned lbase, int n) const {
    using u32x4 = __attribute__((ext_vector_type(4))) unsigned;
    const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rsrc, voff, lbase + (unsigned)n * 1024u, 0);
    return __builtin_bit_cast(f32x4, v);
  }
  __device__ __forceinline__ void init(const KArgs &a, unsigned char *smem, int wave_, int lane_, int first_traj = 0) {
    L = a.L; wave = wave_; lane = lane_;
    const float *__restrict__ img = a.mlp + (a.traj_per_img > 0 ? (size_t)(first_traj / a.traj_per_img) * (size_t)a.mlp_stride : (size_t)0);
    Hs = reinterpret_cast<f32x4 *>(smem);
    f32x4 *w0 = Hs + 2 * ACT;
    float *ws = reinterpret_cast<float *>(w0 + NP);
    const int tid = wave * 64 + lane;
    const f32x4 *src = reinterpret_cast<const f32x4 *>(img);
    for (int i = tid; i < NP; i += 256) w0[i] = src[i];
    const float *wl = img + 4 * (size_t)NP + (size_t)L * ((size_t)4 * 43 * 256 + NP);
    for (int i = tid; i < NP + 4; i += 256) ws[i] = wl[i];
    W0s = w0; wlS = ws;
    // accumulator starts of every layer and block (the four lanes of a block share them) into LDS: fetched from the image at the start
    // of a layer they would cost an L2 round trip per layer on the critical path of a single trajectory
    f32x4 *b4 = reinterpret_cast<f32x4 *>(ws + NP + 4);
    const size_t sec = section_off(L);
    for (int i = tid; i < L * 64; i += 256) {
      const int l = i >> 6, wv = (i >> 4) & 3, bb = i & 15;
      b4[i] = *reinterpret_cast<const f32x4 *>(img + sec + (size_t)l * layer_floats() + (size_t)(3 * FRAGS_FULL + FRAGS_REM) * 256 + (size_t)wv * 256 + (size_t)bb * 16);
    }
    B4s = b4;
    const size_t img_bytes = (sec + (size_t)L * layer_floats()) * 4;
    rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(img), 0, (int)img_bytes, 0x00020000);
    sec0 = (unsigned)(sec * 4);
    lbytes = (unsigned)(layer_floats() * 4);
    voff = (unsigned)(wave * FRAGS_FULL * 1024 + lane * 16);
#pragma unroll
    for (int s = 0; s < NT; ++s)
#pragma unroll
      for (int q = 0; q < 4; ++q) ring[s][q] = (L > 0 && (wave < 3 || s < 4)) ? frag(sec0, s * 4 + q) : f32x4{0, 0, 0, 0};
    {
      const int b = lane >> 2, kq0 = 16 * wave + b;
#pragma unroll
      for (int r = 0; r < 4; ++r) w0r[r] = (kq0 < NP / 4) ? src[4 * kq0 + r] : f32x4{0, 0, 0, 0};
    }
    __syncthreads();
  }
  // store an output block (4 rows of k-tile kt, lane group q, trajectory j); tiles 0..2 also at their second slot
  __device__ __forceinline__ void put_h(f32x4 *__restrict__ H, int kt, int q, int j, f32x4 h) const {
    H[(kt * 4 + q) * 4 + j] = h;
    if (kt < 3) H[((kt + NT) * 4 + q) * 4 + j] = h;
  }
  // The steps of this lane's block: step s reads the four float4 {h[16 kt + 4 q + r]}_r of the lane's trajectory from slot (slot0 + s * stride)
  // and runs the sixteen MFMAs of the k-tile in the canonical order (r-major, q-minor); the ring's fragments of the step are refilled for the
  // coming layer right behind their last use.  ONE code path for both kinds of wavefront (two instantiations merged the 208-register ring
  // through a branch and spilled): the remainder wavefront leaves after its four steps (a wave-uniform exit), its slot stride is a run-time value.
  __device__ __forceinline__ void walk(f32x4 &acc, const f32x4 *__restrict__ Bw, int sstride, int nsteps, unsigned lnext) {
    f32x4 hn[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) hn[q] = Bw[q * 4];
#pragma unroll
    for (int s = 0; s < NT; ++s) {
      if (s == 4 && nsteps == 4) break;
      f32x4 hq[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) hq[q] = hn[q];
      if (s + 1 < NT) {
#pragma unroll
        for (int q = 0; q < 4; ++q) hn[q] = Bw[(s + 1) * sstride + q * 4];
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
#pragma unroll
        for (int q = 0; q < 4; ++q) acc = __builtin_amdgcn_mfma_f32_4x4x1f32(ring[s][q][r], hq[q][r], acc, 0, 0, 0);
        if (r == 3) {
#pragma unroll
          for (int q = 0; q < 4; ++q) ring[s][q] = frag(lnext, s * 4 + q);
        }
        __builtin_amdgcn_sched_barrier(0);
      }
    }
  }
  __device__ __forceinline__ float eval(float x0, float x1) {
    const int j = lane & 3, b = lane >> 2, g = b >> 2, u = b & 3;
    MSTAMP(0);  // slot 0: everything outside the MLP
    // layer 0: Linear(2, N) + LeakyReLU; the lane fills output block (kt, q) = (4 wave + g, u) = kq / 4, kq % 4 of its trajectory
    {
      const int kq = 16 * wave + b;
      if (kq < NP / 4) {
        f32x4 h;
#pragma unroll
        for (int r = 0; r < 4; ++r) h[r] = lrelu(fmaf(w0r[r][2], x1, fmaf(w0r[r][1], x0, w0r[r][0])));
        put_h(Hs, kq >> 2, kq & 3, j, h);
      }
    }
    f32x4 acc_next = (L > 0) ? B4s[wave * 16 + b] : f32x4{0, 0, 0, 0};
    __syncthreads();
    MSTAMP(1);  // slot 1: layer 0 + barrier
    for (int l = 0; l < L; ++l) {
      const f32x4 *__restrict__ Hin = Hs + (l & 1) * ACT;
      f32x4 *__restrict__ Hout = Hs + ((l + 1) & 1) * ACT;
      const int ln = (l + 1 < L) ? l + 1 : 0;   // the ring runs cyclically over the hidden stack (see MlpTile)
      const unsigned lnext = sec0 + (unsigned)ln * lbytes;
      // accumulators: D[i][j] = VGPR i: bias of row i of my block (partial chains c > 0 of the remainder rows start at 0: the image says so);
      // read one layer ahead
      f32x4 acc = acc_next;
      if (l + 1 < L) acc_next = B4s[((l + 1) * 4 + wave) * 16 + b];
      MSTAMP(2);  // slot 2: layer prologue
      // full rows (wavefronts 0..2): block group g walks k-tile (s + g) mod 13 = slot s + g, 13 steps; remainder rows (wavefront 3): block
      // group c = g runs partial chain c over the k-tiles c, c + 4, c + 8 (, 12: chain 0 only -- the others' step 3 reads the duplicate slots
      // 13..15 against -0.0f weights): 4 steps, 4 slots apart
      walk(acc, Hin + (g * 4) * 4 + j, (wave < 3) ? 16 : 64, (wave < 3) ? NT : 4, lnext);
      MSTAMP(3);  // slot 3: the MFMA walk
      if (wave < 3) {
        f32x4 h;
#pragma unroll
        for (int r = 0; r < 4; ++r) h[r] = lrelu(acc[r]);
        put_h(Hout, 4 * wave + g, u, j, h);
      } else {
        // the four chains of a row meet across the lane groups: (p0 + p1) + (p2 + p3)
        f32x4 h;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float pair = acc[r] + __shfl_xor(acc[r], 16);
          h[r] = lrelu(pair + __shfl_xor(pair, 32));
        }
        if (lane < 16) put_h(Hout, NT - 1, u, j, h);
      }
      __syncthreads();
      MSTAMP(4);  // slot 4: LeakyReLU + store + layer barrier
    }
    // Linear(N, 1): chain q = b & 3 per lane (k = 16 kt + 4 q + r, kt ascending, r ascending), folded ((p0 + p1) + (p2 + p3)) + bl
    const f32x4 *__restrict__ Hin = Hs + (L & 1) * ACT;
    const int q = b & 3;
    // all thirteen activation reads in flight at once: one LDS round trip instead of thirteen
    f32x4 hl[NT], wv[NT];
#pragma unroll
    for (int kt = 0; kt < NT; ++kt) {
      hl[kt] = Hin[(kt * 4 + q) * 4 + j];
      wv[kt] = *reinterpret_cast<const f32x4 *>(wlS + 16 * kt + 4 * q);
    }
    float part = 0.0f;
#pragma unroll
    for (int kt = 0; kt < NT; ++kt) {
#pragma unroll
      for (int r = 0; r < 4; ++r) part = fmaf(wv[kt][r], hl[kt][r], part);
    }
    const float pair = part + __shfl_xor(part, 4);    // (p0 + p1) or (p2 + p3): lanes 4 apart hold neighbouring chains
    const float out = (pair + __shfl_xor(pair, 8)) + wlS[NP];
    if ((L & 1) == 0) __syncthreads();   // the next evaluation's layer 0 rewrites buffer 0, which an even stack's last layer reads (odd: buffer 1)
    MSTAMP(5);  // slot 5: Linear(N, 1) + closing barrier
    return out;
  }
};

// ---------------------------------------------------------------------------------------------
// The 4-trajectory net behind the 16-trajectory tile's lane layout (round 6): the tail of a 16-tile solve.  Trajectories of a tile
// stop after their own number of attempts, and a tile's last few hundred attempts run with <= 4 live slots -- at the full 16-column
// price.  Once <= 4 are live, the lean 16-tile kernel swaps its net for this one; the Runge-Kutta, controller and emission code keeps
// the 16-tile layout (lane 16 q + j = slot j) and stays as it is.
//   init: the live slots s_0 < s_1 < ... (<= 4; a uniform mask: every wavefront holds all 16 slots) get the 4-tile's columns c = 0, 1, ...
//   eval: 4-tile lane 4 b + c fetches the stage input of slot s_c (ds_bpermute from lane s_c), runs MlpTile4::eval, and 16-tile lane
//         16 q + j takes its result from lane c(j) -- the 4-tile leaves trajectory c's output in lane c.  Columns without a live slot
//         evaluate s_0's input again (finite, unused); slots that die later keep their column, whose output nobody reads.
// Each column of an MFMA depends on its own B operand only, so trajectory j's value is MlpTile4's for its input: the same bits as the
// 16-tile's (test_four_trajectory_tile_is_bit_identical).
// ---------------------------------------------------------------------------------------------
struct MlpShrink4 {
  MlpTile4 t4;
  int src;   // lane 4 b + c: the 16-tile lane (slot s_c) whose stage input column c evaluates
  int dst;   // lane 16 q + j: the 4-tile lane (column c of slot j) holding slot j's result
  __device__ __forceinline__ void init(const KArgs &a, unsigned char *smem, int wave_, int lane_, int first_traj, unsigned live) {
    const int c = lane_ & 3, j = lane_ & 15;
    unsigned m = live;   // drop the c lowest live slots: slot s_c is then the lowest left (none left: s_0)
#pragma unroll
    for (int i = 0; i < 3; ++i)
      if (i < c) m &= m - 1;
    src = __builtin_ctz(m ? m : live);
    dst = ((live >> j) & 1u) ? __builtin_popcount(live & ((1u << j) - 1u)) : 0;
    t4.init(a, smem, wave_, lane_, first_traj);
  }
  __device__ __forceinline__ float eval(float x0, float x1) {
    const float out = t4.eval(__shfl(x0, src), __shfl(x1, src));
    return __shfl(out, dst);
  }
};

}  // namespace ionode
