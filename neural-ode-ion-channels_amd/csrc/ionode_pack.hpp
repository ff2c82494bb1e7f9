// ionode_pack.hpp -- host only, included by ionode_capi.hip alone: the re-layout of an nn.Sequential state dict into the packed
// weight image the kernels stream (ionode_mlp_packed_floats / ionode_mlp_pack).  One size function and one packer per SECTION:
// Tuned widths:   layer 0 | L x (fragment stream, bias[NP]) | output layer | N <= 16: scalar row pairs | N = 200: 4-trajectory, one-trajectory sections
// Other widths:   layer 0 | L x (generic fragments, bias[NP]) | output layer
#pragma once
#include "ionode_plan.hpp"

namespace {

// Wavefronts per tile of the tuned 16-trajectory tile that serves width N (the fragment stream is laid out per wavefront); false: none.
bool tile_shape(int N, int *G) {
  const ionode::Variant *v = find_variant(IONODE_MODEL_NNF, 0, ionode::Net::Tile, ionode::Lean::General, 16, 0, np_of(N) / 16);
  if (!v) return false;
  *G = v->G;
  return true;
}

// widths without a tuned tile: the image of the run-time-width tile (ionode_mlp_gen.hpp MlpGen)
bool generic_width(int N) {
  int G;
  const int NT = np_of(N) / 16;
  return N >= 1 && !tile_shape(N, &G) && NT >= 2 && NT <= ionode::MlpGen::NT_MAX;
}

// 1 KiB fragments per wavefront per hidden layer: F per step, + R on the steps s % G == 0 (K-slices of the remainder tiles)
size_t frags_per_wave(int NT, int G) {
  const int F = NT / G, R = NT - G * F, NOWN = (NT + G - 1) / G;
  return (size_t)NT * F + (size_t)NOWN * R;
}

// the reference's flat state dict: W0[N][2], b0[N], L x (W[N][N], b[N]), wl[N], bl
struct FlatNet {
  const float *w;
  int L, N;
  const float *W0() const { return w; }
  const float *b0() const { return w + (size_t)2 * N; }
  const float *W(int l) const { return w + (size_t)3 * N + (size_t)l * ((size_t)N * N + N); }
  const float *b(int l) const { return W(l) + (size_t)N * N; }
  const float *wl() const { return W(L); }
};

// element (row, k) of a hidden layer, zero in the padding
inline float wpad(const float *W, int N, int row, int k) { return (row < N && k < N) ? W[(size_t)row * N + k] : 0.0f; }

// layer 0: rows {b0, w00, w01, 0}
size_t layer0_floats(int NP) { return 4 * (size_t)NP; }
void pack_layer0(const FlatNet &n, float *out) {
  for (int r = 0; r < n.N; ++r) {
    out[4 * r + 0] = n.b0()[r];
    out[4 * r + 1] = n.W0()[2 * r + 0];
    out[4 * r + 2] = n.W0()[2 * r + 1];
  }
}

// output layer: wl[NP], bl, 3 pad
size_t output_floats(int NP) { return (size_t)NP + 4; }
void pack_output(const FlatNet &n, int NP, float *out) {
  for (int k = 0; k < n.N; ++k) out[k] = n.wl()[k];
  out[NP] = n.wl()[n.N];
}

// one hidden layer of the 16-column fragment stream, then its bias[NP]
size_t stream_layer_floats(int NT, int G) { return (size_t)G * frags_per_wave(NT, G) * 256 + (size_t)16 * NT; }
void pack_stream_layer(const float *W, const float *b, int N, int NT, int G, float *dst) {
  const int F = NT / G, Rm = NT - G * F;
  const size_t FR = frags_per_wave(NT, G);
  // A operand of v_mfma_f32_16x16x4_f32: lane = 16q + m supplies row 16*rt + m, k = 16*kt + 4*q + r.
  // Stream order: wavefront wv | step s, k-tile kt = (s + wv) mod NT | fragments | lane.  F fragments hold the full
  // row tiles wv + i*G k-step-major (element e = r*F + i -> fragment e/4, component e%4); steps with s % G == 0 add
  // one fragment per remainder tile G*F + j (component = k-step r), zero when the step wraps (s + wv >= NT).
  for (int wv = 0; wv < G; ++wv) {
    size_t pos = 0;  // fragment index inside this wavefront's layer stream
    for (int st = 0; st < NT; ++st) {
      const int kt = (st + wv) % NT;
      for (int lane = 0; lane < 64; ++lane) {
        const int m = lane & 15, q = lane >> 4;
        float *f0 = dst + (((size_t)wv * FR + pos) * 64 + lane) * 4;
        // the asm tile's short form of the half-padded k-tile 12 (N <= 200, ionode_mlp_tile.hpp IONODE_KT12_SHORT): MFMA r = 0 takes
        // k = 192, 196, 193, 197 from the lane groups q = 0..3, MFMA r = 1 takes 194, 198, 195, 199; r = 2, 3 are not executed
        const bool short12 = IONODE_KT12_SHORT && NT == 13 && G == 4 && N <= 200 && kt == 12;
        auto kof = [&](int r) { return short12 ? (r < 2 ? 192 + 4 * (q & 1) + (q >> 1) + 2 * r : N) : 16 * kt + 4 * q + r; };
        for (int e = 0; e < 4 * F; ++e) {
          const int r = e / F, i = e % F, rt = wv + i * G;
          f0[(size_t)(e / 4) * 256 + e % 4] = wpad(W, N, 16 * rt + m, kof(r));
        }
        if (Rm > 0 && st % G == 0)
          for (int j = 0; j < Rm; ++j)
            for (int r = 0; r < 4; ++r)
              f0[(size_t)(F + j) * 256 + r] = (st + wv < NT) ? wpad(W, N, 16 * (G * F + j) + m, kof(r)) : 0.0f;
      }
      pos += F + ((Rm > 0 && st % G == 0) ? Rm : 0);
    }
  }
  float *bias = dst + (size_t)G * FR * 256;
  for (int r = 0; r < N; ++r) bias[r] = b[r];
}

// one hidden layer of the generic layout (MlpGen): [rt][kt][lane = 16 q + m] float4 over r of W[16 rt + m][16 kt + 4 q + r], then bias[NP]
void pack_generic_layer(const float *W, const float *b, int N, int NT, float *dst) {
  for (int rt = 0; rt < NT; ++rt)
    for (int kt = 0; kt < NT; ++kt)
      for (int lane = 0; lane < 64; ++lane) {
        const int m = lane & 15, q = lane >> 4;
        float *f = dst + (((size_t)rt * NT + kt) * 64 + lane) * 4;
        for (int r = 0; r < 4; ++r) f[r] = wpad(W, N, 16 * rt + m, 16 * kt + 4 * q + r);
      }
  float *bias = dst + (size_t)NT * NT * 256;
  for (int r = 0; r < N; ++r) bias[r] = b[r];
}

// one layer of the 4-trajectory tile's section (ionode_mlp_tile4.hpp MlpTile4), round-5 lane layout: wavefronts 0..2: [w][step s][q][lane = 4 b + i]
// float4 over r of W[row][16 kt + 4 q + r], block b = 4 g + u: row 16 (4 w + g) + 4 u + i, kt = (s + g) mod 13; wavefront 3 (partial chains of
// the remainder rows): [step j][q][lane] float4 over r of W[192 + 4 u + i][16 (c + 4 j) + 4 q + r] with c = g, -0.0f where c + 4 j > 12; then per
// (wavefront, lane) the accumulator start float4 {bias of rows i = 0..3 of the lane's block} (chains c > 0: 0)
void pack_tile4_layer(const float *W, const float *b, int N, float *lay) {
  for (int wv = 0; wv < 3; ++wv)
    for (int st = 0; st < 13; ++st)
      for (int q = 0; q < 4; ++q)
        for (int lane = 0; lane < 64; ++lane) {
          const int i = lane & 3, bb = lane >> 2, g = bb >> 2, u = bb & 3;
          float *f = lay + ((((size_t)wv * 13 + st) * 4 + q) * 64 + lane) * 4;
          const int row = 16 * (4 * wv + g) + 4 * u + i, kt = (st + g) % 13;
          for (int r = 0; r < 4; ++r) f[r] = wpad(W, N, row, 16 * kt + 4 * q + r);
        }
  float *rem = lay + (size_t)3 * 13 * 4 * 256;
  for (int jj = 0; jj < 4; ++jj)
    for (int q = 0; q < 4; ++q)
      for (int lane = 0; lane < 64; ++lane) {
        const int i = lane & 3, bb = lane >> 2, c = bb >> 2, u = bb & 3;
        float *f = rem + (((size_t)jj * 4 + q) * 64 + lane) * 4;
        const int row = 192 + 4 * u + i, kt = c + 4 * jj;
        for (int r = 0; r < 4; ++r) f[r] = (kt >= 13) ? -0.0f : wpad(W, N, row, 16 * kt + 4 * q + r);
      }
  float *bias = rem + (size_t)4 * 4 * 256;
  for (int wv = 0; wv < 4; ++wv)
    for (int lane = 0; lane < 64; ++lane) {
      const int bb = lane >> 2, g = bb >> 2, u = bb & 3;
      for (int i = 0; i < 4; ++i) {
        const int row = (wv < 3) ? 16 * (4 * wv + g) + 4 * u + i : 192 + 4 * u + i;
        bias[((size_t)wv * 64 + lane) * 4 + i] = (row < N && (wv < 3 || g == 0)) ? b[row] : 0.0f;
      }
    }
}

// one layer of the one-trajectory tile's section (ionode_mlp_row1.hpp MlpRow1): wavefronts 0..2: [w][step s][r][lane] float4 over q of
// W[64 w + lane][16 ((s + lane / 16) mod 13) + 4 q + r]; wavefront 3 (partial chains of the remainder rows): [step j][r][lane = 16 c + i]
// float4 over q of W[192 + i][16 (c + 4 j) + 4 q + r], -0.0f where c + 4 j > 12; then per (wavefront, lane) the accumulator start (the
// row's bias; chains c > 0: 0)
void pack_row1_layer(const float *W, const float *b, int N, float *lay) {
  for (int wv = 0; wv < 3; ++wv)
    for (int st = 0; st < 13; ++st)
      for (int r = 0; r < 4; ++r)
        for (int lane = 0; lane < 64; ++lane) {
          float *f = lay + ((((size_t)wv * 13 + st) * 4 + r) * 64 + lane) * 4;
          const int row = 64 * wv + lane, kt = (st + (lane >> 4)) % 13;
          for (int q = 0; q < 4; ++q) f[q] = wpad(W, N, row, 16 * kt + 4 * q + r);
        }
  float *rem = lay + (size_t)3 * 13 * 4 * 256;
  for (int j = 0; j < 4; ++j)
    for (int r = 0; r < 4; ++r)
      for (int lane = 0; lane < 64; ++lane) {
        float *f = rem + (((size_t)j * 4 + r) * 64 + lane) * 4;
        const int row = 192 + (lane & 15), kt = (lane >> 4) + 4 * j;
        for (int q = 0; q < 4; ++q) f[q] = (kt >= 13) ? -0.0f : wpad(W, N, row, 16 * kt + 4 * q + r);
      }
  float *bias = rem + (size_t)4 * 4 * 256;
  for (int wv = 0; wv < 4; ++wv)
    for (int lane = 0; lane < 64; ++lane) {
      const int row = (wv < 3) ? 64 * wv + lane : 192 + (lane & 15);
      bias[wv * 64 + lane] = (row < N && (wv < 3 || lane < 16)) ? b[row] : 0.0f;
    }
}

// scalar section (ionode_mlp_lane.hpp MlpLane), in row PAIRS (2 m, 2 m + 1) -- the two halves of a v_pk_fma_f32; an odd N's last
// pair has a zero second row.  Layer 0: {b0, b0'} {w00, w00'} {w01, w01'} {0, 0}.  Hidden layer l, pair m: {W[2m][k], W[2m+1][k]}
// for k = 4 q + r < N in the order r-major / q-minor (the order in which the 16 x 16 x 4 MFMA tile accumulates them), then the
// biases as bias + 0.0f (a -0 bias becomes +0: see MlpLane), pad to a multiple of 4 floats.
int scalar_pairs(int N) { return (N + 1) / 2; }
int scalar_block(int N) { return (2 * (N + 1) + 3) & ~3; }
size_t scalar_floats(int L, int N) { return (size_t)scalar_pairs(N) * 8 + (size_t)L * scalar_pairs(N) * scalar_block(N); }
void pack_scalar(const FlatNet &n, float *sc) {
  const int N = n.N, NPAIR = scalar_pairs(N), PB = scalar_block(N);
  float *sh = sc + NPAIR * 8;
  for (int j = 0; j < N; ++j) {
    const int m = j / 2, e = j % 2;
    sc[m * 8 + 0 + e] = n.b0()[j];
    sc[m * 8 + 2 + e] = n.W0()[2 * j + 0];
    sc[m * 8 + 4 + e] = n.W0()[2 * j + 1];
    for (int l = 0; l < n.L; ++l) {
      float *blk = sh + ((size_t)l * NPAIR + m) * PB;
      int pos = 0;
      for (int r = 0; r < 4; ++r)
        for (int q = 0; q < 4; ++q)
          if (4 * q + r < N) blk[2 * (pos++) + e] = n.W(l)[(size_t)j * N + 4 * q + r];
      blk[2 * N + e] = (N < 16) ? n.b(l)[j] + 0.0f : n.b(l)[j];
    }
  }
}

// where the sections of the image of an (L, N) net start; total == 0: no kernel serves the width
struct ImageLayout {
  bool generic = false;
  int G = 0, NP = 0, NT = 0;
  size_t layer = 0;   // floats per hidden layer of the main stream
  size_t hidden = 0, output = 0, scalar = 0, tile4 = 0, row1 = 0, total = 0;
};
ImageLayout image_layout(int L, int N) {
  ImageLayout y;
  if (L < 0 || N < 1) return y;
  y.generic = generic_width(N);
  if (!y.generic && !tile_shape(N, &y.G)) return y;
  y.NP = np_of(N); y.NT = y.NP / 16;
  y.layer = y.generic ? ionode::MlpGen::layer_floats(y.NT) : stream_layer_floats(y.NT, y.G);
  y.hidden = layer0_floats(y.NP);
  y.output = y.hidden + (size_t)L * y.layer;
  y.scalar = y.output + output_floats(y.NP);
  y.tile4 = y.scalar + ((!y.generic && y.NT == 1) ? scalar_floats(L, N) : 0);                       // N <= 16: the per-lane net's section
  y.row1 = y.tile4 + ((!y.generic && y.NT == 13) ? (size_t)L * ionode::MlpTile4::layer_floats() : 0);   // N = 200: the 4-trajectory tile's ...
  y.total = y.row1 + ((!y.generic && y.NT == 13) ? (size_t)L * ionode::MlpRow1::layer_floats() : 0);    // ... and the one-trajectory tile's
  return y;
}

// ionode_mlp_pack
int pack_image(const float *w, int L, int N, float *out) {
  if (!w || !out || L < 0 || N < 1) { set_err("ionode_mlp_pack: bad argument"); return IONODE_ERR_ARG; }
  const ImageLayout y = image_layout(L, N);
  if (y.total == 0) { set_err("ionode_mlp_pack: MLP width outside the supported range (1 <= N <= 512)"); return IONODE_ERR_UNSUPPORTED; }
  const FlatNet n = {w, L, N};
  memset(out, 0, y.total * sizeof(float));
  pack_layer0(n, out);
  for (int l = 0; l < L; ++l) {
    float *dst = out + y.hidden + (size_t)l * y.layer;
    if (y.generic) pack_generic_layer(n.W(l), n.b(l), N, y.NT, dst);
    else pack_stream_layer(n.W(l), n.b(l), N, y.NT, y.G, dst);
  }
  pack_output(n, y.NP, out + y.output);
  if (y.tile4 > y.scalar) pack_scalar(n, out + y.scalar);
  for (int l = 0; l < L && y.row1 > y.tile4; ++l) pack_tile4_layer(n.W(l), n.b(l), N, out + y.tile4 + (size_t)l * ionode::MlpTile4::layer_floats());
  for (int l = 0; l < L && y.total > y.row1; ++l) pack_row1_layer(n.W(l), n.b(l), N, out + y.row1 + (size_t)l * ionode::MlpRow1::layer_floats());
  return IONODE_OK;
}

}  // namespace
