// ionode_grad_step.hpp -- what the backward sweep's kernels and their host share (ionode_grad.hpp: the one-phase sweep and its
// fused sum-of-squares variant in ionode_grad_sweep_body.hpp, the two-phase recompute and walk kernels; ionode_grad_gc.hpp: the fused
// objective's G_c kernel for the two-phase sweep; ionode_grad_reduce.hpp):
// the argument block and the layouts of the streams between the launches, each named once.  The algebra of a step is still
// written per kernel: shared routines compiled to other code (DESIGN_HISTORY.md, "the backward sweep's step algebra").
#pragma once

#include "ionode_kargs.hpp"

namespace ionode {

struct GArgs {
  KArgs k;                 // protocol lookup fields (prot_t, Np, prot_t0, prot_dt, v_oob), params, prot_v, prot_of_traj, t_eval, B, Nt, P, L, N, NP, NT
  const float *img;        // grad image (ionode_grad_pack)
  const double *ckpt;      // [B][ckpt_cap][CkptRecord<D>::WIDTH] accepted-step records of the forward launch
  const int32_t *nacc;     // [B] accepted steps to replay (0: nothing to differentiate, e.g. a failed trajectory)
  const void *grad_y;      // [B][Nt][D] dL/dy_out in the state dtype; two-phase kernels: NULL = the fused objective (G_c and the sample-0 term come from ionode_grad_sse_gc_kernel)
  double *state;           // [B][2 * D + NPAR] adjoint state carried between chunk launches: lam[D], mu[D], gp[NPAR]
  float *records;          // [n_tiles][it_end - it_begin][6][record_floats] (d, h) stream for ionode_grad_reduce, or NULL
  double *grad_params;     // [B][NPAR]   written by the launch with it_end == n_iter
  double *grad_y0;         // [B][D]
  int32_t ckpt_cap, it_begin, it_end, n_iter;
  int64_t record_floats;
  double *packets;            // two-phase sweep: the adjoint-independent scalars of every (tile, step): [n_tiles][it_end - it_begin][16][GRAD_PACKET] fp64
  int32_t reserved;           // (was the host's kernel selector; kept so that the offsets of the fields behind it, and with them every kernel's argument loads, stay as they were)
  // fused objective's seed (ionode_dopri5_backward_sse_kernel; grad_y unused): dL/dy_k is formed in the kernel from
  // dL/dsse[b] and the residual of sample k against sse_ref -- no [B][Nt][D] gradient exists.  k.obj_abs: the objective's kind
  // (squares or absolute values: residual_weight, ionode_interp.hpp)
  const double *grad_sse;     // [B] upstream dL/dsse: the gradient of the trajectory's sum, whichever kind it is
  const double *sse_ref;      // [P][Nt] reference currents
  const double *v_tab;        // optional [P][Nt] V(t_k) (ionode_protocol_at_outputs), or NULL: protocol_v per sample
  double obs_g, obs_e;
  int32_t obs_open;
  double *sse_y0;             // two-phase fused objective: [B][D] sample-0 term of dL/dy0 (ionode_grad_sse_gc_kernel writes it, the walk adds it where grad_y is NULL)
};

// ---- packet of one trajectory and step (two-phase sweep, fp64): what the recompute kernel hands to the walk ----
namespace pkt {
constexpr int DTS = 0, STEP = 1, INITEV = 2;   // step length in the state dtype; flags (0.0 / 1.0); [3] spare
constexpr int GC = 4;                          // G_c[d] at GC + c * D + d: interpolant-coefficient adjoint sums (D = 2)
constexpr int STAGE = 16, STAGE_W = 8;         // stage e = 0..5 (i = 5 - e) at STAGE + STAGE_W * e: the eight fields below
constexpr int V = 0, Y0 = 1, Y1 = 2, E3 = 3, E4 = 4, E1 = 5, E2 = 6, C = 7;   // V, Y_i, exp(p6 V), exp(-p8 V), exp(p2 V), exp(-p4 V), c = d net / d x1 at unit seed
}  // namespace pkt
constexpr int GRAD_PACKET = pkt::STAGE + pkt::STAGE_W * 6;
static_assert(GRAD_PACKET == 64 && pkt::GC + 5 * 2 <= pkt::STAGE, "one packet: eight 64-byte lines");

// ---- record of one tile evaluation (fp32): H_0..H_L, D_0..D_L (NT tiles of 64 lanes x float4 each), then a scalar block of 16 x
// {x0, x1, seed, pad} (ionode_grad_reduce.hpp reads it; the walk writes the seeds of unit-seed records) ----
// (the scalar block's offset is a macro, and the tile part is spelled once per integer type: the record count multiplies the signed form,
// pointers add the unsigned one, and behind a function call or a conversion the kernels compile to other code -- DESIGN_HISTORY.md)
__host__ __device__ constexpr int64_t grad_record_floats(int L, int NT) { return (int64_t)2 * (L + 1) * NT * 256 + 64; }
#define IONODE_RECORD_SCALARS(L, NT) ((size_t)2 * ((L) + 1) * (NT) * 256)   // float offset of the scalar block
constexpr int REC_X0 = 0, REC_X1 = 16, REC_SEED = 32, REC_PAD = 48;
static_assert(grad_record_floats(5, 13) == (int64_t)IONODE_RECORD_SCALARS(5, 13) + REC_PAD + 16, "scalar block: 4 x 16 floats behind the tiles");

// ---- checkpoint record of one accepted step (fp64, written by the forward: ionode_attempt_body.hpp): [t0, dt, oi, nout, y[D], k1..k7[D]] ----
template <int D>
struct CkptRecord {
  static constexpr int T0 = 0, DT = 1, OI = 2, NOUT = 3, Y = 4, K = Y + D, WIDTH = 4 + 8 * D;
};

__host__ __device__ constexpr size_t grad_closed_lds_bytes(int D) { return (size_t)16 * 5 * D * 8; }   // [16][5 * D] fp64 G_c scratch: all the LDS of a sweep without a net

}  // namespace ionode
