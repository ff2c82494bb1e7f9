// ionode_rhs.hpp -- the right-hand sides: func.forward(t, y) of the reference per lane (included by ionode_device.hpp, behind KArgs).
#pragma once

namespace ionode {

// Closed-form models carry an empty stand-in so the integrator code is shared.
struct NoMlp {
  static constexpr int GW = 1;
  __device__ __forceinline__ float eval(float, float) { return 0.0f; }
};

// ---------------------------------------------------------------------------------------------
// func.forward(t, y) of the reference, per lane.  The protocol voltage at the stage time (and whether
// the time was inside the protocol's range) is looked up by the caller, ahead of the stage.
// ---------------------------------------------------------------------------------------------
// (rate constants of one stage voltage; see closed_rates() below)
template <int MODEL> struct ClosedRates {
  static constexpr int NR = (MODEL == IONODE_MODEL_MARKOV6) ? 6 : 4;
  double k[NR];
  float kf[NR];
  bool oob32;
};
template <int MODEL, typename S, bool WIDE = false, typename MLP>
__device__ __forceinline__ void rhs(const KArgs &a, const double *p, double v, bool inrange, const S *y, S *f,
                                    MLP &mlp, ClosedRates<IONODE_MODEL_HH2> *cr = nullptr, bool fresh = true) {
  using MT = ModelTraits<MODEL>;
  constexpr bool F32 = sizeof(S) == 4;

  if constexpr (MODEL == IONODE_MODEL_MARKOV6) {
    if (F32 && !inrange) {
      // v = torch.tensor([-80]) is int64: `p * v` is float32 and exp runs in fp32 (train-d1.py:169-178)
      const float vf = (float)a.v_oob;
      const float a1 = (float)p[0] * det_expf((float)p[1] * vf);
      const float b1 = (float)p[2] * det_expf((float)(-p[3]) * vf);
      const float bh = (float)p[4] * det_expf((float)p[5] * vf);
      const float ah = (float)p[6] * det_expf((float)(-p[7]) * vf);
      const float a2 = (float)p[8] * det_expf((float)p[9] * vf);
      const float b2 = (float)p[10] * det_expf((float)(-p[11]) * vf);
      const float c1 = y[0], c2 = y[1], i_ = y[2], ic1 = y[3], ic2 = y[4], o = y[5];
      f[0] = a1 * c2 + ah * ic1 + b2 * o - (b1 + bh + a2) * c1;
      f[1] = b1 * c1 + ah * ic2 - (a1 + bh) * c2;
      f[2] = a2 * ic1 + bh * o - (b2 + ah) * i_;
      f[3] = a1 * ic2 + bh * c1 + b2 * i_ - (b1 + ah + a2) * ic1;
      f[4] = b1 * ic1 + bh * c2 - (ah + a1) * ic2;
      f[5] = a2 * c1 + ah * i_ - (b2 + bh) * o;
      return;
    }
    const double a1 = p[0] * det_exp(p[1] * v);
    const double b1 = p[2] * det_exp(-p[3] * v);
    const double bh = p[4] * det_exp(p[5] * v);
    const double ah = p[6] * det_exp(-p[7] * v);
    const double a2 = p[8] * det_exp(p[9] * v);
    const double b2 = p[10] * det_exp(-p[11] * v);
    const double c1 = y[0], c2 = y[1], i_ = y[2], ic1 = y[3], ic2 = y[4], o = y[5];
    f[0] = (S)(a1 * c2 + ah * ic1 + b2 * o - (b1 + bh + a2) * c1);
    f[1] = (S)(b1 * c1 + ah * ic2 - (a1 + bh) * c2);
    f[2] = (S)(a2 * ic1 + bh * o - (b2 + ah) * i_);
    f[3] = (S)(a1 * ic2 + bh * c1 + b2 * i_ - (b1 + ah + a2) * ic1);
    f[4] = (S)(b1 * ic1 + bh * c2 - (ah + a1) * ic2);
    f[5] = (S)(a2 * c1 + ah * i_ - (b2 + bh) * o);
    return;
  } else {
    constexpr bool HAS_HH_A = (MODEL == IONODE_MODEL_HH2 || MODEL == IONODE_MODEL_NND);
    const S av = y[0], rv = y[1];
    const bool oob32 = F32 && !inrange;

    // MLP term first: it is a tile-wide collective, so every lane takes part whatever its branch below
    float net = 0.0f;
    if constexpr (MT::MLP) {
      const float vf = (float)a.v_oob;
      // v / self.vrange, then .float(); net / self.netscale -- exact quotients by the constants 100 and 1000 (div_const)
      const float nv = oob32 ? vf / 100.0f : (float)div_const(v, 100.0, 0.01);
      if constexpr (WIDE) net = div_constf(mlp.eval_tiny64(nv, (float)av), 1000.0f, 0.001f);  // 64 trajectories per wavefront (N <= 16)
      else net = div_constf(mlp.eval(nv, (float)av), 1000.0f, 0.001f);
    }

    if (oob32) {
      const float vf = (float)a.v_oob;
      const float af = (float)av, rf = (float)rv;
      const float k3 = (float)p[4] * det_expf((float)p[5] * vf);
      const float k4 = (float)p[6] * det_expf((float)(-p[7]) * vf);
      const float drdt = -k3 * rf + k4 * (1.0f - rf);
      float dadt = 0.0f;
      if constexpr (HAS_HH_A) {
        const float k1 = (float)p[0] * det_expf((float)p[1] * vf);
        const float k2 = (float)p[2] * det_expf((float)(-p[3]) * vf);
        dadt = k1 * (1.0f - af) - k2 * af;
      }
      if constexpr (MT::MLP) dadt = (MODEL == IONODE_MODEL_NND) ? dadt + net : net;
      f[0] = (S)dadt;
      f[1] = (S)drdt;
      return;
    }
    const S one_m_a = (S)1 - av;  // `1. - a` / `self.unity - r` are formed in y.dtype
    const S one_m_r = (S)1 - rv;
    // (not for the 64-per-wavefront N <= 16 kernel: two interleaved branch-free exps cost ~30 registers -- it went from 252 to 284
    // VGPRs, i.e. from two wavefronts per SIMD to one, 58 -> 87 ms)
    // (the 4-trajectory tile keeps a 208-register weight ring: the branchy form with one exp in flight, same bits)
    constexpr bool TIGHT = std::is_same<MLP, MlpTile4>::value || std::is_same<MLP, MlpShrink4>::value || std::is_same<MLP, MlpRow1>::value ||
                           std::is_same<MLP, MlpRow1Deep>::value;
    auto dexp = [](double x) { if constexpr (TIGHT) return det_exp_ldexp(x); else if constexpr (MT::MLP && !WIDE) return det_exp_s(x); else return det_exp(x); };
    double k3, k4, dadt = 0.0;
    if constexpr (MT::MLP && WIDE) {
      // one trajectory per lane (N <= 16): the closed-form kernels' exp -- addend constants as scalar operands, one v_ldexp_f64, and
      // the three range cases skipped when every lane's arguments are in range (closed_rates); same operations, same bits
      // (round 5) the rates depend on the stage VOLTAGE only: the integrator says `fresh = false` when every lane of the wavefront sees the
      // previous stage's voltage again (stage 6 always; every stage on a protocol's plateaus) and the products kept in *cr are reused
      constexpr int NX = HAS_HH_A ? 4 : 2;
      double kk[4];
      if (fresh || cr == nullptr) {
        double x[NX], e[NX];
        x[0] = p[5] * v; x[1] = -p[7] * v;
        if constexpr (HAS_HH_A) { x[2] = p[1] * v; x[3] = -p[3] * v; }
        bool in = true;
#pragma unroll
        for (int i = 0; i < NX; ++i) in = in && (__builtin_fabs(x[i]) <= 708.0);
        if (__ballot(!in) == 0ull) {
#pragma unroll
          for (int i = 0; i < NX; ++i) e[i] = det_exp_inrange(x[i]);
        } else {
#pragma unroll
          for (int i = 0; i < NX; ++i) e[i] = det_exp_ldexp(x[i]);
        }
        kk[2] = p[4] * e[0]; kk[3] = p[6] * e[1];
        if constexpr (HAS_HH_A) { kk[0] = p[0] * e[2]; kk[1] = p[2] * e[3]; }
        if (cr != nullptr) {
          cr->k[2] = kk[2]; cr->k[3] = kk[3];
          if constexpr (HAS_HH_A) { cr->k[0] = kk[0]; cr->k[1] = kk[1]; }
        }
      } else {
        kk[2] = cr->k[2]; kk[3] = cr->k[3];
        if constexpr (HAS_HH_A) { kk[0] = cr->k[0]; kk[1] = cr->k[1]; }
      }
      k3 = kk[2]; k4 = kk[3];
      if constexpr (HAS_HH_A) dadt = kk[0] * (double)one_m_a - kk[1] * (double)av;
    } else {
      k3 = p[4] * dexp(p[5] * v);
      k4 = p[6] * dexp(-p[7] * v);
      if constexpr (HAS_HH_A) {
        const double k1 = p[0] * dexp(p[1] * v);
        const double k2 = p[2] * dexp(-p[3] * v);
        dadt = k1 * (double)one_m_a - k2 * (double)av;
      }
    }
    const double drdt = -k3 * (double)rv + k4 * (double)one_m_r;
    if constexpr (MT::MLP) dadt = (MODEL == IONODE_MODEL_NND) ? dadt + (double)net : (double)net;
    f[0] = (S)dadt;
    f[1] = (S)drdt;
  }
}

// Closed-form models, split form of rhs(): the rate constants depend on the stage VOLTAGE only, and the last two stages of a
// dopri5 attempt share their time (alpha = 1, 1), so the integrator evaluates them once for both (4 of 24 exp per attempt for
// the 2-state model, 12 of 72 for the 6-state model).  Same expressions as rhs(), same bits.
template <int MODEL, typename S>
__device__ __forceinline__ void closed_rates(const KArgs &a, const double *p, double v, bool inrange, ClosedRates<MODEL> &R) {
  constexpr int NR = ClosedRates<MODEL>::NR;
  R.oob32 = (sizeof(S) == 4) && !inrange;
  if (R.oob32) {
    const float vf = (float)a.v_oob;  // int64 tensor([-80]): `p * v` is float32 and exp runs in fp32
#pragma unroll
    for (int i = 0; i < NR; ++i) R.kf[i] = (float)p[2 * i] * det_expf((float)((i & 1) ? -p[2 * i + 1] : p[2 * i + 1]) * vf);
  } else {
    double x[NR];
    bool inr = true;
#pragma unroll
    for (int i = 0; i < NR; ++i) {
      x[i] = ((i & 1) ? -p[2 * i + 1] : p[2 * i + 1]) * v;
      inr = inr && (__builtin_fabs(x[i]) <= 708.0);
    }
    if (__ballot(!inr) == 0ull) {   // every argument of every lane in range: none of exp's special cases can apply (wave-uniform branch)
#pragma unroll
      for (int i = 0; i < NR; ++i) R.k[i] = p[2 * i] * det_exp_inrange(x[i]);
    } else {
#pragma unroll
      for (int i = 0; i < NR; ++i) R.k[i] = p[2 * i] * det_exp_ldexp(x[i]);
    }
  }
}
template <int MODEL, typename S>
__device__ __forceinline__ void closed_rhs(const ClosedRates<MODEL> &R, const S *y, S *f) {
  if constexpr (MODEL == IONODE_MODEL_MARKOV6) {
    if (R.oob32) {
      const float a1 = R.kf[0], b1 = R.kf[1], bh = R.kf[2], ah = R.kf[3], a2 = R.kf[4], b2 = R.kf[5];
      const float c1 = y[0], c2 = y[1], i_ = y[2], ic1 = y[3], ic2 = y[4], o = y[5];
      f[0] = a1 * c2 + ah * ic1 + b2 * o - (b1 + bh + a2) * c1;
      f[1] = b1 * c1 + ah * ic2 - (a1 + bh) * c2;
      f[2] = a2 * ic1 + bh * o - (b2 + ah) * i_;
      f[3] = a1 * ic2 + bh * c1 + b2 * i_ - (b1 + ah + a2) * ic1;
      f[4] = b1 * ic1 + bh * c2 - (ah + a1) * ic2;
      f[5] = a2 * c1 + ah * i_ - (b2 + bh) * o;
      return;
    }
    const double a1 = R.k[0], b1 = R.k[1], bh = R.k[2], ah = R.k[3], a2 = R.k[4], b2 = R.k[5];
    const double c1 = y[0], c2 = y[1], i_ = y[2], ic1 = y[3], ic2 = y[4], o = y[5];
    f[0] = (S)(a1 * c2 + ah * ic1 + b2 * o - (b1 + bh + a2) * c1);
    f[1] = (S)(b1 * c1 + ah * ic2 - (a1 + bh) * c2);
    f[2] = (S)(a2 * ic1 + bh * o - (b2 + ah) * i_);
    f[3] = (S)(a1 * ic2 + bh * c1 + b2 * i_ - (b1 + ah + a2) * ic1);
    f[4] = (S)(b1 * ic1 + bh * c2 - (ah + a1) * ic2);
    f[5] = (S)(a2 * c1 + ah * i_ - (b2 + bh) * o);
  } else {
    const S av = y[0], rv = y[1];
    if (R.oob32) {
      const float af = (float)av, rf = (float)rv;
      const float drdt = -R.kf[2] * rf + R.kf[3] * (1.0f - rf);
      const float dadt = R.kf[0] * (1.0f - af) - R.kf[1] * af;
      f[0] = (S)dadt;
      f[1] = (S)drdt;
      return;
    }
    const S one_m_a = (S)1 - av, one_m_r = (S)1 - rv;
    const double drdt = -R.k[2] * (double)rv + R.k[3] * (double)one_m_r;
    const double dadt = R.k[0] * (double)one_m_a - R.k[1] * (double)av;
    f[0] = (S)dadt;
    f[1] = (S)drdt;
  }
}

}  // namespace ionode
