// ionode_grad_sweep_body.hpp -- body of the one-phase backward sweep (ionode_grad.hpp), included inside its two kernels:
// ionode_dopri5_backward_kernel (SSE = false: output gradients read from grad_y) and ionode_dopri5_backward_sse_kernel (SSE = true:
// the fused sum-of-squares seed).  It reads the kernel's `a`, MODEL, S, NT and SSE.  Included rather than called, so that the
// grad_y kernels compile to the code they had before the fused variant existed.
// The checkpoint load, the G_c reduction and the stage input stand a second time in ionode_grad_recompute_kernel; the interpolant
// adjoint, the 2-state stage terms, the stage propagation and the adjoint state's load and store in ionode_grad_walk_kernel.  Shared
// routines compiled to other code (DESIGN_HISTORY.md, "The backward sweep's step algebra"), so a correction here is made there too.
  constexpr int D = ModelTraits<MODEL>::D, NPAR = ModelTraits<MODEL>::NPAR;
  static_assert(!SSE || !ModelTraits<MODEL>::MLP, "the fused sum-of-squares sweep is built for the closed-form models");
  constexpr bool M6 = MODEL == IONODE_MODEL_MARKOV6;  // 6-state model (train-d1.py:165-187): f = M(rates(V)) y, closed form
  // HH 2-state (train-s1.py:161-177): the same sweep without the MLP collective -- da/dt = k1 (1 - a) - k2 a is the closed-form
  // a-term of NN-d, so the kernel only skips the vector-Jacobian product and the record stream (NT is 1 and unused)
  constexpr bool HAS_MLP = ModelTraits<MODEL>::MLP;
  constexpr bool NND = MODEL == IONODE_MODEL_NND || MODEL == IONODE_MODEL_HH2;  // closed-form a-gate terms
  using R = Real<S>;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int j = lane & 15;
  const int traj_raw = blockIdx.x * 16 + j;
  const bool valid = traj_raw < a.k.B;
  const int traj = valid ? traj_raw : a.k.B - 1;
  const bool writer = valid && wave == 0 && lane < 16;

  GradMlp<NT> mlp;
  double *__restrict__ Gs = reinterpret_cast<double *>(smem);  // [16][5 * D] fp64 scratch
  if constexpr (HAS_MLP) {
    mlp.init(a, smem, wave, lane);
    Gs = mlp.gs();
  }

  double p[NPAR];
#pragma unroll
  for (int i = 0; i < NPAR; ++i) p[i] = a.k.params[(size_t)traj * a.k.n_params + i];
  const int pidx = a.k.prot_of_traj ? a.k.prot_of_traj[traj] : (traj % a.k.P);
  const double *__restrict__ pv = a.k.prot_v + (size_t)pidx * a.k.Np;
  const int nst = valid ? a.nacc[traj] : 0;
  using CK = CkptRecord<D>;
  constexpr int RECW = CK::WIDTH, RECY = CK::Y;
  const double *__restrict__ ck = a.ckpt + (size_t)traj * a.ckpt_cap * RECW;
  const S *__restrict__ gy = SSE ? nullptr : reinterpret_cast<const S *>(a.grad_y) + (size_t)traj * a.k.Nt * D;
  const int Nt = a.k.Nt;

  constexpr int STATE = 2 * D + NPAR;  // adjoint state carried between chunk launches
  double lam[D], mu[D], gp[NPAR];
  {
    const double *st = a.state + (size_t)traj * STATE;
#pragma unroll
    for (int d = 0; d < D; ++d) { lam[d] = a.it_begin > 0 ? st[d] : 0.0; mu[d] = a.it_begin > 0 ? st[D + d] : 0.0; }
#pragma unroll
    for (int i = 0; i < NPAR; ++i) gp[i] = a.it_begin > 0 ? st[2 * D + i] : 0.0;
  }

  for (int it = a.it_begin; it < a.it_end; ++it) {
    const int s = nst - 1 - it;
    const bool step = s >= 0;
    const bool initev = (s == -1) && nst > 0;  // k1 of the first step: f(t[0], y0)
    // ---- checkpoint of my step (init evaluation: the first step's start state is y0) ----
    double t0 = 0.0, dt = 1.0, y[D], k[7][D];
    int oi = 0, nout = 0;
    {
      const double *rec = ck + (size_t)(step ? s : 0) * RECW;
      const bool ld = step || initev;
      if (ld) { t0 = rec[CK::T0]; dt = rec[CK::DT]; }
      if (step) { oi = (int)rec[CK::OI]; nout = (int)rec[CK::NOUT]; }
#pragma unroll
      for (int d = 0; d < D; ++d) y[d] = ld ? rec[CK::Y + d] : 0.0;
#pragma unroll
      for (int jx = 0; jx < 7; ++jx)
#pragma unroll
        for (int d = 0; d < D; ++d) k[jx][d] = step ? rec[CK::K + jx * D + d] : 0.0;
    }
    const double t1 = t0 + dt;
    const S t0s = (S)t0, dts_s = (S)dt, t1s = (S)t1;
    const double dts = (double)dts_s;

    // fused objective: my step's dense-output coefficients (e, d, c, b, a), fitted as the forward fitted them (sse_fit_step).  y1 is the
    // next accepted step's checkpointed start state; the last step recomputes it as the forward did.
    S cf[SSE ? 5 : 1][SSE ? D : 1];
    if constexpr (SSE) sse_fit_step<S, D>(dt, y, k, (step && s + 1 < nst) ? ck + (size_t)(s + 1) * RECW + RECY : nullptr, cf);

    // ---- adjoints of the interpolant coefficients: G_c = sum_k gy[k] * x_k^c over the step's output samples ----
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int jj = wave + 4 * u;  // this wavefront reduces trajectory slots wave, wave+4, ...
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
        if constexpr (SSE) {
          S cb[5][D];
#pragma unroll
          for (int c = 0; c < 5; ++c)
#pragma unroll
            for (int d = 0; d < D; ++d) cb[c][d] = bcast<S>(cf[c][d], jj);
          const int pj = __builtin_amdgcn_readlane(pidx, jj);
          const double *__restrict__ pvb = a.k.prot_v + (size_t)pj * a.k.Np;
          const double *__restrict__ refb = a.sse_ref + (size_t)pj * Nt;
          const double *__restrict__ vtb = a.v_tab ? a.v_tab + (size_t)pj * Nt : nullptr;
          const double gb = a.grad_sse[tr];
          const double den = t1b - t0b, rden = 1.0 / den;   // the forward's reciprocal and div_pos: the same x bits
          sse_step_samples(a.k.obj_abs, [&](auto kind) {
            for (int c0 = 0; c0 < n; c0 += 64) {
              if (c0 + lane < n) {
                const int idx = o + c0 + lane;
                const double tk = a.k.t_eval[idx];
                double vk;
                if (vtb) vk = vtb[idx];
                else protocol_v(a.k, pvb, tk, vk);
                sse_sample_term<S, D, decltype(kind)::value>(a, cb, interp_x<S>(tk, t0b, den, rden), vk, refb[idx], gb, P);
              }
            }
          });
        } else {
        const S *__restrict__ gyb = reinterpret_cast<const S *>(a.grad_y) + (size_t)tr * Nt * D;
        for (int c0 = 0; c0 < n; c0 += 64) {
          if (c0 + lane < n) {
            const int idx = o + c0 + lane;
            const double tk = a.k.t_eval[idx];
            const double x = (double)(S)((tk - t0b) / (t1b - t0b));
            double xp = 1.0;
#pragma unroll
            for (int c = 0; c < 5; ++c) {
#pragma unroll
              for (int d = 0; d < D; ++d) P[c][d] += (double)gyb[(size_t)idx * D + d] * xp;
              xp *= x;
            }
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
    __syncthreads();
    double Gc[5][D];
#pragma unroll
    for (int c = 0; c < 5; ++c)
#pragma unroll
      for (int d = 0; d < D; ++d) Gc[c][d] = Gs[j * (5 * D) + c * D + d];

    // ---- interpolant adjoint -> (Y0, Y1, k1..k7); FSAL carry (tests/grad_check.py manual_adjoint) ----
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

    float *__restrict__ rec_it = a.records
        ? a.records + ((size_t)blockIdx.x * (a.it_end - a.it_begin) + (it - a.it_begin)) * 6 * a.record_floats : nullptr;

    // ---- stages 6..1 (k[i+1] = f(t_i, Y_i)), one collective MLP vector-Jacobian product each ----
    auto stage = [&](const int e) {
      const int i = 5 - e;
      double Yi[D], seed[D];
      double tq;
      if (step) {
#pragma unroll
        for (int d = 0; d < D; ++d) {
          double sacc = 0.0;
          for (int jx = 0; jx <= i; ++jx) sacc += k[jx][d] * (kBeta[i][jx] * dts);
          Yi[d] = y[d] + sacc;
          seed[d] = ak[i + 1][d];
        }
        const S ti = (i >= 4) ? R::prev_(t1s) : t0s + (S)kAlpha[i] * dts_s;
        tq = (double)ti;
      } else {
#pragma unroll
        for (int d = 0; d < D; ++d) { Yi[d] = y[d]; seed[d] = (initev && e == 0) ? mu[d] : 0.0; }
        tq = (double)(S)a.k.t_eval[0];
      }
      double v;
      protocol_v(a.k, pv, tq, v);
      // Note (fp32 state, stage time OUTSIDE the protocol): the forward then follows torch's int64 -80 promotion and evaluates the
      // rate terms in fp32 (`p * v` and exp in float32: ionode_device.hpp rhs(), train-s1.py:236-241); the sweep below always
      // linearises the fp64 formulas at v = v_oob.  Forward value and linearised function differ there by fp32 rounding of the
      // rates (relative 1e-7) -- two orders below the agreement the checker asserts (GRAD_REL_TOL 1e-4), and only on stages whose
      // time lies beyond the protocol's last sample (the overshooting last step).  The checker (tests/grad_check.py) makes the same
      // choice, so it is a property of the gradient's definition, not a kernel-vs-checker difference.
      double w[D];
      if constexpr (M6) {
        // f = M(rates) y (train-d1.py:165-187): w = M^T seed; rate_i = p[2i] exp(+-p[2i+1] V), g_i = seed . df/drate_i
        double ex[6], r[6];
#pragma unroll
        for (int q = 0; q < 6; ++q) { ex[q] = det_exp(((q & 1) ? -p[2 * q + 1] : p[2 * q + 1]) * v); r[q] = p[2 * q] * ex[q]; }
        const double a1 = r[0], b1 = r[1], bh = r[2], ah = r[3], a2 = r[4], b2 = r[5];
        const double c1 = Yi[0], c2 = Yi[1], in = Yi[2], ic1 = Yi[3], ic2 = Yi[4], o = Yi[5];
        const double s0 = seed[0], s1 = seed[1], s2 = seed[2], s3 = seed[3], s4 = seed[4], s5 = seed[5];
        w[0] = -(b1 + bh + a2) * s0 + b1 * s1 + bh * s3 + a2 * s5;
        w[1] = a1 * s0 - (a1 + bh) * s1 + bh * s4;
        w[2] = -(b2 + ah) * s2 + b2 * s3 + ah * s5;
        w[3] = ah * s0 + a2 * s2 - (b1 + ah + a2) * s3 + b1 * s4;
        w[4] = ah * s1 + a1 * s3 - (ah + a1) * s4;
        w[5] = b2 * s0 + bh * s2 - (b2 + bh) * s5;
        double g[6];
        g[0] = (s0 - s1) * c2 + (s3 - s4) * ic2;                                    // a1
        g[1] = (s1 - s0) * c1 + (s4 - s3) * ic1;                                    // b1
        g[2] = (s3 - s0) * c1 + (s4 - s1) * c2 + (s2 - s5) * o;                     // bh
        g[3] = (s0 - s3) * ic1 + (s1 - s4) * ic2 + (s5 - s2) * in;                  // ah
        g[4] = (s5 - s0) * c1 + (s2 - s3) * ic1;                                    // a2
        g[5] = (s0 - s5) * o + (s3 - s2) * in;                                      // b2
#pragma unroll
        for (int q = 0; q < 6; ++q) {
          gp[2 * q] += g[q] * ex[q];
          gp[2 * q + 1] += g[q] * r[q] * ((q & 1) ? -v : v);
        }
      } else {
      const double av = Yi[0], rv = Yi[1];
      const float x0 = (float)(v / 100.0), x1 = (float)av;
      const float seedf = (float)(seed[0] / 1000.0);
      float dx1 = 0.0f;
      if constexpr (HAS_MLP) {
        float *__restrict__ rec_e = rec_it ? rec_it + (size_t)e * a.record_floats : nullptr;
        dx1 = mlp.vjp(x0, x1, seedf, rec_e);
      }
      // closed-form terms of the RHS and their parameter gradients
      const double e3 = det_exp(p[5] * v), e4 = det_exp(-p[7] * v);
      const double k3 = p[4] * e3, k4 = p[6] * e4;
      w[0] = (double)dx1;
      w[1] = -seed[1] * (k3 + k4);
      gp[4] += seed[1] * (-e3 * rv);
      gp[5] += seed[1] * (-k3 * v * rv);
      gp[6] += seed[1] * (e4 * (1.0 - rv));
      gp[7] += seed[1] * (-k4 * v * (1.0 - rv));
      if constexpr (NND) {
        const double e1 = det_exp(p[1] * v), e2 = det_exp(-p[3] * v);
        const double k1 = p[0] * e1, k2 = p[2] * e2;
        w[0] += -seed[0] * (k1 + k2);
        gp[0] += seed[0] * (e1 * (1.0 - av));
        gp[1] += seed[0] * (k1 * v * (1.0 - av));
        gp[2] += seed[0] * (-e2 * av);
        gp[3] += seed[0] * (k2 * v * av);
      }
      }
      if (step) {
#pragma unroll
        for (int d = 0; d < D; ++d) {
          const double wd = (i == 5) ? w[d] + aY1[d] : w[d];
          aY0[d] += wd;
          for (int jx = 0; jx <= i; ++jx) ak[jx][d] += (kBeta[i][jx] * dts) * wd;
        }
      } else if (initev && e == 0) {
#pragma unroll
        for (int d = 0; d < D; ++d) lam[d] += w[d];
      }
    };
    if constexpr (HAS_MLP) {
#pragma unroll 1
      for (int e = 0; e < 6; ++e) stage(e);   // one instance of the MLP collective in the code
    } else {
#pragma unroll
      for (int e = 0; e < 6; ++e) stage(e);   // closed form: unrolled, so that k[jx][d] / ak[jx][d] are register-indexed
    }
    if (step) {
#pragma unroll
      for (int d = 0; d < D; ++d) { lam[d] = aY0[d]; mu[d] = ak[0][d]; }
    }
    if constexpr (!HAS_MLP) __syncthreads();  // the next iteration rewrites Gs (the MLP variants pass barriers inside vjp)
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
      if constexpr (SSE) {
        // sample 0 of the objective is y0 itself (ionode_device.hpp: the forward's initial residual); the first checkpoint holds y0
        double s0[D];
#pragma unroll
        for (int d = 0; d < D; ++d) s0[d] = 0.0;
        if (nst > 0) {
          S y0s[D];
#pragma unroll
          for (int d = 0; d < D; ++d) y0s[d] = (S)ck[RECY + d];
          double v0;
          if (a.v_tab) v0 = a.v_tab[(size_t)pidx * Nt];
          else protocol_v(a.k, pv, a.k.t_eval[0], v0);
          double dr[D];
          const double gr = residual_weight(sse_residual<S, D>(a, y0s, v0, a.sse_ref[(size_t)pidx * Nt], dr), a.grad_sse[traj], a.k.obj_abs);
#pragma unroll
          for (int d = 0; d < D; ++d) s0[d] = gr * dr[d];
        }
#pragma unroll
        for (int d = 0; d < D; ++d) a.grad_y0[(size_t)traj * D + d] = lam[d] + s0[d];
      } else {
#pragma unroll
        for (int d = 0; d < D; ++d) a.grad_y0[(size_t)traj * D + d] = lam[d] + (double)gy[d];  // solution[0] = y0
      }
    }
  }
