// ionode_attempt_body.hpp -- ONE ATTEMPT of ionode_dopri5_kernel (ionode_device.hpp), the body of its attempt loop(s): assertions, the
// Runge-Kutta step on the net IONODE_NET, error control, dense output, state advance.  `break` leaves the enclosing loop when no
// trajectory of the tile is live.  Included inside the kernel only: it reads and writes the kernel's locals.  Round 6: the lean N = 200
// 16-tile runs it in two loops, on its own net and then on MlpShrink4; every other kernel in one, as before.
#ifdef IONODE_STAMPS
    constexpr int NET = std::is_same<typename std::decay<decltype(IONODE_NET)>::type, MlpShrink4>::value ? 1 : 0;
    const unsigned long long att0_ = stamp_now();
#endif
    if constexpr (LW) {
      // Lane-wise kernels run at a fixed register budget (2-state: 168 for three wavefronts per SIMD).  Everything DERIVED from the
      // per-lane parameters that is invariant over the attempts -- fp32 copies and out-of-range rate constants for the fp32-state
      // rule, negated exponents, protocol row addresses -- would be hoisted out of this loop and stay live through it: ~20 VGPRs for
      // values the hot path never reads.  An empty asm makes the parameters opaque once per attempt: no instruction, no hoisting.
#pragma unroll
      for (int i = 0; i < NPAR; ++i) asm volatile("" : "+v"(p[i]));
    }
    // ---- per-trajectory assertions of _adaptive_step / _advance ----
    bool failed_now = false;
    if (active) {
      if ((int64_t)since >= a.max_steps || (int64_t)nacc + nrej >= a.max_total) { status = IONODE_STATUS_MAX_STEPS; failed_now = true; }
      else if (!(t + dt > t)) { status = IONODE_STATUS_DT_UNDERFLOW; failed_now = true; }
      else {
        bool fin = true;
#pragma unroll
        for (int d = 0; d < D; ++d) fin = fin && isfinite((double)y[d]);
        if (!fin) { status = IONODE_STATUS_NONFINITE; failed_now = true; }
      }
      if (failed_now) active = false;
    }
    // failed trajectories: the rest of their output is NaN (cooperative fill)
    {
      unsigned long long fm = __ballot(failed_now && lane < LPS);
      while (fm) {
        const int jj = __builtin_ctzll(fm);
        fm &= fm - 1;
        if (WPS == 1 || (jj % WPS) == wis) {
          const int o0 = __builtin_amdgcn_readlane(oi, jj);
          const int tr = __builtin_amdgcn_readlane(traj, jj);
          S *__restrict__ yo = reinterpret_cast<S *>(a.y_out) + (size_t)tr * Nt * D;
          for (int idx = o0 + lane; idx < Nt && (a.y_out || a.i_out); idx += 64) {
            if (a.y_out) {
#pragma unroll
              for (int d = 0; d < D; ++d) yo[(size_t)idx * D + d] = nan_s;
            }
            if (a.i_out) a.i_out[(size_t)tr * Nt + idx] = __builtin_nan("");
          }
        }
      }
    }
    if constexpr (NSETS > 1) {
      // two column sets: the wavefronts of one set may be done while the other set still integrates -- but every stage evaluation is a
      // collective of all G wavefronts (each computes its row tiles for BOTH sets), so the tile leaves the loop together
      if (__syncthreads_or(active ? 1 : 0) == 0) break;
    } else {
      if (__ballot(active) == 0ull) break;
    }

    // ---- _runge_kutta_step ----
    const double t0 = t;
    const double t1 = t0 + dt;
    const S dts = (S)dt;
    S k[7][D], yi[D];
#pragma unroll
    for (int d = 0; d < D; ++d) k[0][d] = f[d];
    // stage voltages: pure functions of (t0, dt), so all protocol loads are issued ahead of the stages
    if constexpr (!CARRY_V) lookup_stages(t0, dt);
    STAMP(stamps_, 1);  // slot 1 (asm tile: layer 0 is inside the stream): attempt prologue = stage-voltage lookups
    ClosedRates<MT::MLP ? IONODE_MODEL_HH2 : MODEL> cr;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      S bd[6];
#pragma unroll
      for (int jx = 0; jx <= i; ++jx) bd[jx] = (S)kBeta[i][jx] * dts;
#pragma unroll
      for (int d = 0; d < D; ++d) {
        S s = k[0][d] * bd[0];
#pragma unroll
        for (int jx = 1; jx <= i; ++jx) s = s + k[jx][d] * bd[jx];
        yi[d] = y[d] + s;
      }
      if constexpr (MT::MLP && T64) {
        // the lane-wise nets: the rate constants of the Hodgkin-Huxley terms are reused as in the closed-form kernels below
        bool fresh = (i == 0);
        if (i > 0 && i < 5) fresh = __ballot(vst[i] != vst[i > 0 ? i - 1 : 0] || inst[i] != inst[i > 0 ? i - 1 : 0]) != 0ull;
        rhs<MODEL, S, T64>(a, p, vst[i < 4 ? i : 4], inst[i < 4 ? i : 4], yi, k[i + 1], IONODE_NET, &cr, fresh);
      } else if constexpr (MT::MLP) rhs<MODEL, S, T64>(a, p, vst[i < 4 ? i : 4], inst[i < 4 ? i : 4], yi, k[i + 1], IONODE_NET);
      else {
        // rate constants depend on the stage VOLTAGE only: i == 5 shares its stage time with i == 4, and on the holding / step
        // segments of the reference's protocols (Pr3, Pr5, staircase plateaus: train-s1.py:69-95) consecutive stages see the very same
        // voltage -- when every lane of the wavefront does, the previous stage's rates are reused (same inputs, same bits):
        // 4 instead of 20 exp per attempt of the 2-state model on a plateau, 12 instead of 60 for the 6-state model
        if (i < 5) {
          bool fresh = (i == 0);
          if (i > 0) fresh = __ballot(vst[i] != vst[i > 0 ? i - 1 : 0] || inst[i] != inst[i > 0 ? i - 1 : 0]) != 0ull;
          if (fresh) closed_rates<MODEL, S>(a, p, vst[i], inst[i], cr);
        }
        closed_rhs<MODEL, S>(cr, yi, k[i + 1]);
      }
    }
    // y1 = y_5 (c_sol == beta[5] + [0]); error estimate; _compute_error_ratio
    S tmp[D];
    {
      S be[7];
#pragma unroll
      for (int jx = 0; jx < 7; ++jx) be[jx] = dts * (S)kCerr[jx];
#pragma unroll
      for (int d = 0; d < D; ++d) {
        S e = k[0][d] * be[0];
#pragma unroll
        for (int jx = 1; jx < 7; ++jx) e = e + k[jx][d] * be[jx];
        const S ay0 = abs_(y[d]), ay1 = abs_(yi[d]);
        const S tol = atol + rtol * (ay0 > ay1 ? ay0 : ay1);
        tmp[d] = e / tol;
      }
    }
    const S ratio = abs_(rms_norm<S, D>(tmp));
    const bool accept = ratio <= (S)1;

    // _optimal_step_size (fp64)
    double dt_next;
    if (ratio == (S)0) dt_next = dt * 10.0;
    else {
      const double dfactor = (ratio < (S)1) ? 1.0 : 0.2;
      const double er = (double)ratio;
      double fac = 0.9 / det_root5(er);
      if (!(fac > dfactor)) fac = dfactor;
      if (!(fac < 10.0)) fac = 10.0;
      if (er != er) fac = __builtin_nan("");
      dt_next = dt * fac;
    }

    STAMP(stamps_, 6);  // slot 6: stage assembly + error control (scalar RK work outside the MLP)
    const bool acc_now = active && accept;
#ifndef IONODE_STAMPS
    if (a.step_log != nullptr && active && primary && traj_raw == 0 && (int64_t)nacc + nrej < a.step_log_cap) {
      double *row = a.step_log + 4 * ((int64_t)nacc + nrej);
      row[0] = t0; row[1] = dt; row[2] = (double)ratio; row[3] = accept ? 1.0 : 0.0;
    }
#endif
    const int nacc_before = nacc, oi_before = oi;
    if (active) { if (accept) ++nacc; else ++nrej; }
    const double dt_capped = (dt_next > a.dt_max) ? a.dt_max : dt_next;  // NaN stays NaN (-> 'underflow in dt')
    if constexpr (CARRY_V) lookup_stages(acc_now ? t1 : t0, (active || acc_now) ? dt_capped : dt);

    // ---- _interp_fit + cooperative dense output ----
    // x = (t_k - t0) / (t1 - t0) of every dense-output sample: ONE division per attempt (the reciprocal of the step length),
    // then div_by() per sample -- the same correctly rounded quotient
    const double den = t1 - t0;
    const double rden = 1.0 / den;
    using IRow = InterpRow<D>;      // an LDS row of the lane-wise kernels (16-byte aligned)
    S ic[LW ? 1 : 5][LW ? 1 : D];   // e, d, c, b, a -- tile kernels keep them in registers (broadcast by v_readlane)
    {
      // (the weights and the per-component call are written in this shape on purpose: through a routine for the weights, or without
      // the lambda, hipcc schedules the 6-state kernels differently -- fused objective forward +3.7 %, profiles/interp_refactor.md)
      S bm[7];
#pragma unroll
      for (int jx = 0; jx < 7; ++jx) bm[jx] = dts * (S)kCmid[jx];
      auto fit = [&](int d, S *c5) { interp_fit<S, D>(dts, bm, y, yi, k, d, c5); };
      if constexpr (LW) {
        // Lane-wise kernels: a lane's interpolant (t0, step length, its reciprocal, 5 x D coefficients) goes to its LDS row;
        // the wavefront then reads the emitting trajectory's row at a uniform address (7 broadcast ds_read_b128 for D = 2)
        // instead of ~29 v_readlane per emitting trajectory.  The workgroup is one wavefront: LDS is in order, no barrier.
        // The coefficients are fitted and stored two components at a time, so that at most 10 of the 5 x D are live
        // (6-state model: 60 registers fewer at the kernel's pressure peak).
        double2 *row = reinterpret_cast<double2 *>(lsm + lane * ROWB);
        row[0] = make_double2(t0, den);
        row[1] = make_double2(rden, 0.0);
#pragma unroll
        for (int d = 0; d < D; d += 2) {
          S ca[5], cb2[5];
          fit(d, ca);
          fit(d + 1, cb2);
#pragma unroll
          for (int c = 0; c < 5; ++c) row[IRow::coef(c, d) / 2] = make_double2((double)ca[c], (double)cb2[c]);
          if constexpr (D > 2) __builtin_amdgcn_sched_barrier(0);
        }
      } else {
#pragma unroll
        for (int d = 0; d < D; ++d) {
          S c5[5];
          fit(d, c5);
#pragma unroll
          for (int c = 0; c < 5; ++c) ic[c][d] = c5[c];
        }
      }
    }
    // the interpolant of emitting trajectory jj, wave-uniform: from its LDS row, or from its lane's registers
    auto load_interp = [&](Interp<S, D> &itp, int jj) {
      if constexpr (LW) itp.from_row(reinterpret_cast<const double2 *>(lsm + jj * ROWB));
      else itp.from_lanes(t0, den, rden, ic, jj);
    };
    STAMP(stamps_, 8);  // slot 8: interpolant fit
    if (LEAN || LEANM || a.te_dt > 0.0) {
      // ---- output cursor, lane-parallel: how many requested times fall in (t0, t1] for MY trajectory? ----
      // Guess the last index from the (nearly) uniform output grid, then VERIFY against t_eval itself and walk to the
      // exact answer: correct for any increasing t_eval, one L2 round trip for the whole tile when the guess is right
      // (instead of one dependent load per trajectory in the cooperative scan below).
      int n_out = 0;
      if (acc_now) {
        const double gf = floor((t1 - a.te_t0) * a.te_rdt);  // a guess: verified below
        long long g = (gf < (double)(oi - 1)) ? (long long)(oi - 1) : ((gf > (double)(Nt - 1)) ? (long long)(Nt - 1) : (long long)gf);
        // lean lane-wise kernels: the 6-state one verifies its cursor against arithmetic times too (262 144 x 20 001: 76.1 -> 72.1 ms);
        // the 2-state ones keep the load -- the two scalars cost them 24 spilled SGPRs (393 216: 31.1 -> 38.0 ms)
        if ((LW && LEAN && D > 2) || (!LW && a.te_exact)) {  // verified uniform output grid: t_k is formed arithmetically, no load
          while (g >= oi && te_at((int)g) > t1) --g;
          while (g + 1 < Nt && te_at((int)g + 1) <= t1) ++g;
        } else {
          while (g >= oi && a.t_eval[g] > t1) --g;
          while (g + 1 < Nt && a.t_eval[g + 1] <= t1) ++g;
        }
        n_out = (int)(g - oi + 1);
      }
      STAMP(stamps_, 9);  // slot 9: output cursor
      if constexpr (!LW && G > 1) {
      // ---- MLP tile kernels: the owner wavefront emits its NS = TPW / G trajectories.  Everything that has to come from
      // memory for the first 64-sample chunk of ALL of them -- output times (unless the grid is verified uniform: arithmetic),
      // the two protocol samples per output time of the observation model -- is issued before anything is evaluated: one
      // round trip per accepted step instead of two dependent ones per emitting trajectory.  Samples beyond the first chunk
      // (steps spanning more than 64 outputs) take the plain loop.
      constexpr int NS = (LPS >= WPS) ? LPS / WPS : 1;   // (one trajectory per tile: wavefront 0 emits it, the others nothing)
      const bool exact = a.te_exact != 0;
      const bool want_i = (a.i_out != nullptr) || (a.sse_out != nullptr);
      const bool ugrid = a.prot_t == nullptr;
      // ---- deferred dense output (KernelForm::defer, a record workspace given): the step leaves ONE record to ionode_dense_expand_kernel
      // instead of evaluating its samples here.  Lanes 16 q + j of all four wavefronts hold slot j's values: replica 4 wis + q stores
      // 16-byte chunk 4 wis + q of the row -- one store instruction per wavefront.  A trajectory whose records are full emits inline.
      int n_emit = n_out;
      if constexpr (F::defer) {
        if (a.defer_rec != nullptr) {
          using Rec = DenseRecord<D>;
          const bool rec_now = n_out > 0 && nrec < a.defer_fill;
          const int rq = lane >> 4;
          auto chunk = [&](int r) {   // (r: a constant once unrolled)
            if (r == 0) return make_double2(t0, den);
            if (r == 1) return make_double2(rden, Rec::pack_cursor(oi_before, n_out));
            const int e = 2 * (r - 2);   // coefficient pair e, e + 1 of [c][d]
            return make_double2((double)ic[e / D][e % D], (double)ic[(e + 1) / D][(e + 1) % D]);
          };
          double2 *__restrict__ row = reinterpret_cast<double2 *>(a.defer_rec + ((size_t)traj * (size_t)a.defer_cap + (size_t)nrec) * Rec::ROW);
#pragma unroll
          for (int w = 0; 4 * w < Rec::CHUNKS; ++w) {
            if (wis == w) {
              double2 v = chunk(4 * w);
#pragma unroll
              for (int qq = 1; qq < 4; ++qq) {
                if (4 * w + qq < Rec::CHUNKS) {
                  const double2 c = chunk(4 * w + qq);
                  if (rq == qq) v = c;
                }
              }
              if (rec_now && 4 * w + rq < Rec::CHUNKS) row[4 * w + rq] = v;
            }
          }
          if (rec_now) { n_emit = 0; ++nrec; }
        }
      }
      if (!F::defer || __ballot(n_emit > 0) != 0ull) {
      int o_[NS], n_[NS], ip_[NS];
      double tk_[NS], plo_[NS], phi_[NS];
      bool inr_[NS];
      const double *pv_[NS];
#pragma unroll
      for (int k = 0; k < NS; ++k) {
        const int jj = wis + WPS * k;
        o_[k] = __builtin_amdgcn_readlane(oi, jj);
        n_[k] = (LPS >= WPS || jj < LPS) ? __builtin_amdgcn_readlane(n_emit, jj) : 0;
        pv_[k] = a.prot_v + (size_t)__builtin_amdgcn_readlane(pidx, jj) * a.Np;
        tk_[k] = 0.0;
        if (lane < n_[k]) tk_[k] = exact ? te_at(o_[k] + lane) : a.t_eval[o_[k] + lane];
      }
      if (want_i && ugrid) {
#pragma unroll
        for (int k = 0; k < NS; ++k) {
          inr_[k] = protocol_index(a, tk_[k], ip_[k]);  // (idle lanes: t = 0, a valid index; their loads are harmless)
          plo_[k] = pv_[k][ip_[k] - 1]; phi_[k] = pv_[k][ip_[k]];
        }
      }
      STAMP(stamps_, 10);  // slot 10: emission, gather phase
#pragma unroll
      for (int k = 0; k < NS; ++k) {
        const int jj = wis + WPS * k;
        const int n = n_[k], o = o_[k];
        if (n > 0) {
          Interp<S, D> itp;
          load_interp(itp, jj);
          const int tr = __builtin_amdgcn_readlane(traj, jj);
          S *__restrict__ yo = a.y_out ? reinterpret_cast<S *>(a.y_out) + (size_t)tr * Nt * D : nullptr;
          double *__restrict__ io = a.i_out ? a.i_out + (size_t)tr * Nt : nullptr;
          const double *__restrict__ refb = a.sse_out ? a.sse_ref + (size_t)__builtin_amdgcn_readlane(pidx, jj) * Nt : nullptr;
          double sacc = 0.0;
          for (int c0 = 0; c0 < n; c0 += 64) {
            const int idx = o + c0 + lane;
            double tk = tk_[k];
            if (c0 > 0 && c0 + lane < n) tk = exact ? te_at(idx) : a.t_eval[idx];
            if (c0 + lane < n) {
              S out[D];
              interp_eval<S, D>(itp.cb, itp.x(tk), out);
              if (yo) store_state<S, D>(yo + (size_t)idx * D, out);
              if (want_i) {
                double vk;
                if (c0 == 0 && ugrid) vk = inr_[k] ? protocol_from(a, plo_[k], phi_[k], ip_[k], tk) : a.v_oob;
                else protocol_v(a, pv_[k], tk, vk);
                const double ik = obs_current<S, D>(a, out, vk);
                if (io) io[idx] = ik;
                if (refb) { const double rr = ik - refb[idx]; sacc += residual_term(rr, F::objective_kinds ? a.obj_abs : 0); }
              }
            }
          }
          if (a.sse_out) {  // fused objective: the step's squared residuals of trajectory jj
#pragma unroll
            for (int msk = 32; msk >= 1; msk >>= 1) sacc += __shfl_xor(sacc, msk);
            if (j == jj) sse += sacc;
          }
        }
      }
      }   // (deferring tile: no trajectory of the tile emits inline this attempt)
      oi += n_out;
      } else {
      // ---- lane-wise kernels on a verified uniform output grid: WORK-LIST emission.
      // Steps differ wildly in the number of output samples they cover (2-state, sine-wave legs: 10 % of the accepted steps cover
      // <= 5 samples, the median 39, 10 % >= 170; 6-state: ~20 on average).  Round 3 handed each group of 8 lanes one emitting
      // trajectory at a time and ran a pass until the longest of its 8 trajectories was done: 78 iterations per attempt where 36 would
      // do (a CPU replay of the step logs of one wavefront, tools/emit_replay.py), and the dense output was 72 % of the kernel.  Every emitting lane
      // appends its step's 8-sample chunks {lane, 8 * chunk number} to the LDS work list; a pass takes the next 8 entries, one per
      // group of 8 lanes; what used to be wave-uniform per trajectory (interpolant row, cursor, protocol, trajectory index) is read
      // per lane from LDS: the owner's row, whose spare slot carries (oi, n_out), the protocol index parked in `owp`, the
      // trajectory index in `trl`.  Same samples, same arithmetic; the fused objective keeps its summation order (a chunk = the same
      // 8 consecutive samples as before, partial sum number = chunk number -- which is why steps of more than 64 samples take the
      // one-trajectory-per-pass loop below); V(t_k) and the reference current of the NEXT pass are loaded before this pass's stores.
      bool packed_lane = false;   // my trajectory's samples are emitted by the work-list passes (the others: the loop below)
      if constexpr (LW && (VTAB || D > 2 || (CF2 && F::lean == Lean::States))) {
        // a chunk of PK = 8 samples is served by PKL lanes x NSL samples each (lane kk: samples kk, kk + PKL, ...): one row read per
        // NSL samples -- with one sample per lane the LDS pipe, not the vector ALU, bounded these passes (the 6-state row is 272 bytes)
        constexpr int PK = 8, PKL = (D == 2) ? 4 : 2, NSL = PK / PKL;
        typedef S SV __attribute__((ext_vector_type(NSL)));
        const bool want_i = (a.i_out != nullptr) || (a.sse_out != nullptr);
        // one instance per compiled variant: the table variant serves the current / objective epilogue, the plain one
        // states only (its epilogue without the table -- a protocol lookup per sample -- stays on the loop below)
        // (2-state kernels that also store the states keep the loop below: at ~34 samples per step its 64 consecutive samples per
        // store instruction touch half the cache lines of 8 x 8, and that path is store-bound: 41.5 against 44.7 ms packed)
        if (a.te_exact && (VTAB ? (want_i && (D > 2 || a.y_out == nullptr)) : (!want_i && a.y_out != nullptr))) {
          int lane_e = lane;   // opaque per-attempt copy: what is derived from it (row / list addresses, group and sample numbers) is computed here, per
                               // attempt, instead of being hoisted out of the attempt loop into a dozen VGPRs that stay live through the stage loop
          asm volatile("" : "+v"(lane_e));
          packed_lane = n_out > 0 && lane_e < LPS && n_out <= 64;
          const unsigned long long emd = __ballot(packed_lane);
          auto emit_packed = [&](auto wi_tag) {
            constexpr bool WI = decltype(wi_tag)::value;
            const int nch = (n_out + PK - 1) / PK;   // 1 .. 8 for the listed lanes
            if (packed_lane) *reinterpret_cast<int2 *>(lsm + lane_e * ROWB + IRow::SPARE * 8) = make_int2(oi, oi + n_out);   // the row's spare slot
            const int x = nch - 1;
            const unsigned long long m0 = __ballot(packed_lane && (x & 1)), m1 = __ballot(packed_lane && (x & 2)), m2 = __ballot(packed_lane && (x & 4));
            const int q = mbcnt(m0, mbcnt(emd)) + 2 * mbcnt(m1) + 4 * mbcnt(m2);
            const int C = __builtin_popcountll(emd) + __builtin_popcountll(m0) + 2 * __builtin_popcountll(m1) + 4 * __builtin_popcountll(m2);
#pragma unroll
            for (int i = 0; i < 8; ++i)
              if (packed_lane && i < nch) clist[q + i] = (unsigned short)(lane_e | (i * PK) << 6);
            const int slot = lane_e / PKL, kk = lane_e % PKL;
            // decode of a list entry: trajectory lane, first sample of the lane, and (table variant) the loads of V(t_k) / reference
            struct Ent { int jj, idx0, end, part; bool has; double vk[NSL], rf[NSL]; };
            auto decode = [&](int c0) {
              Ent t;
              t.has = c0 + slot < C;
              const unsigned e = clist[t.has ? c0 + slot : (c0 < C ? c0 : 0)];
              t.jj = (int)(e & 63u);
              t.part = (int)(e >> 9);   // chunk number: the objective's partial-sum slot
              const int2 on2 = *reinterpret_cast<const int2 *>(lsm + t.jj * ROWB + IRow::SPARE * 8);
              t.idx0 = on2.x + (int)(e >> 6) + kk;
              t.end = on2.y;
#pragma unroll
              for (int u = 0; u < NSL; ++u) { t.vk[u] = 0.0; t.rf[u] = 0.0; }
              if constexpr (VTAB && WI) {
                const int pj = owp[t.jj];
#pragma unroll
                for (int u = 0; u < NSL; ++u) {
                  const int idx = t.idx0 + u * PKL;
                  if (t.has && idx < t.end) {
                    t.vk[u] = a.v_tab[(size_t)pj * Nt + idx];
                    if (a.sse_out) t.rf[u] = a.sse_ref[(size_t)pj * Nt + idx];
                  }
                }
              }
              return t;
            };
            // 6-state kernels (one wavefront per SIMD, registers to spare): the next pass's entry and table loads are issued before this
            // pass is evaluated.  2-state kernels (three per SIMD, 168 registers): no cross-pass prefetch -- two live entries cost
            // 14-28 spilled registers, and the fused objective stores nothing its loads could queue behind
            constexpr bool PREF = (D > 2);
            Ent nx{};
            if constexpr (PREF) nx = decode(0);
            for (int c0 = 0; c0 < C; c0 += 64 / PKL) {
              const Ent cur = PREF ? nx : decode(c0);
              if constexpr (PREF) { if (c0 + 64 / PKL < C) nx = decode(c0 + 64 / PKL); }
              const int jj = cur.jj;
              Interp<S, D> itp;
              load_interp(itp, jj);
              const int tr = trl[jj];
              double tk[NSL];
              SV xv;
#pragma unroll
              for (int u = 0; u < NSL; ++u) {
                tk[u] = te_at(cur.idx0 + u * PKL);
                xv[u] = itp.x(tk[u]);
              }
              SV ov[D];
              interp_eval<S, D>(itp.cb, xv, ov);
              double rr2[NSL];
#pragma unroll
              for (int u = 0; u < NSL; ++u) {
                const int idx = cur.idx0 + u * PKL;
                rr2[u] = 0.0;
                if (cur.has && idx < cur.end) {
                  S out[D];
#pragma unroll
                  for (int d = 0; d < D; ++d) out[d] = ov[d][u];
                  if (!WI || a.y_out) store_state<S, D>(reinterpret_cast<S *>(a.y_out) + ((size_t)tr * Nt + idx) * D, out);
                  if constexpr (WI) {
                    double vk;
                    if constexpr (VTAB) vk = cur.vk[u];  // == protocol_v(a, pvb, t_eval[idx]), evaluated once per protocol by the pre-pass
                    else protocol_v(a, a.prot_v + (size_t)owp[jj] * a.Np, tk[u], vk);
                    const double ik = obs_current<S, D>(a, out, vk);
                    if (a.i_out) a.i_out[(size_t)tr * Nt + idx] = ik;
                    if (a.sse_out) { const double rr = ik - (VTAB ? cur.rf[u] : a.sse_ref[(size_t)owp[jj] * Nt + idx]); rr2[u] = rr; }
                  }
                }
              }
              if (WI && a.sse_out) {
                residual_terms(rr2, F::objective_kinds ? a.obj_abs : 0);   // the residuals' terms (rr2[u] held the residual itself up to here; 0 for no sample)
                // the chunk's sum in the canonical tree ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7)) over its 8 consecutive samples
                double g8;
                if constexpr (PKL == 4) {
                  double ql = rr2[0] + dpp_f64<0xB1, 0xf>(rr2[0]), qh = rr2[1] + dpp_f64<0xB1, 0xf>(rr2[1]);   // quad_perm [1,0,3,2]
                  ql = ql + dpp_f64<0x4E, 0xf>(ql); qh = qh + dpp_f64<0x4E, 0xf>(qh);                           // quad_perm [2,3,0,1]
                  g8 = ql + qh;
                } else {
                  double sj[NSL];
#pragma unroll
                  for (int u = 0; u < NSL; ++u) sj[u] = rr2[u] + dpp_f64<0xB1, 0xf>(rr2[u]);
                  g8 = (sj[0] + sj[1]) + (sj[2] + sj[3]);
                }
                if (kk == 0 && cur.has) ssep[jj * 8 + cur.part] += g8;
              }
            }
          };
          if (emd) emit_packed(std::integral_constant<bool, VTAB>{});
        }
      }
      {
      // ---- owner wavefront evaluates and stores; the t_eval loads of the next trajectory are issued ahead ----
      unsigned long long em = __ballot(n_out > 0 && lane < LPS && !packed_lane);
      if (G > 1) {  // trajectory jj belongs to wavefront jj % G
        unsigned long long mine = 0ull;
#pragma unroll
        for (int k = 0; k < (TPW + G - 1) / G; ++k) mine |= 1ull << (wave + k * G);   // (fewer trajectories than wavefronts: masked by lane < LPS above)
        em &= mine;
      }
      int jj = em ? __builtin_ctzll(em) : 0;
      int o = __builtin_amdgcn_readlane(oi, jj);
      // closed-form kernels on a verified uniform output grid form t_k arithmetically (bit-equal to the t_eval entry)
      const bool arith_t = LW && a.te_exact;
      double tk_nxt = (em && o + lane < Nt) ? (arith_t ? te_at(o + lane) : a.t_eval[o + lane]) : 0.0;
      // table variant: V(t_k) and the reference current of the next trajectory's first chunk are in flight as well
      double vk_nxt = 0.0, rf_nxt = 0.0;
      auto prefetch_obs = [&](int jx, int ox) {
        if constexpr (VTAB) {
          const int pjx = __builtin_amdgcn_readlane(pidx, jx);
          if (ox + lane < Nt) {
            vk_nxt = a.v_tab[(size_t)pjx * Nt + ox + lane];
            if (a.sse_out) rf_nxt = a.sse_ref[(size_t)pjx * Nt + ox + lane];
          }
        }
      };
      if (em) prefetch_obs(jj, o);
      while (em) {
        em &= em - 1;
        const int jn = em ? __builtin_ctzll(em) : 0;
        const int on = __builtin_amdgcn_readlane(oi, jn);
        double tk = tk_nxt;
        const double vk_first = vk_nxt, rf_first = rf_nxt;
        if (em && on + lane < Nt) tk_nxt = arith_t ? te_at(on + lane) : a.t_eval[on + lane];  // next trajectory's first chunk, in flight meanwhile
        if (em) prefetch_obs(jn, on);
        const int n = __builtin_amdgcn_readlane(n_out, jj);
        Interp<S, D> itp;
        load_interp(itp, jj);
        const int tr = __builtin_amdgcn_readlane(traj, jj);
        S *__restrict__ yo = a.y_out ? reinterpret_cast<S *>(a.y_out) + (size_t)tr * Nt * D : nullptr;
        double *__restrict__ io = nullptr;
        const double *__restrict__ pvb = nullptr, *__restrict__ refb = nullptr, *__restrict__ vtb = nullptr;
        if (a.i_out || a.sse_out) {
          if (a.i_out) io = a.i_out + (size_t)tr * Nt;
          int pj;
          if constexpr (LW) pj = __builtin_amdgcn_readlane(pidx, jj);  // no dependent global load per emitting trajectory
          else pj = a.prot_of_traj ? a.prot_of_traj[tr] : (tr % a.P);
          pvb = a.prot_v + (size_t)pj * a.Np;
          if (a.sse_out) refb = a.sse_ref + (size_t)pj * Nt;
          if constexpr (VTAB) vtb = a.v_tab + (size_t)pj * Nt;
        }
        double sacc = 0.0;
        for (int c0 = 0; c0 < n; c0 += 64) {
          const int idx = o + c0 + lane;
          if (c0 > 0 && c0 + lane < n) tk = arith_t ? te_at(idx) : a.t_eval[idx];
          if (c0 + lane < n) {
            S out[D];
            interp_eval<S, D>(itp.cb, itp.x(tk), out);
            if (yo) store_state<S, D>(yo + (size_t)idx * D, out);
            if (pvb) {
              double vk;
              if constexpr (VTAB) vk = (c0 == 0) ? vk_first : vtb[idx];  // == protocol_v(a, pvb, t_eval[idx]), evaluated once per protocol by the pre-pass
              else protocol_v(a, pvb, tk, vk);
              const double ik = obs_current<S, D>(a, out, vk);
              if (io) io[idx] = ik;
              if (refb) { const double rr = ik - ((VTAB && c0 == 0) ? rf_first : refb[idx]); sacc += residual_term(rr, F::objective_kinds ? a.obj_abs : 0); }
            }
          }
        }
        if (a.sse_out) {  // fused objective: the step's squared residuals of trajectory jj
          if constexpr (LW) {
            // lane-wise kernels: a full wavefront reduction per emitting trajectory (6 DPP steps + broadcast) was a quarter of
            // the epilogue's instructions.  Reduce over groups of 8 lanes only and keep 8 partial sums per trajectory in LDS
            // (the aux region); they are added up once, at the end.
            const double g8 = group8_sum_f64(sacc);
            if ((lane & 7) == 0) ssep[jj * 8 + (lane >> 3)] += g8;
          } else {
#pragma unroll
            for (int msk = 32; msk >= 1; msk >>= 1) sacc += __shfl_xor(sacc, msk);
            if (j == jj) sse += sacc;
          }
        }
        jj = jn;
        o = on;
      }
      oi += n_out;
      }
      }
    } else {
      // ---- no grid hint: cooperative scan, every wavefront advances every cursor ----
      unsigned long long em = __ballot(acc_now && lane < LPS);
      while (em) {
        const int jj = __builtin_ctzll(em);
        em &= em - 1;
        const bool owner = (WPS == 1) || ((jj % WPS) == wis);
        int o = __builtin_amdgcn_readlane(oi, jj);
        const double t1b = bcast_f64(t1, jj);
        // every wavefront advances the output cursor; only the owner evaluates and stores
        // (this site loads the interpolant in place: through load_interp the register allocation of the 4- and 32-trajectory N = 200
        // tiles moved by 20 registers, profiles/interp_refactor.md)
        double t0b = 0.0, denb = 1.0, rdenb = 1.0;
        S cb[5][D];
        S *__restrict__ yo = nullptr;
        double *__restrict__ io = nullptr;
        const double *__restrict__ pvb = nullptr;
        if (owner) {
          if constexpr (LW) {
            const double2 *rj = reinterpret_cast<const double2 *>(lsm) + jj * IRow::CHUNKS;
            const double2 h0 = rj[0], h1 = rj[1];
            t0b = h0.x; denb = h0.y; rdenb = h1.x;
#pragma unroll
            for (int c = 0; c < 5; ++c)
#pragma unroll
              for (int d = 0; d < D; d += 2) {
                const double2 cc = rj[IRow::coef(c, d) / 2];
                cb[c][d] = (S)cc.x; cb[c][d + 1] = (S)cc.y;
              }
          } else {
            t0b = bcast_f64(t0, jj); denb = bcast_f64(den, jj); rdenb = bcast_f64(rden, jj);
#pragma unroll
            for (int c = 0; c < 5; ++c)
#pragma unroll
              for (int d = 0; d < D; ++d) cb[c][d] = bcast<S>(ic[c][d], jj);
          }
          const int tr = __builtin_amdgcn_readlane(traj, jj);
          yo = reinterpret_cast<S *>(a.y_out) + (size_t)tr * Nt * D;
          if (a.i_out) {
            io = a.i_out + (size_t)tr * Nt;
            const int pj = a.prot_of_traj ? a.prot_of_traj[tr] : (tr % a.P);
            pvb = a.prot_v + (size_t)pj * a.Np;
          }
        }
        for (;;) {
          const int idx = o + lane;
          const double tk = (idx < Nt) ? a.t_eval[idx] : __builtin_inf();
          const bool ok = tk <= t1b;
          if (owner && ok) {
            S out[D];
            interp_eval<S, D>(cb, interp_x<S>(tk, t0b, denb, rdenb), out);
            store_state<S, D>(yo + (size_t)idx * D, out);
            if (io) {
              double vk;
              protocol_v(a, pvb, tk, vk);
              io[idx] = obs_current<S, D>(a, out, vk);
            }
          }
          const int n = __builtin_popcountll(__ballot(ok));
          o += n;
          if (n < 64) break;
        }
        if (j == jj) oi = o;
      }
    }
    STAMP(stamps_, 7);  // slot 7: interpolant fit + cooperative dense output
    if (active) since = (acc_now && oi > oi_before) ? 0 : since + 1;
    // ---- checkpoint of the accepted step for the backward sweep: (t0, dt, first output index, outputs, y, k1..k7) ----
    if (a.ckpt != nullptr && acc_now && primary && nacc_before < a.ckpt_cap) {
      double *__restrict__ rec = a.ckpt + ((size_t)traj * a.ckpt_cap + nacc_before) * (4 + 8 * D);
      rec[0] = t0; rec[1] = dt; rec[2] = (double)oi_before; rec[3] = (double)(oi - oi_before);
#pragma unroll
      for (int d = 0; d < D; ++d) rec[4 + d] = (double)y[d];
#pragma unroll
      for (int jx = 0; jx < 7; ++jx)
#pragma unroll
        for (int d = 0; d < D; ++d) rec[4 + D + jx * D + d] = (double)k[jx][d];
    }
    // ---- advance the RK state ----
    if (acc_now) {
#pragma unroll
      for (int d = 0; d < D; ++d) { y[d] = yi[d]; f[d] = k[6][d]; }
      t = t1;
      if (oi >= Nt) active = false;  // all requested outputs produced
    }
    if (active || acc_now) dt = dt_capped;
#ifdef IONODE_STAMPS
    att_cyc[NET] += stamp_now() - att0_;
    att_n[NET] += 1;
#endif
