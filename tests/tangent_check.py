"""Checker for the forward sensitivities of the current trace (sensitivity.current_s1 / gauss_newton).  TEST INFRASTRUCTURE ONLY.

The reference has no sensitivities (PINTS' simulateS1 is never called), so, as for the gradients, the checker is automatic
differentiation of the torch restatement that replays the oracle's accepted steps (tests/grad_check.py `replay`): here in FORWARD
mode, one pass per rate parameter, which gives the Jacobian J[k, j] = di_k/dp_j of the current trace column by column.
`manual_jacobian` is the tangent sweep the HIP kernel implements (csrc/ionode_tangent.hpp), written out by hand in numpy, as
grad_check.manual_adjoint is for the reverse sweep; tests/test_tangent_checker.py checks the two against each other, against central
differences and against reverse-mode autograd on the CPU, before any GPU run.  No GPU needed.
"""
from types import SimpleNamespace

import numpy as np
import torch

import grad_check as G
import kat_cases as K
import sse_cases as S


def obs_of(model):
    """HH 2-state: gate = a r, the reference's current; 6-state: the open state, with a conductance (tests/test_gpu_sse_grad.py)."""
    return dict(obs_g=1.0, obs_e=-86.0, obs_open_state_only=False) if model == K.MODEL_HH2 else \
        dict(obs_g=0.7, obs_e=-86.0, obs_open_state_only=True)


def problem(ion, model, B, seed, f32=False, te=None, obs=None, prot_t=None, pot="random", **over):
    """A batch on three protocols with steps and holds, in sse_cases' namespace form (what its oracle helpers read), with the
    stable step cap the gradient comparisons run under."""
    rng = np.random.default_rng(seed)
    m6 = model == K.MODEL_MARKOV6
    pv = np.stack([K.atau(30)[1][900:1300], K.atau(100)[1][900:1300], K.activation(20)[1][:400]])
    te = np.arange(0.0, 140.0, 1.0) if te is None else np.asarray(te, dtype=np.float64)
    params = np.tile(K.P_M6 if m6 else K.P_HH, (B, 1)) * rng.uniform(0.8, 1.25, (B, 12 if m6 else 8))
    y0 = np.stack([rng.uniform(0.0, 0.3, B), rng.uniform(0.6, 1.0, B)], 1)
    if m6:
        y0 = np.concatenate([y0, rng.uniform(0.0, 0.1, (B, 4))], 1)
    if f32:
        y0 = y0.astype(np.float32).astype(np.float64)
    cap = ion.grad.stable_step_cap(model, torch.from_numpy(params), torch.from_numpy(pv))
    c = SimpleNamespace(model=model, f32=f32, B=B, P=3, pv=pv, prot_t=prot_t, prot_t0=0.0, prot_dt=1.0, te=te, params=params, y0=y0,
                        pot=rng.integers(0, 3, B).astype(np.int32) if isinstance(pot, str) else pot, rtol=1e-7, atol=1e-9, max_steps=0,
                        max_total_steps=0, max_step=cap, obs=obs or obs_of(model), ref=rng.normal(0.0, 3.0, (3, te.size)))
    for k, v in over.items():
        setattr(c, k, v)
    return c


def steps_and_anchors(oracle, c, b):
    """The oracle's accepted steps of trajectory b and (fp32 state) its own end-of-step states, as sse_cases.reference_gradient."""
    o, steps = S.accepted_steps_of(oracle, c, b)
    assert o["status"][0] == 0, "the checker differentiates successful solves only"
    anchors = None
    if c.f32:
        ends = np.array([t0 + dt for t0, dt in steps])
        anchors = oracle.solve(c.model, c.params[b], c.pv[S.prot_index(c, b)], c.y0[b], np.concatenate([[c.te[0]], ends]), state_f32=True,
                               **{**S.solve_kw(c), "max_steps": 0, "max_total_steps": 0})["y"][0][1:]
    return steps, anchors


def _grid(c):
    return c.prot_t if c.prot_t is not None else c.prot_t0 + np.arange(c.pv.shape[1]) * c.prot_dt


def replay_current(oracle, c, b, p, steps, anchors):
    """i [Nt] fp64 of the frozen-step replay at rate parameters p (a torch tensor: plain, dual or requiring grad)."""
    yr = G.replay(c.model, None, 0, 0, p, torch.tensor(c.y0[b], dtype=torch.float64), _grid(c), c.pv[S.prot_index(c, b)], c.te, steps,
                  f32_times=c.f32, anchors=anchors)
    gate = yr[:, -1] if c.obs["obs_open_state_only"] else yr[:, 0] * yr[:, 1]
    return c.obs["obs_g"] * gate * torch.from_numpy(S.voltage_at_outputs(oracle, c, b) - c.obs["obs_e"])


def jacobian(oracle, c, b, steps=None, anchors=None):
    """(i [Nt], J [Nt, NPAR]) of trajectory b: forward-mode AD through the replay, the parameters' passes run as one (vmap over
    the dual numbers: the same bits as one pass per parameter, a tenth of the time)."""
    if steps is None:
        steps, anchors = steps_and_anchors(oracle, c, b)
    p0 = torch.tensor(c.params[b], dtype=torch.float64)
    with torch.no_grad():
        i0 = replay_current(oracle, c, b, p0, steps, anchors).numpy()
    J = torch.autograd.functional.jacobian(lambda p: replay_current(oracle, c, b, p, steps, anchors), p0, strategy="forward-mode",
                                           vectorize=True)
    return i0, J.numpy()


# ---- the tangent sweep by hand (csrc/ionode_tangent.hpp) ----
# Both models are linear in their rates: f(Y) = sum_q k_q g_q(Y), g_q affine in Y.  g_q per model, rate order as the parameters' (p[2q]
# the amplitude, p[2q + 1] the exponent, sign + for even q and - for odd q).
def _g(model, q, Y):
    if model == K.MODEL_MARKOV6:
        c1, c2, i_, ic1, ic2, o = Y
        z = 0.0 * c1
        return np.array([[c2, -c2, z, ic2, -ic2, z], [-c1, c1, z, -ic1, ic1, z], [-c1, -c2, o, c1, c2, -o],
                         [ic1, ic2, -i_, -ic1, -ic2, i_], [-c1, z, ic1, -ic1, z, c1], [o, z, -i_, i_, z, -o]][q])
    a, r = Y
    z = 0.0 * a
    return np.array([[1.0 - a, z], [-a, z], [z, -r], [z, 1.0 - r]][q])


def manual_jacobian(oracle, c, b, steps, anchors):
    """J [Nt, NPAR] by the step algebra of the kernel: S = dy/dp carried through the accepted steps (K1 of a step is K7 of its
    predecessor, S <- the tangent of y1), the interpolant's formulas applied to (S, S_next, Kd1, Kd7, S_mid), the observation's
    product rule.  Forward values are recomputed in fp64 (anchored on the oracle's end-of-step states in fp32 state), as the kernel
    reads them from the checkpoints."""
    model, p = c.model, c.params[b]
    npar, nr = p.size, p.size // 2
    prot_t, prot_v = _grid(c), c.pv[S.prot_index(c, b)]
    te = np.asarray(c.te, dtype=np.float64)
    Sx = np.float32 if c.f32 else np.float64
    V = S.voltage_at_outputs(oracle, c, b)
    sign = np.array([1.0 if q % 2 == 0 else -1.0 for q in range(nr)])

    def stage(v, Y, Yd):
        """f(v, Y) and its tangent columns [D, NPAR] given the tangent Yd [D, NPAR] of Y."""
        E = np.exp(sign * p[1::2] * v)
        k = p[0::2] * E
        zero = np.zeros_like(Y)
        f = sum(k[q] * _g(model, q, Y) for q in range(nr))
        fd = np.zeros_like(Yd)
        for j in range(npar):
            q = j // 2
            fd[:, j] = sum(k[m] * (_g(model, m, Yd[:, j]) - _g(model, m, zero)) for m in range(nr))   # A(v) Yd
            fd[:, j] += (E[q] if j % 2 == 0 else sign[q] * v * k[q]) * _g(model, q, Y)                  # dk_q/dp_j g_q(Y)
        return f, fd

    y = np.array(c.y0[b], dtype=np.float64)
    D = y.size
    Sd = np.zeros((D, npar))
    f, fd = stage(G.protocol_v(float(Sx(te[0])), prot_t, prot_v), y, Sd)
    out = [np.zeros(npar)]
    oi = 1
    g, e = c.obs["obs_g"], c.obs["obs_e"]
    for n, (t0, dt) in enumerate(steps):
        if oi >= te.size:
            break
        t1 = t0 + dt
        ts = G.stage_times(t0, dt, c.f32)
        dts = float(Sx(dt))
        k, kd = [f], [fd]
        for i in range(6):
            Yi = y + sum(k[m] * (G.BETA[i][m] * dts) for m in range(i + 1))
            Yd = Sd + sum(kd[m] * (G.BETA[i][m] * dts) for m in range(i + 1))
            if i == 5 and anchors is not None:
                Yi = np.asarray(anchors[n], dtype=np.float64)
            kn, kdn = stage(G.protocol_v(ts[i], prot_t, prot_v), Yi, Yd)
            k.append(kn)
            kd.append(kdn)
        y1, S1 = Yi, Yd

        def coefficients(Y0, Y1, F0, F1, ks):
            YM = Y0 + sum(ks[m] * (G.CMID[m] * dts) for m in range(7))
            return [Y0, dts * F0, dts * (F1 - 4 * F0) - 11 * Y0 - 5 * Y1 + 16 * YM, dts * (5 * F0 - 3 * F1) + 18 * Y0 + 14 * Y1 - 32 * YM,
                    2 * dts * (F1 - F0) - 8 * (Y1 + Y0) + 16 * YM]
        cy, cs = coefficients(y, y1, k[0], k[6], k), coefficients(Sd, S1, kd[0], kd[6], kd)
        while oi < te.size and te[oi] <= t1:
            x = float(Sx((te[oi] - t0) / (t1 - t0)))
            yk = sum(cy[m] * x ** m for m in range(5))
            sk = sum(cs[m] * x ** m for m in range(5))
            gd = g * (V[oi] - e)
            out.append(gd * sk[-1] if c.obs["obs_open_state_only"] else gd * (sk[0] * yk[1] + yk[0] * sk[1]))
            oi += 1
        y, f, Sd, fd = y1, k[6], S1, kd[6]
    assert oi == te.size
    return np.stack(out)


def column_errors(J, want):
    """Per parameter column, rel-L2 over the samples."""
    J, want = np.asarray(J, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return np.linalg.norm(J - want, axis=0) / np.maximum(np.linalg.norm(want, axis=0), 1e-300)
