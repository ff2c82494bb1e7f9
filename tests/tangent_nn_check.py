"""Checker for the forward sensitivities of the NN models (sensitivity.current_s1 / gauss_newton with weights).  TEST INFRASTRUCTURE ONLY.

As tangent_check.jacobian for the closed-form models: forward-mode automatic differentiation through the torch restatement that
replays the oracle's accepted steps (tests/grad_check.py `replay`), here WITH the net's weights, one pass per rate parameter.  The
net is evaluated in fp32 as the reference evaluates it, its tangent with it.  Problems are sse_nn_cases' (weights c.w, protocols
c.pv, optional explicit protocol times c.pt, protocol per trajectory c.pot).  `manual_jacobian` is the tangent walk the HIP kernel
implements (csrc/ionode_tangent_nn.hpp) written out by hand in numpy; tests/test_tangent_nn_host.py checks the two against each
other on the CPU.  The Jacobians of the GPU comparisons' cases are recorded (tests/golden/make_tangent_nn_fixtures.py).  No GPU needed.
"""
import os

import numpy as np
import torch

import grad_check as G
import sse_nn_cases as N


CASES = [(2, 10, G.MODEL_NND), (1, 200, G.MODEL_NNF)]   # (L, N, model) of the GPU comparisons; both state dtypes each
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tangent_nn_jacobians.npz")


def case_key(L, N_, model, f32):
    return f"L{L}_N{N_}_model{model}_{'f32' if f32 else 'f64'}"


def checked_rows(c):
    """Every third healthy trajectory."""
    return [b for b in range(0, c.B, 3) if b != c.nan_row]


def recorded_jacobians(L, N_, model, f32):
    """{b: J [Nt, 8]} of sse_nn_cases.problem(L, N_, model, f32): `jacobian` below as tests/golden/make_tangent_nn_fixtures.py
    recorded it (a forward-mode pass through the replay takes 1.5 s per parameter on a CPU)."""
    with np.load(GOLDEN) as z:
        J = z[case_key(L, N_, model, f32)]
    return dict(zip(checked_rows(N.problem(L, N_, model, f32)), J))


def steps_and_anchors(oracle, c, b):
    """The oracle's accepted steps of trajectory b and (fp32 state) its own end-of-step states, as sse_nn_cases.checker takes them."""
    steps = N.accepted_steps_of(oracle, c, b)
    anchors = None
    if c.f32:
        ends = np.array([t0 + dt for t0, dt in steps])
        anchors = oracle.solve(c.model, c.params[b], c.pv[c.pot[b]], c.y0[b], np.concatenate([[c.te[0]], ends]), weights=c.w,
                               mlp_layers=c.L, mlp_width=c.N, prot_t=c.pt, prot_t0=0.0, prot_dt=1.0, state_f32=True)["y"][0][1:]
    return steps, anchors


def replay_current(oracle, c, b, p, steps, anchors):
    """i [Nt] fp64 of the frozen-step replay at rate parameters p (a torch tensor: plain or dual)."""
    pvb = c.pv[c.pot[b]]
    ptx = c.pt if c.pt is not None else np.arange(c.pv.shape[1], dtype=np.float64)
    yr = G.replay(c.model, torch.from_numpy(c.w.copy()), c.L, c.N, p, torch.tensor(c.y0[b], dtype=torch.float64), ptx, pvb, c.te, steps,
                  f32_times=c.f32, anchors=anchors)
    V = oracle.protocol_v(pvb, c.te, prot_t=c.pt, prot_t0=0.0, prot_dt=1.0)[0]
    return c.obs["obs_g"] * (yr[:, 0] * yr[:, 1]) * torch.from_numpy(V - c.obs["obs_e"])


def jacobian(oracle, c, b):
    """(i [Nt], J [Nt, 8]) of trajectory b: forward-mode AD through the replay, one pass of dual numbers per rate parameter (the
    net's one-dimensional matrix products do not batch under vmap, so the passes are not run as one).  NN-f: the passes of p1..p4,
    which its right-hand side never reads, are left out and their columns are the zeros they would return."""
    steps, anchors = steps_and_anchors(oracle, c, b)
    p0 = torch.tensor(c.params[b], dtype=torch.float64)
    fn = lambda p: replay_current(oracle, c, b, p, steps, anchors)   # noqa: E731
    i0, cols = None, []
    for j in range(8):
        if c.model == G.MODEL_NNF and j < 4:
            cols.append(None)
            continue
        i0, dj = torch.func.jvp(fn, (p0,), (torch.eye(8, dtype=torch.float64)[j],))
        cols.append(dj.numpy())
    J = np.stack([np.zeros(i0.shape[0]) if x is None else x for x in cols], axis=1)
    return i0.numpy(), J


def manual_jacobian(oracle, c, b, steps, anchors):
    """J [Nt, 8] by the step algebra of the HIP walk (csrc/ionode_tangent_nn.hpp), written out in numpy: per stage the net enters
    through ONE number, c = d net / d a at the stage input -- taken here, as the recompute kernel takes it, from a reverse pass
    through the fp32 net with unit seed -- and the tangent recurrence is Kd[a] = (c / 1000 - [NN-d](k1 + k2)) Yd[a] + [NN-d] df_a/dp_j,
    Kd[r] = -(k3 + k4) Yd[r] + df_r/dp_j, with k = p E, dk/dp_2q = E, dk/dp_2q+1 = +-V k.  Forward values in fp64 (anchored on the
    oracle's end-of-step states in fp32 state), as the kernel reads them from the checkpoints."""
    nnd = c.model == G.MODEL_NND
    p = c.params[b]
    pvb = c.pv[c.pot[b]]
    prot_t = c.pt if c.pt is not None else np.arange(c.pv.shape[1], dtype=np.float64)
    te = np.asarray(c.te, dtype=np.float64)
    Sx = np.float32 if c.f32 else np.float64
    V = oracle.protocol_v(pvb, c.te, prot_t=c.pt, prot_t0=0.0, prot_dt=1.0)[0]
    layers = G.split_flat(torch.from_numpy(c.w.copy()), c.L, c.N)
    sign = np.array([1.0, -1.0, 1.0, -1.0])

    def stage(v, Y, Yd):
        """f(v, Y) [2] and its tangent columns [2, 8] given the tangent Yd [2, 8] of Y."""
        a = torch.tensor(np.float32(Y[0]), requires_grad=True)
        net = G.net_eval(layers, torch.stack([torch.tensor(np.float32(v / 100.0)), a]))
        (cn,) = torch.autograd.grad(net, a)
        cn = float(cn) / 1000.0
        E = np.exp(sign * p[1::2] * v)
        if not nnd:
            E[:2] = 0.0
        k = p[0::2] * E
        g = np.array([[1.0 - Y[0], 0.0], [-Y[0], 0.0], [0.0, -Y[1]], [0.0, 1.0 - Y[1]]])   # df/dk_q
        f = k @ g + np.array([float(net.detach()) / 1000.0, 0.0])
        fd = np.zeros((2, 8))
        for j in range(8):
            q = j // 2
            fd[0, j] = (cn - (k[0] + k[1])) * Yd[0, j]
            fd[1, j] = -(k[2] + k[3]) * Yd[1, j]
            fd[:, j] += (E[q] if j % 2 == 0 else sign[q] * v * k[q]) * g[q]
        return f, fd

    y = np.array(c.y0[b], dtype=np.float64)
    Sd = np.zeros((2, 8))
    f, fd = stage(G.protocol_v(float(Sx(te[0])), prot_t, pvb), y, Sd)
    out = [np.zeros(8)]
    oi = 1
    g_, e_ = c.obs["obs_g"], c.obs["obs_e"]
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
            kn, kdn = stage(G.protocol_v(ts[i], prot_t, pvb), Yi, Yd)
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
            out.append(g_ * (V[oi] - e_) * (sk[0] * yk[1] + yk[0] * sk[1]))
            oi += 1
        y, f, Sd, fd = y1, k[6], S1, kd[6]
    assert oi == te.size
    return np.stack(out)


def column_errors(J, want, cols):
    """Per parameter column of `cols`, rel-L2 over the samples."""
    J, want = np.asarray(J, dtype=np.float64)[:, cols], np.asarray(want, dtype=np.float64)[:, cols]
    return np.linalg.norm(J - want, axis=0) / np.maximum(np.linalg.norm(want, axis=0), 1e-300)
