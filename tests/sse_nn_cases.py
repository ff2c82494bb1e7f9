"""Problems and references for the fused sum-of-squares gradient of the NN models (grad.sum_of_squares with weights_flat).  No GPU
needed to import.  The problem is test_gpu_grad.test_other_widths_and_depths_against_the_checker's (19 trajectories = two tiles, the
second ragged; two protocols of 400 samples; one NaN start) with a random reference trace and random positive upstream weights.
References: the materialised route (grad.solve -> current and residuals in torch -> autograd) and autograd through the torch replay
of the oracle's accepted steps (tests/grad_check.py)."""
from types import SimpleNamespace

import numpy as np
import torch

import grad_check as G
import kat_cases as K

NAN_ROW = 5


def rand_weights(L, N, seed):
    rng = np.random.default_rng(seed)  # gain ~1 per layer so that deep stacks stay O(1): sigma = 1 / sqrt(N), capped (tests/test_gpu_grad.py)
    return rng.normal(0, min(0.3, 1.0 / np.sqrt(N)), 2 * N + N + L * (N * N + N) + N + 1).astype(np.float32)


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def obs_of(model):
    # NN-f: the reference's current; NN-d: a conductance and another reversal potential, so that both reach the kernel
    return dict(obs_g=1.0, obs_e=-86.0, obs_open_state_only=False) if model == K.MODEL_NNF else \
        dict(obs_g=0.7, obs_e=-80.0, obs_open_state_only=False)


def problem(L, N, model, f32, te=None, explicit=True, nan_row=NAN_ROW):
    rng = np.random.default_rng(L + N + 2 * f32)
    c = SimpleNamespace(L=L, N=N, model=model, f32=f32, B=19, nan_row=nan_row)
    c.w = rand_weights(L, N, 11 * L + N)
    c.pv = np.stack([K.atau(30)[1][900:1300], K.atau(100)[1][900:1300]])
    pt = np.arange(400, dtype=np.float64) * 1.0
    pt[1:] += rng.uniform(-1e-7, 1e-7, 399)                  # not uniform in bits: the explicit-grid lookup
    c.pt = pt if explicit else None
    c.te = np.arange(0.0, 140.0, 1.0) if te is None else np.asarray(te, dtype=np.float64)
    c.params = np.tile(K.P_HH, (c.B, 1)) * rng.uniform(0.9, 1.1, (c.B, 8))
    c.pot = (np.arange(c.B) % 2).astype(np.int32)
    y0 = np.stack([rng.uniform(0.0, 0.3, c.B), rng.uniform(0.6, 1.0, c.B)], 1)
    if f32:
        y0 = y0.astype(np.float32).astype(np.float64)        # the state dtype of the caller's y0
    if nan_row is not None:
        y0[nan_row, 0] = np.nan
    c.y0 = y0
    c.ref = rng.normal(0.0, 3.0, (2, c.te.size))
    c.up = rng.uniform(0.5, 1.5, c.B)                        # upstream dL/dsse
    c.obs = obs_of(model)
    return c


def rows_of(c, rows):
    """The same problem restricted to `rows` (the loss then sums those trajectories only)."""
    d = SimpleNamespace(**vars(c))
    d.B = len(rows)
    d.params, d.pot, d.y0, d.up = c.params[rows], c.pot[rows], c.y0[rows], c.up[rows]
    d.nan_row = None
    return d


def _dev(gpu, *xs):
    return [None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(gpu) for x in xs]


def _leaves(gpu, c):
    sdt = torch.float32 if c.f32 else torch.float64
    wt = torch.from_numpy(c.w.copy()).to(gpu).requires_grad_(True)
    p = torch.from_numpy(c.params).to(gpu).requires_grad_(True)
    y0t = torch.from_numpy(c.y0).to(gpu).to(sdt).requires_grad_(True)
    return wt, p, y0t


def _out(st, wt, p, y0t, sse=None):
    return SimpleNamespace(sse=None if sse is None else sse.detach().cpu().numpy(), st=st.cpu().numpy(), gw=wt.grad.double().cpu().numpy(),
                           gp=p.grad.cpu().numpy(), gy0=y0t.grad.double().cpu().numpy())


def fused(ion, gpu, c, **kw):
    pv, te, pot, ref, pt = _dev(gpu, c.pv, c.te, c.pot, c.ref, c.pt)
    wt, p, y0t = _leaves(gpu, c)
    sse, st = ion.grad.sum_of_squares(c.model, p, pv, y0t, te, ref, prot_t=pt, prot_t0=0.0, prot_dt=1.0, prot_of_traj=pot,
                                      weights_flat=wt, mlp_layers=c.L, mlp_width=c.N, **c.obs, **kw)
    sse.backward(torch.from_numpy(c.up).to(gpu))             # failed rows: upstream ignored
    return _out(st, wt, p, y0t, sse)


def materialised(ion, gpu, c, **kw):
    pv, te, pot, ref, pt = _dev(gpu, c.pv, c.te, c.pot, c.ref, c.pt)
    wt, p, y0t = _leaves(gpu, c)
    y, st = ion.grad.solve(c.model, wt, p, pv, y0t, te, mlp_layers=c.L, mlp_width=c.N, prot_t=pt, prot_t0=0.0, prot_dt=1.0,
                           prot_of_traj=pot, **kw)
    d = ion.capi.make_desc(n_out=c.te.size, n_prot=c.pv.shape[0], prot_n=c.pv.shape[1], prot_t0=0.0, prot_dt=1.0, v_oob=-80.0)
    V = ion.capi.protocol_at_outputs(d, pv, pt, te)[pot.long()]                       # [B, Nt]
    yd = y.double()
    i = c.obs["obs_g"] * (yd[..., 0] * yd[..., 1]) * (V - c.obs["obs_e"])
    per = ((i - ref[pot.long()]) ** 2).sum(1)
    (torch.where(st == 0, per, torch.zeros_like(per)) * torch.from_numpy(c.up).to(gpu)).sum().backward()
    return _out(st, wt, p, y0t)


def fused_forward(ion, gpu, c):
    """sse of batched.solve(sse_ref=, states=False): the values the fused route must return."""
    pv, te, pot, ref, pt = _dev(gpu, c.pv, c.te, c.pot, c.ref, c.pt)
    sdt = torch.float32 if c.f32 else torch.float64
    sol = ion.batched.solve(c.model, torch.from_numpy(c.params).to(gpu), pv, torch.from_numpy(c.y0).to(gpu).to(sdt), te,
                            weights=c.w, mlp_layers=c.L, mlp_width=c.N, prot_t=pt, prot_t0=0.0, prot_dt=1.0, prot_of_traj=pot,
                            sse_ref=ref, states=False, **c.obs)
    return sol


def param_cols(model):
    return slice(4, 8) if model == K.MODEL_NNF else slice(0, 8)   # NN-f has no p1..p4


def accepted_steps_of(oracle, c, b):
    o = oracle.solve(c.model, c.params[b], c.pv[c.pot[b]], c.y0[b], c.te, weights=c.w, mlp_layers=c.L, mlp_width=c.N, prot_t=c.pt,
                     prot_t0=0.0, prot_dt=1.0, state_f32=c.f32, step_log_cap=1 << 15)
    assert o["status"][0] == 0
    return G.accepted_steps(o["step_log"])


def checker(oracle, c, rows):
    """Autograd through the replay of the oracle's accepted steps, the sum of squares formed in torch fp64:
    ({b: (dL/dp, dL/dy0)}, dL/dW summed over `rows`) of L = sum_b up[b] sse[b]."""
    flat = torch.from_numpy(c.w.copy()).requires_grad_(True)
    ptx = c.pt if c.pt is not None else np.arange(c.pv.shape[1], dtype=np.float64)
    out = {}
    for b in rows:
        pvb = c.pv[c.pot[b]]
        steps = accepted_steps_of(oracle, c, b)
        anchors = None
        if c.f32:   # fp32 state: the Jacobians along the forward's own end-of-step states (grad_check.replay)
            ends = np.array([t0 + dt for t0, dt in steps])
            anchors = oracle.solve(c.model, c.params[b], pvb, c.y0[b], np.concatenate([[c.te[0]], ends]), weights=c.w, mlp_layers=c.L,
                                   mlp_width=c.N, prot_t=c.pt, prot_t0=0.0, prot_dt=1.0, state_f32=True)["y"][0][1:]
        pb = torch.tensor(c.params[b], dtype=torch.float64, requires_grad=True)
        yb = torch.tensor(c.y0[b], dtype=torch.float64, requires_grad=True)
        yr = G.replay(c.model, flat, c.L, c.N, pb, yb, ptx, pvb, c.te, steps, f32_times=c.f32, anchors=anchors)
        V = oracle.protocol_v(pvb, c.te, prot_t=c.pt, prot_t0=0.0, prot_dt=1.0)[0]
        i = c.obs["obs_g"] * (yr[:, 0] * yr[:, 1]) * torch.from_numpy(V - c.obs["obs_e"])
        (c.up[b] * ((i - torch.from_numpy(c.ref[c.pot[b]])) ** 2).sum()).backward()
        out[b] = (pb.grad.numpy(), yb.grad.numpy())
    return out, flat.grad.double().numpy()


def check_against_checker(ion, gpu, oracle, c, got, tol):
    """Every third healthy trajectory against the checker (dL/dp, dL/dy0 per trajectory); dL/dW: the fused route once more on the
    checked rows only, so that both sides sum the same trajectories.  Returns the worst relative errors."""
    rows = [b for b in range(0, c.B, 3) if b != c.nan_row]
    want, want_w = checker(oracle, c, rows)
    cols = param_cols(c.model)
    worst = max(max(rel(got.gp[b, cols], want[b][0][cols]), rel(got.gy0[b], want[b][1])) for b in rows)
    sub = fused(ion, gpu, rows_of(c, rows))
    assert (sub.st == 0).all()
    ew = rel(sub.gw, want_w)
    assert worst <= tol and ew <= tol, (worst, ew)
    return worst, ew
