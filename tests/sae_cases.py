"""References for the fused sum-of-absolute-errors gradient (grad.sum_of_abs), on the problems of tests/sse_cases.py (closed-form
models) and tests/sse_nn_cases.py (NN-f / NN-d).  No GPU needed to import; neither of those helpers nor grad_check.py is modified.

The derivative of sum_k |r_k| is discontinuous in r, so the checker must not decide the sign pattern itself: its fp64 replay of the
accepted steps differs from the solve by the state dtype's rounding, and one flipped sample in a few thousand moves the gradient by
about 1e-3 (seed 10 of sse_cases, fp32 state on a dense grid: min |r| = 1.3e-4 against max |i_oracle - i_replay| = 6.4e-5).  The
signs come from the arithmetic the kernel runs: s_k = sign(oracle.current(oracle states, state dtype) - ref_k) -- the HIP kernels
are bit-identical to the oracle -- and the checker differentiates up[b] * sum_k s_k * r_k(replay) by autograd through
grad_check.replay, exactly as sse_cases.reference_gradient and sse_nn_cases.checker differentiate the squares.  No sample and no case
is left out; the samples where the replay's own sign differs from s_k are COUNTED and reported, never filtered on.

`wrong`: one deliberately wrong weight per sample instead of s_k (WRONG_WEIGHTS); tests/test_sae_cases.py shows with them that the
drawn inputs would expose the corresponding kernel mistakes."""
import numpy as np
import torch

import grad_check as G
import sse_cases as S
import sse_nn_cases as N

WRONG_WEIGHTS = ["plus_one", "two_r", "sign0_is_1"]


def sample_weights(i_kernel, ref, wrong=None):
    """d term / d r per sample from the kernel's own residuals r = i_kernel - ref: sign(r) with sign(0) = 0 (torch.abs's backward), or
    one of WRONG_WEIGHTS -- +1 everywhere, the squares' 2 r, sign with sign(0) = 1."""
    r = np.asarray(i_kernel, dtype=np.float64) - np.asarray(ref, dtype=np.float64)
    assert wrong is None or wrong in WRONG_WEIGHTS
    if wrong is None:
        return np.sign(r)
    if wrong == "plus_one":
        return np.ones_like(r)
    if wrong == "two_r":
        return 2.0 * r
    return np.where(r >= 0.0, 1.0, -1.0)


def sign_flips(i_replay, i_kernel, ref):
    """Samples at which the replay's own residual has another sign than the kernel's."""
    return int((np.sign(np.asarray(i_replay) - ref) != np.sign(np.asarray(i_kernel) - ref)).sum())


# ---- closed-form models: the cases of sse_cases.case(seed) ----

def kernel_current(oracle, c, b, y):
    """The current the kernel forms for trajectory b from its states y [Nt, D]: the oracle's, in the state dtype."""
    return oracle.current(y, S.voltage_at_outputs(oracle, c, b), g=c.obs["obs_g"], e_rev=c.obs["obs_e"], state_f32=c.f32,
                          open_state_only=c.obs["obs_open_state_only"])


def ref_with_exact_zeros(oracle, c, b, every=4):
    """c.ref's row of trajectory b with every `every`-th sample (sample 0 included) set to the kernel's own current there: exact zeros
    of the residual."""
    o, _ = S.accepted_steps_of(oracle, c, b)
    row = c.ref[S.prot_index(c, b)].copy()
    row[::every] = kernel_current(oracle, c, b, o["y"][0])[::every]
    return row


def reference_gradient(oracle, c, b, wrong=None, ref_row=None):
    """(dL/dp [n_par], dL/dy0 [D], sign flips) of L = w[b] * sae[b]: sse_cases.reference_gradient with sum_k s_k r_k(replay) in the
    place of the sum of squares.  ref_row: another reference trace for this trajectory than c.ref's."""
    p = S.prot_index(c, b)
    o, steps = S.accepted_steps_of(oracle, c, b)
    assert o["status"][0] == 0, "the checker differentiates successful solves only"
    kw = S.solve_kw(c)
    anchors = None
    if c.f32:
        ends = np.array([t0 + dt for t0, dt in steps])
        anchors = oracle.solve(c.model, c.params[b], c.pv[p], c.y0[b], np.concatenate([[c.te[0]], ends]), state_f32=True,
                               **{**kw, "max_steps": 0, "max_total_steps": 0})["y"][0][1:]
    ptx = c.prot_t if c.prot_t is not None else c.prot_t0 + np.arange(c.pv.shape[1]) * c.prot_dt
    pb = torch.tensor(c.params[b], dtype=torch.float64, requires_grad=True)
    yb = torch.tensor(c.y0[b], dtype=torch.float64, requires_grad=True)
    yr = G.replay(c.model, None, 0, 0, pb, yb, ptx, c.pv[p], c.te, steps, f32_times=c.f32, anchors=anchors)
    gate = yr[:, -1] if c.obs["obs_open_state_only"] else yr[:, 0] * yr[:, 1]
    i = c.obs["obs_g"] * gate * torch.from_numpy(S.voltage_at_outputs(oracle, c, b) - c.obs["obs_e"])
    ref = c.ref[p] if ref_row is None else np.asarray(ref_row, dtype=np.float64)
    i_kernel = kernel_current(oracle, c, b, o["y"][0])
    s = sample_weights(i_kernel, ref, wrong)
    (c.w[b] * (torch.from_numpy(s) * (i - torch.from_numpy(ref))).sum()).backward()
    return pb.grad.numpy(), yb.grad.numpy(), sign_flips(i.detach().numpy(), i_kernel, ref)


# ---- NN-f / NN-d: the problems of sse_nn_cases.problem ----

def _nn_oracle(oracle, c, b):
    o = oracle.solve(c.model, c.params[b], c.pv[c.pot[b]], c.y0[b], c.te, weights=c.w, mlp_layers=c.L, mlp_width=c.N, prot_t=c.pt,
                     prot_t0=0.0, prot_dt=1.0, state_f32=c.f32, step_log_cap=1 << 15)
    assert o["status"][0] == 0
    return o


def nn_kernel_current(oracle, c, b, y=None):
    """(i, V): the current the kernel forms for trajectory b (the oracle's, state dtype) and the voltages at the output times."""
    if y is None:
        y = _nn_oracle(oracle, c, b)["y"][0]
    V = oracle.protocol_v(c.pv[c.pot[b]], c.te, prot_t=c.pt, prot_t0=0.0, prot_dt=1.0)[0]
    return oracle.current(y, V, g=c.obs["obs_g"], e_rev=c.obs["obs_e"], state_f32=c.f32,
                          open_state_only=c.obs["obs_open_state_only"]), V


def nn_checker(oracle, c, rows):
    """sse_nn_cases.checker with sum_k s_k r_k(replay) in the place of the sum of squares:
    ({b: (dL/dp, dL/dy0)}, dL/dW summed over `rows`, sign flips over `rows`) of L = sum_b up[b] sae[b]."""
    flat = torch.from_numpy(c.w.copy()).requires_grad_(True)
    ptx = c.pt if c.pt is not None else np.arange(c.pv.shape[1], dtype=np.float64)
    out, flips = {}, 0
    for b in rows:
        pvb = c.pv[c.pot[b]]
        o = _nn_oracle(oracle, c, b)
        steps = G.accepted_steps(o["step_log"])
        anchors = None
        if c.f32:   # fp32 state: the Jacobians along the forward's own end-of-step states (grad_check.replay)
            ends = np.array([t0 + dt for t0, dt in steps])
            anchors = oracle.solve(c.model, c.params[b], pvb, c.y0[b], np.concatenate([[c.te[0]], ends]), weights=c.w, mlp_layers=c.L,
                                   mlp_width=c.N, prot_t=c.pt, prot_t0=0.0, prot_dt=1.0, state_f32=True)["y"][0][1:]
        pb = torch.tensor(c.params[b], dtype=torch.float64, requires_grad=True)
        yb = torch.tensor(c.y0[b], dtype=torch.float64, requires_grad=True)
        yr = G.replay(c.model, flat, c.L, c.N, pb, yb, ptx, pvb, c.te, steps, f32_times=c.f32, anchors=anchors)
        i_kernel, V = nn_kernel_current(oracle, c, b, o["y"][0])
        i = c.obs["obs_g"] * (yr[:, 0] * yr[:, 1]) * torch.from_numpy(V - c.obs["obs_e"])
        ref = c.ref[c.pot[b]]
        s = sample_weights(i_kernel, ref)
        (c.up[b] * (torch.from_numpy(s) * (i - torch.from_numpy(ref))).sum()).backward()
        out[b] = (pb.grad.numpy(), yb.grad.numpy())
        flips += sign_flips(i.detach().numpy(), i_kernel, ref)
    return out, flat.grad.double().numpy(), flips


def nn_fused(ion, gpu, c, **kw):
    """grad.sum_of_abs on the problem, backward with c.up: sse_nn_cases.fused for the absolute values (the sums under .sse)."""
    pv, te, pot, ref, pt = N._dev(gpu, c.pv, c.te, c.pot, c.ref, c.pt)
    wt, p, y0t = N._leaves(gpu, c)
    sae, st = ion.grad.sum_of_abs(c.model, p, pv, y0t, te, ref, prot_t=pt, prot_t0=0.0, prot_dt=1.0, prot_of_traj=pot,
                                  weights_flat=wt, mlp_layers=c.L, mlp_width=c.N, **c.obs, **kw)
    sae.backward(torch.from_numpy(c.up).to(gpu))             # failed rows: upstream ignored
    return N._out(st, wt, p, y0t, sae)


def nn_materialised(ion, gpu, c, **kw):
    """grad.solve, then the current and abs() in torch: sse_nn_cases.materialised for the absolute values.  Also returns the
    residuals' smallest magnitude and the currents' largest over the healthy rows (the comparison's precondition)."""
    pv, te, pot, ref, pt = N._dev(gpu, c.pv, c.te, c.pot, c.ref, c.pt)
    wt, p, y0t = N._leaves(gpu, c)
    y, st = ion.grad.solve(c.model, wt, p, pv, y0t, te, mlp_layers=c.L, mlp_width=c.N, prot_t=pt, prot_t0=0.0, prot_dt=1.0,
                           prot_of_traj=pot, **kw)
    d = ion.capi.make_desc(n_out=c.te.size, n_prot=c.pv.shape[0], prot_n=c.pv.shape[1], prot_t0=0.0, prot_dt=1.0, v_oob=-80.0)
    V = ion.capi.protocol_at_outputs(d, pv, pt, te)[pot.long()]                       # [B, Nt]
    yd = y.double()
    i = c.obs["obs_g"] * (yd[..., 0] * yd[..., 1]) * (V - c.obs["obs_e"])
    r = i - ref[pot.long()]
    per = r.abs().sum(1)
    (torch.where(st == 0, per, torch.zeros_like(per)) * torch.from_numpy(c.up).to(gpu)).sum().backward()
    out = N._out(st, wt, p, y0t)
    ok = st == 0
    out.min_abs_r, out.max_abs_i = float(r[ok].detach().abs().min()), float(i[ok].detach().abs().max())
    return out


def nn_check_against_checker(ion, gpu, oracle, c, got, tol):
    """sse_nn_cases.check_against_checker for the absolute values: every third healthy trajectory (dL/dp, dL/dy0 per trajectory);
    dL/dW: the fused route once more on the checked rows only.  Returns the worst relative errors and the checker's sign flips."""
    rows = [b for b in range(0, c.B, 3) if b != c.nan_row]
    want, want_w, flips = nn_checker(oracle, c, rows)
    cols = N.param_cols(c.model)
    worst = max(max(N.rel(got.gp[b, cols], want[b][0][cols]), N.rel(got.gy0[b], want[b][1])) for b in rows)
    sub = nn_fused(ion, gpu, N.rows_of(c, rows))
    assert (sub.st == 0).all()
    ew = N.rel(sub.gw, want_w)
    print(f"  checker: worst dL/dp, dL/dy0 {worst:.2e}, dL/dW {ew:.2e}; {flips} samples where the replay's own sign differs")
    assert worst <= tol and ew <= tol, (worst, ew, flips)
    return worst, ew, flips
