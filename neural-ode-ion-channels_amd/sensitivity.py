"""Forward sensitivities of the current trace and their Gauss-Newton sums (closed-form HH 2-state and 6-state models).

Reference interface: PINTS `ForwardModelS1.simulateS1` -- the output AND its per-sample sensitivities dI(t_k)/dp_j -- the third of
the three PINTS evaluations behind the reference's fits (train-d0.py:508-540: SumOfSquaresError under a LogTransformation);
`batched.solve` / its fused `sse` are `simulate` / `SumOfSquaresError.__call__`, `grad.sum_of_squares` is `evaluateS1`.  The Jacobian
J[k, j] = di_k/dp_j is what Gauss-Newton / Levenberg-Marquardt steps (J^T J, J^T r), Fisher information and protocol design need; the
reverse sweep yields one row of J^T per launch, finite differences NPAR + 1 solves and half the digits.

What is computed: the tangent-mode derivative of the discretisation the forward launch executed (accepted steps as constants,
csrc/ionode_tangent.hpp) -- the same rule as grad.py's reverse mode, so 2 J^T r here equals the gradient of grad.sum_of_squares.
Two launches: the checkpointed forward (capi.dopri5, sized and regrown by grad._forward_with_checkpoints) and ionode_tangent_sweep.
Plain evaluations: no autograd graph is built, and there is no CPU fallback.

The optimiser is not here: fit.py's Levenberg-Marquardt driver builds on gauss_newton.  Out of scope: sensitivities with respect to y0, the NN models
(their tangent needs a Jacobian-vector product through the MLP tiles) and an absolute-error variant of the sums.
"""
import ctypes as C

import torch

from . import capi, grad


class _Saved:
    """What grad._forward_with_checkpoints leaves on an autograd context, kept on a plain object: (params, ckpt, stats, status)."""

    def save_for_backward(self, *tensors):
        self.saved_tensors = tensors

    def mark_non_differentiable(self, *tensors):
        pass


def _checked(who, model, params, prot_v, y0, kw):
    """The argument checks both entry points share; returns the keywords with max_step resolved."""
    if model in (capi.MODEL_NNF, capi.MODEL_NND):
        raise capi.IonodeError(f"{who}: the closed-form HH 2-state and 6-state models only (the NN models' tangent would need a "
                               "Jacobian-vector product through the MLP tiles)")
    if model not in (capi.MODEL_HH2, capi.MODEL_MARKOV6):
        raise NotImplementedError("unknown model")
    D, npar = capi.n_state(model), capi.n_params(model)
    if not (isinstance(y0, torch.Tensor) and isinstance(params, torch.Tensor)) or y0.dim() != 2 or y0.shape[1] != D or params.dim() != 2 \
            or params.shape[0] != y0.shape[0] or params.shape[1] != npar:
        raise capi.IonodeError(f"params [B, {npar}] and y0 [B, {D}] expected")
    if not y0.is_cuda:
        raise capi.IonodeError("no HIP tensors: the integrator and its tangent sweep have no CPU path")
    kw["max_step"] = grad._resolve_max_step(model, params.detach(), prot_v, kw["v_oob"], kw["max_step"], frames=3)
    return kw


def _forward(model, params, prot_v, y0, t_eval, kw, **cfg_extra):
    """The checkpointed forward with grad.py's sizing / regrow / budget logic.  Returns (capi.dopri5's result, params, checkpoints,
    n_accepted [B] int32 with failed trajectories zeroed)."""
    pot = kw["prot_of_traj"]
    cfg = dict(model=model, mlp_layers=0, mlp_width=0, prot_v=prot_v, prot_t=kw["prot_t"], prot_t0=float(kw["prot_t0"]),
               prot_dt=float(kw["prot_dt"]), t_eval=t_eval,
               prot_of_traj=None if pot is None else torch.as_tensor(pot, device=y0.device).to(torch.int32).contiguous(),
               rtol=float(kw["rtol"]), atol=float(kw["atol"]), v_oob=float(kw["v_oob"]), max_steps=int(kw["max_steps"]),
               max_total_steps=int(kw["max_total_steps"]), max_step=float(kw["max_step"]), obs_g=float(kw["obs_g"]),
               obs_e=float(kw["obs_e"]), obs_open_state_only=bool(kw["obs_open_state_only"]), ckpt_cap=kw["ckpt_cap"],
               ckpt_budget_bytes=kw["ckpt_budget_bytes"], **cfg_extra)
    ctx = _Saved()
    with torch.no_grad():
        r = grad._forward_with_checkpoints(ctx, None, params.detach().contiguous(), y0.detach().contiguous(), cfg, objective="sse_ref" in cfg)
    p, ckpt, stats, status = ctx.saved_tensors
    n_acc = torch.where(status != 0, torch.zeros_like(stats[:, 0]), stats[:, 0]).to(torch.int32).contiguous()
    return r, cfg, p, ckpt, n_acc


def _sweep(r, cfg, params, ckpt, n_acc, di_dp, jtr, jtj):
    """ionode_tangent_sweep on the current stream, with the descriptor of the forward that wrote `ckpt`."""
    desc = r["desc"]
    desc.ckpt, desc.ckpt_cap = ckpt.data_ptr(), ckpt.shape[1]
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())   # noqa: E731
    rc = capi.lib().ionode_tangent_sweep(C.byref(desc), ptr(params), ptr(cfg["prot_v"]), ptr(cfg["prot_t"]), ptr(cfg["prot_of_traj"]),
                                         ptr(cfg["t_eval"]), ptr(n_acc), ptr(di_dp), ptr(jtr), ptr(jtj),
                                         C.c_void_p(torch.cuda.current_stream(params.device).cuda_stream))
    if rc != 0:
        raise capi.IonodeError(f"ionode_tangent_sweep failed ({rc}): {capi.lib().ionode_grad_last_error().decode()}")


def current_s1(model, params, prot_v, y0, t_eval, *, prot_t=None, prot_t0=0.0, prot_dt=1.0, prot_of_traj=None, obs_g=1.0, obs_e=-86.0,
               obs_open_state_only=False, rtol=1e-7, atol=1e-9, v_oob=-80.0, max_steps=0, max_total_steps=0, max_step=0.0, ckpt_cap=None,
               ckpt_budget_bytes=None):
    """The current trace and its sensitivities to the rate parameters: PINTS simulateS1 over a batch.

    params [B, 8 | 12] fp64, y0 [B, D] fp32 | fp64 (the state dtype), prot_v [P, Np], t_eval [Nt] (any increasing grid) -- device
    tensors.  Keywords (prot_t, prot_t0, prot_dt, prot_of_traj, obs_g, obs_e, obs_open_state_only, rtol, atol, v_oob, max_steps,
    max_total_steps, max_step, ckpt_cap, ckpt_budget_bytes) as grad.sum_of_squares, max_step="auto" included.
    Returns (i [B, Nt] fp64, di_dp [B, Nt, NPAR] fp64, status [B] int32): i_k = obs_g gate(y_k) (V(t_k) - obs_e), bit for bit
    batched.solve(current=True)'s; di_dp[b, k, j] = di_k/dp_j, the exact derivative of the discretisation the forward executed (fp64
    tangents whatever the state dtype); row k = 0 (y0) is zero.  Failed trajectories (status != 0): NaN-filled i, zero di_dp rows.
    Memory: the states and the two traces, the checkpoints (sized, regrown and bounded by ckpt_cap / ckpt_budget_bytes as grad.solve).
    Not differentiable further; no optimiser, no y0 sensitivities, no NN models (module docstring)."""
    kw = dict(prot_t=prot_t, prot_t0=prot_t0, prot_dt=prot_dt, prot_of_traj=prot_of_traj, obs_g=obs_g, obs_e=obs_e,
              obs_open_state_only=obs_open_state_only, rtol=rtol, atol=atol, v_oob=v_oob, max_steps=max_steps, max_total_steps=max_total_steps,
              max_step=max_step, ckpt_cap=ckpt_cap, ckpt_budget_bytes=ckpt_budget_bytes)
    kw = _checked("sensitivity.current_s1", model, params, prot_v, y0, kw)
    fkw = dict(current=True, obs_g=float(kw["obs_g"]), obs_e=float(kw["obs_e"]), obs_open_state_only=bool(kw["obs_open_state_only"]))
    r, cfg, p, ckpt, n_acc = _forward(model, params, prot_v, y0, t_eval, kw, forward_kw=fkw)
    B, Nt = y0.shape[0], t_eval.shape[0]
    di_dp = torch.empty((B, Nt, capi.n_params(model)), dtype=torch.float64, device=y0.device)
    _sweep(r, cfg, p, ckpt, n_acc, di_dp, None, None)
    return r["i"], di_dp, r["status"]


def gauss_newton(model, params, prot_v, y0, t_eval, sse_ref, *, prot_t=None, prot_t0=0.0, prot_dt=1.0, prot_of_traj=None, obs_g=1.0, obs_e=-86.0,
                 obs_open_state_only=False, rtol=1e-7, atol=1e-9, v_oob=-80.0, max_steps=0, max_total_steps=0, max_step=0.0, ckpt_cap=None,
                 ckpt_budget_bytes=None):
    """The sum of squares with its Gauss-Newton terms, nothing of size [B, Nt] allocated.

    Arguments as current_s1, plus sse_ref [P, Nt] fp64: the reference currents.  Returns (sse [B], jtr [B, NPAR],
    jtj [B, NPAR, NPAR], status [B]) with r_k = i_k - sse_ref[protocol(b)][k] and J[k, j] = di_k/dp_j: sse = sum_k r_k^2 is the fused
    forward's own sum (batched.solve(sse_ref=..., states=False), bit for bit; inf where the solve failed), jtr = J^T r, jtj = J^T J
    (full, exactly symmetric).  The gradient of sse is 2 jtr, its Gauss-Newton Hessian 2 jtj.  Failed trajectories: zero jtr, jtj.
    The sums and current_s1's trace come from one per-sample device routine and differ by summation order only.
    The output grid must be uniform (the fused forward's output cursor, the rule of grad.sum_of_squares); for any other t_eval use
    sensitivity.current_s1 and contract the trace in torch.  The Levenberg-Marquardt driver on these sums: fit.levenberg_marquardt."""
    kw = dict(prot_t=prot_t, prot_t0=prot_t0, prot_dt=prot_dt, prot_of_traj=prot_of_traj, obs_g=obs_g, obs_e=obs_e,
              obs_open_state_only=obs_open_state_only, rtol=rtol, atol=atol, v_oob=v_oob, max_steps=max_steps, max_total_steps=max_total_steps,
              max_step=max_step, ckpt_cap=ckpt_cap, ckpt_budget_bytes=ckpt_budget_bytes)
    kw = _checked("sensitivity.gauss_newton", model, params, prot_v, y0, kw)
    hint = grad.uniform_grid_hint(t_eval)
    if hint is None:
        raise capi.IonodeError("sensitivity.gauss_newton needs a uniform output grid t_eval (the fused objective's output cursor); for "
                               "other grids use sensitivity.current_s1 and form the sums over its trace in torch")
    r, cfg, p, ckpt, n_acc = _forward(model, params, prot_v, y0, t_eval, kw, sse_ref=sse_ref, objective="sse", t_eval_hint=hint)
    B, npar = y0.shape[0], capi.n_params(model)
    jtr = torch.empty((B, npar), dtype=torch.float64, device=y0.device)
    jtj = torch.empty((B, npar, npar), dtype=torch.float64, device=y0.device)
    _sweep(r, cfg, p, ckpt, n_acc, None, jtr, jtj)
    return r["sse"], jtr, jtj, r["status"]
