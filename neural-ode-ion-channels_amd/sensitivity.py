"""Forward sensitivities of the current trace and their Gauss-Newton sums (closed-form HH 2-state and 6-state models, and -- with
their weights -- NN-f and NN-d).

Reference interface: PINTS `ForwardModelS1.simulateS1` -- the output AND its per-sample sensitivities dI(t_k)/dp_j -- the third of
the three PINTS evaluations behind the reference's fits (train-d0.py:508-540: SumOfSquaresError under a LogTransformation);
`batched.solve` / its fused `sse` are `simulate` / `SumOfSquaresError.__call__`, `grad.sum_of_squares` is `evaluateS1`.  The Jacobian
J[k, j] = di_k/dp_j is what Gauss-Newton / Levenberg-Marquardt steps (J^T J, J^T r), Fisher information and protocol design need; the
reverse sweep yields one row of J^T per launch, finite differences NPAR + 1 solves and half the digits.

What is computed: the tangent-mode derivative of the discretisation the forward launch executed (accepted steps as constants,
csrc/ionode_tangent.hpp) -- the same rule as grad.py's reverse mode, so 2 J^T r here equals the gradient of grad.sum_of_squares.
Two launches: the checkpointed forward (capi.dopri5, sized and regrown by grad._forward_with_checkpoints) and ionode_tangent_sweep.
Plain evaluations: no autograd graph is built, and there is no CPU fallback.

NN models (NN-f, NN-d; `weights`, mlp_layers, mlp_width: one weight set, every width the backward sweep serves): the state the net sees is
one scalar, so its Jacobian-vector product is a multiplication by d net / d a -- which grad.py's two-phase reverse sweep already
computes per (trajectory, accepted step, stage) into its packets.  Their route is the checkpointed forward, then per chunk of
iterations ionode_tangent_sweep_nn: the reverse sweep's recompute kernel without an output gradient, and a tangent walk over its packets
forward in time (csrc/ionode_tangent_nn.hpp), chunked by grad.plan_backward_chunks inside grad.py's memory budget.  What is served for
them: dI/dp for the 8 rate parameters (NN-f: p5..p8; its columns p1..p4 are exactly zero).  Not served: an NN model without weights
(refused as before), a weight set per candidate, dL/dW by forward mode (grad.py's reverse sweep has it).

The optimiser is not here: fit.py's Levenberg-Marquardt driver builds on gauss_newton.  Out of scope: sensitivities with respect to y0 and to the
weights, and an absolute-error variant of the sums.
"""
import ctypes as C

import numpy as np
import torch

from . import capi, grad


class _Saved:
    """What grad._forward_with_checkpoints leaves on an autograd context, kept on a plain object: (params, ckpt, stats, status)."""

    def save_for_backward(self, *tensors):
        self.saved_tensors = tensors

    def mark_non_differentiable(self, *tensors):
        pass


def nn_route(who, model, weights, mlp_layers, mlp_width, free=None):
    """The one rule for an NN model in everything built on the tangent sweep (this module, objective.population_gauss_newton / _fit /
    _mala, fit.levenberg_marquardt, mala.sample).  Returns the keywords to hand on: {} for a closed-form model,
    dict(weights, mlp_layers, mlp_width) for NN-f / NN-d with one weight set.  Refused: an NN model without weights (as before the NN
    route existed), a weight population [C, n] (the sweep differentiates one weight set), weights for a closed-form model, and --
    `free` given -- NN-f with a free index below 4 (NN-f has no p1..p4: those columns are identically zero, J^T J would be singular)."""
    if model not in (capi.MODEL_NNF, capi.MODEL_NND):
        if weights is not None:
            raise capi.IonodeError(f"{who}: the closed-form models have no MLP: pass weights=None")
        return {}
    if weights is None:
        raise capi.IonodeError(f"{who}: without weights only the closed-form HH 2-state and 6-state models are served; NN-f / NN-d need "
                               "`weights`, mlp_layers and mlp_width (one shared weight set, as objective.population_cmaes / "
                               "population_mcmc take them)")
    if np.ndim(weights) != 1:
        raise capi.IonodeError(f"{who}: weights [C, n] (a weight set per candidate) are not served: the tangent sweep differentiates one "
                               "weight set; pass one flat state dict [n]")
    if model == capi.MODEL_NNF and free is not None and any(int(f) < 4 for f in free):
        raise capi.IonodeError(f"{who}: NN-f has no p1..p4 (the net replaces the a gate): free = {tuple(int(f) for f in free)} holds an "
                               "index below 4, whose columns of the Jacobian are identically zero (J^T J would be singular)")
    if int(mlp_layers) < 1 or int(mlp_width) < 1:
        raise capi.IonodeError(f"{who}: an NN model needs mlp_layers >= 1 and mlp_width >= 1")
    return dict(weights=weights, mlp_layers=int(mlp_layers), mlp_width=int(mlp_width))


def _checked(who, model, params, prot_v, y0, kw, weights=None, mlp_layers=0, mlp_width=0):
    """The argument checks both entry points share; returns the keywords with max_step resolved."""
    if model not in (capi.MODEL_HH2, capi.MODEL_MARKOV6, capi.MODEL_NNF, capi.MODEL_NND):
        raise NotImplementedError("unknown model")
    nn_route(who, model, weights, mlp_layers, mlp_width)
    D, npar = capi.n_state(model), capi.n_params(model)
    if not (isinstance(y0, torch.Tensor) and isinstance(params, torch.Tensor)) or y0.dim() != 2 or y0.shape[1] != D or params.dim() != 2 \
            or params.shape[0] != y0.shape[0] or params.shape[1] != npar:
        raise capi.IonodeError(f"params [B, {npar}] and y0 [B, {D}] expected")
    if not y0.is_cuda:
        raise capi.IonodeError("no HIP tensors: the integrator and its tangent sweep have no CPU path")
    kw["max_step"] = grad._resolve_max_step(model, params.detach(), prot_v, kw["v_oob"], kw["max_step"], frames=3)
    return kw


def _forward(model, params, prot_v, y0, t_eval, kw, nn=None, **cfg_extra):
    """The checkpointed forward with grad.py's sizing / regrow / budget logic.  nn: an NN model's (weights, mlp_layers, mlp_width,
    weights_key, record_budget_bytes, chunk_iters).  Returns (capi.dopri5's result, cfg, params, checkpoints, n_accepted [B] int32 with
    failed trajectories zeroed); cfg["w_np"]: the weights as grad.py keeps them, a flat fp32 numpy array, or None."""
    pot = kw["prot_of_traj"]
    weights, L, N, wkey, rbudget, chunk_iters = nn if nn is not None else (None, 0, 0, None, None, None)
    if weights is not None:
        weights = weights.detach() if isinstance(weights, torch.Tensor) else \
            torch.from_numpy(np.ascontiguousarray(np.asarray(weights, dtype=np.float32)))
    cfg = dict(model=model, mlp_layers=int(L), mlp_width=int(N), weights_key=wkey, record_budget_bytes=rbudget, chunk_iters=chunk_iters,
               prot_v=prot_v, prot_t=kw["prot_t"], prot_t0=float(kw["prot_t0"]),
               prot_dt=float(kw["prot_dt"]), t_eval=t_eval,
               prot_of_traj=None if pot is None else torch.as_tensor(pot, device=y0.device).to(torch.int32).contiguous(),
               rtol=float(kw["rtol"]), atol=float(kw["atol"]), v_oob=float(kw["v_oob"]), max_steps=int(kw["max_steps"]),
               max_total_steps=int(kw["max_total_steps"]), max_step=float(kw["max_step"]), obs_g=float(kw["obs_g"]),
               obs_e=float(kw["obs_e"]), obs_open_state_only=bool(kw["obs_open_state_only"]), ckpt_cap=kw["ckpt_cap"],
               ckpt_budget_bytes=kw["ckpt_budget_bytes"], **cfg_extra)
    ctx = _Saved()
    with torch.no_grad():
        r = grad._forward_with_checkpoints(ctx, weights, params.detach().contiguous(), y0.detach().contiguous(), cfg, objective="sse_ref" in cfg)
    p, ckpt, stats, status = ctx.saved_tensors
    n_acc = torch.where(status != 0, torch.zeros_like(stats[:, 0]), stats[:, 0]).to(torch.int32).contiguous()
    cfg["w_np"] = ctx.w_np
    return r, cfg, p, ckpt, n_acc


def nn_chunks(n_iter, tiles, packet_doubles, budget, chunk_iters=None):
    """The NN route's launches over the sweep's n_iter iterations, in call order: [it0, it1) ranges from [n_iter - c, n_iter) down to
    [0, c) -- forward in time is descending iterations -- and c, the iterations one packet buffer holds.  c is
    grad.plan_backward_chunks' two-phase chunk without weight gradients (packets inside half the budget, at most 256 iterations),
    or chunk_iters (tests, measurements), inside HIP's grid.y limit for the recompute kernel either way.  Pure arithmetic."""
    chunk, _n_buf, _bounds = grad.plan_backward_chunks(n_iter, tiles, 0, packet_doubles, budget, False, True)
    if chunk_iters:
        chunk = max(1, min(int(chunk_iters), n_iter, grad.MAX_RECOMPUTE_ITERS))
    hi = list(range(n_iter, 0, -chunk))
    return chunk, [(max(0, h - chunk), h) for h in hi]


def _sweep_nn(r, cfg, params, ckpt, n_acc, di_dp, jtr, jtj):
    """The chunk loop of ionode_tangent_sweep_nn on the current stream: per chunk the recompute kernel fills `packets` and the tangent
    walk consumes them; `state` carries the tangents and the running sums from launch to launch."""
    desc = r["desc"]
    desc.ckpt, desc.ckpt_cap = ckpt.data_ptr(), ckpt.shape[1]
    dev, lib = params.device, capi.lib()
    L, N, B = cfg["mlp_layers"], cfg["mlp_width"], desc.n_traj
    n_iter = int(n_acc.max().item()) + 1
    image = grad.grad_image(cfg["w_np"], L, N, dev, key=cfg.get("weights_key"))
    tiles, pkd = (B + 15) // 16, int(lib.ionode_grad_packet_doubles())
    budget = grad._bounded_budget(cfg.get("record_budget_bytes"), grad.DEFAULT_RECORD_BUDGET, dev, 0.5)
    chunk, bounds = nn_chunks(n_iter, tiles, pkd, budget, cfg.get("chunk_iters"))
    packets = torch.empty(tiles * chunk * pkd, dtype=torch.float64, device=dev)
    state = torch.empty((B, int(lib.ionode_tangent_nn_state_doubles())), dtype=torch.float64, device=dev)
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())   # noqa: E731
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    for it0, it1 in bounds:
        rc = lib.ionode_tangent_sweep_nn(C.byref(desc), it0, it1, n_iter, ptr(image), ptr(params), ptr(cfg["prot_v"]), ptr(cfg["prot_t"]),
                                         ptr(cfg["prot_of_traj"]), ptr(cfg["t_eval"]), ptr(n_acc), ptr(packets), ptr(state), ptr(di_dp),
                                         ptr(jtr), ptr(jtj), stream)
        if rc != 0:
            raise capi.IonodeError(f"ionode_tangent_sweep_nn failed ({rc}): {lib.ionode_grad_last_error().decode()}")


def _sweep(r, cfg, params, ckpt, n_acc, di_dp, jtr, jtj):
    """ionode_tangent_sweep on the current stream, with the descriptor of the forward that wrote `ckpt`; NN models (cfg["w_np"]): _sweep_nn."""
    if cfg.get("w_np") is not None:
        return _sweep_nn(r, cfg, params, ckpt, n_acc, di_dp, jtr, jtj)
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
               ckpt_budget_bytes=None, weights=None, mlp_layers=0, mlp_width=0, weights_key=None, record_budget_bytes=None, chunk_iters=None):
    """The current trace and its sensitivities to the rate parameters: PINTS simulateS1 over a batch.

    params [B, 8 | 12] fp64, y0 [B, D] fp32 | fp64 (the state dtype), prot_v [P, Np], t_eval [Nt] (any increasing grid) -- device
    tensors.  Keywords (prot_t, prot_t0, prot_dt, prot_of_traj, obs_g, obs_e, obs_open_state_only, rtol, atol, v_oob, max_steps,
    max_total_steps, max_step, ckpt_cap, ckpt_budget_bytes) as grad.sum_of_squares, max_step="auto" included.
    Returns (i [B, Nt] fp64, di_dp [B, Nt, NPAR] fp64, status [B] int32): i_k = obs_g gate(y_k) (V(t_k) - obs_e), bit for bit
    batched.solve(current=True)'s; di_dp[b, k, j] = di_k/dp_j, the exact derivative of the discretisation the forward executed (fp64
    tangents whatever the state dtype); row k = 0 (y0) is zero.  Failed trajectories (status != 0): NaN-filled i, zero di_dp rows.
    Memory: the states and the two traces, the checkpoints (sized, regrown and bounded by ckpt_cap / ckpt_budget_bytes as grad.solve).
    NN models (NN-f, NN-d) run with weights [n] fp32 (the reference's flat state dict: a tensor or an array), mlp_layers and mlp_width
    (weights_key: the weight images' cache key, as grad.solve's); without weights they are refused.  params [B, 8], y0 [B, 2]; NN-f's
    columns p1..p4 are exactly zero.  Their sweep is chunked over iterations (module docstring): record_budget_bytes bounds the
    chunk's packets as in grad.solve, chunk_iters (tests, measurements) sets the iterations per launch; the result has the same bits
    for any chunking.  Not differentiable further; no optimiser, no y0 sensitivities, no weight sensitivities (module docstring)."""
    kw = dict(prot_t=prot_t, prot_t0=prot_t0, prot_dt=prot_dt, prot_of_traj=prot_of_traj, obs_g=obs_g, obs_e=obs_e,
              obs_open_state_only=obs_open_state_only, rtol=rtol, atol=atol, v_oob=v_oob, max_steps=max_steps, max_total_steps=max_total_steps,
              max_step=max_step, ckpt_cap=ckpt_cap, ckpt_budget_bytes=ckpt_budget_bytes)
    kw = _checked("sensitivity.current_s1", model, params, prot_v, y0, kw, weights, mlp_layers, mlp_width)
    fkw = dict(current=True, obs_g=float(kw["obs_g"]), obs_e=float(kw["obs_e"]), obs_open_state_only=bool(kw["obs_open_state_only"]))
    r, cfg, p, ckpt, n_acc = _forward(model, params, prot_v, y0, t_eval, kw, forward_kw=fkw,
                                      nn=(weights, mlp_layers, mlp_width, weights_key, record_budget_bytes, chunk_iters))
    B, Nt = y0.shape[0], t_eval.shape[0]
    di_dp = torch.empty((B, Nt, capi.n_params(model)), dtype=torch.float64, device=y0.device)
    _sweep(r, cfg, p, ckpt, n_acc, di_dp, None, None)
    return r["i"], di_dp, r["status"]


def gauss_newton(model, params, prot_v, y0, t_eval, sse_ref, *, prot_t=None, prot_t0=0.0, prot_dt=1.0, prot_of_traj=None, obs_g=1.0, obs_e=-86.0,
                 obs_open_state_only=False, rtol=1e-7, atol=1e-9, v_oob=-80.0, max_steps=0, max_total_steps=0, max_step=0.0, ckpt_cap=None,
                 ckpt_budget_bytes=None, weights=None, mlp_layers=0, mlp_width=0, weights_key=None, record_budget_bytes=None, chunk_iters=None):
    """The sum of squares with its Gauss-Newton terms, nothing of size [B, Nt] allocated.

    Arguments as current_s1, plus sse_ref [P, Nt] fp64: the reference currents.  Returns (sse [B], jtr [B, NPAR],
    jtj [B, NPAR, NPAR], status [B]) with r_k = i_k - sse_ref[protocol(b)][k] and J[k, j] = di_k/dp_j: sse = sum_k r_k^2 is the fused
    forward's own sum (batched.solve(sse_ref=..., states=False), bit for bit; inf where the solve failed), jtr = J^T r, jtj = J^T J
    (full, exactly symmetric).  The gradient of sse is 2 jtr, its Gauss-Newton Hessian 2 jtj.  Failed trajectories: zero jtr, jtj.
    The sums and current_s1's trace come from one per-sample device routine and differ by summation order only.
    The output grid must be uniform (the fused forward's output cursor, the rule of grad.sum_of_squares); for any other t_eval use
    sensitivity.current_s1 and contract the trace in torch.  The Levenberg-Marquardt driver on these sums: fit.levenberg_marquardt.
    NN models: weights, mlp_layers, mlp_width, weights_key, record_budget_bytes and chunk_iters as current_s1; beside the checkpoints
    the route holds one chunk's packets and O(B), nothing of size [B, Nt]."""
    kw = dict(prot_t=prot_t, prot_t0=prot_t0, prot_dt=prot_dt, prot_of_traj=prot_of_traj, obs_g=obs_g, obs_e=obs_e,
              obs_open_state_only=obs_open_state_only, rtol=rtol, atol=atol, v_oob=v_oob, max_steps=max_steps, max_total_steps=max_total_steps,
              max_step=max_step, ckpt_cap=ckpt_cap, ckpt_budget_bytes=ckpt_budget_bytes)
    kw = _checked("sensitivity.gauss_newton", model, params, prot_v, y0, kw, weights, mlp_layers, mlp_width)
    hint = grad.uniform_grid_hint(t_eval)
    if hint is None:
        raise capi.IonodeError("sensitivity.gauss_newton needs a uniform output grid t_eval (the fused objective's output cursor); for "
                               "other grids use sensitivity.current_s1 and form the sums over its trace in torch")
    r, cfg, p, ckpt, n_acc = _forward(model, params, prot_v, y0, t_eval, kw, sse_ref=sse_ref, objective="sse", t_eval_hint=hint,
                                      nn=(weights, mlp_layers, mlp_width, weights_key, record_budget_bytes, chunk_iters))
    B, npar = y0.shape[0], capi.n_params(model)
    jtr = torch.empty((B, npar), dtype=torch.float64, device=y0.device)
    jtj = torch.empty((B, npar, npar), dtype=torch.float64, device=y0.device)
    _sweep(r, cfg, p, ckpt, n_acc, None, jtr, jtj)
    return r["sse"], jtr, jtj, r["status"]
