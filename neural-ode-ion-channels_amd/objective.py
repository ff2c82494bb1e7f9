"""Batched candidate-model objective: the consumer of the batched solve that replaces the reference's
PINTS `ForwardModel.simulate` + `SumOfSquaresError` + process pool (train-d0.py:377-439, :508-540).

The reference evaluates ONE candidate at a time: for each protocol, `odeint(ODEFunc(p1..p4 = x), y0, t)`, current
`o[:,0,0]*o[:,0,1]*(V+86)`, and a SIGALRM time limit that turns a stuck solve into an `inf` error vector
(train-d0.py:426-438).  Here a whole CMA-ES population is one launch: C candidates x P protocols = C*P trajectories,
per-trajectory rate parameters, the current trace fused into the dense output, failed solves -> inf.  With several GPUs
the candidates are sharded contiguously and the per-candidate errors are all-gathered (the optimiser needs every
candidate's value on every rank); a scalar loss needs only `distributed.allreduce_sum_count`.
"""
import numpy as np
import torch

from . import batched, capi, distributed, grad


def _auto_max_step(max_step, model, rows, protocols_v):
    """max_step as a number: "auto" is resolved ONCE, before sharding, to grad.stable_step_cap over rows() [*, NPAR] -- the parameter
    rows the caller caps over: every candidate, or the stiffest corner of the box (_corner_or_starts) -- so that the function being
    evaluated is the same on every rank and in every iteration.  Non-finite rows are left out (they fail either way and must not void
    everyone's cap); 0.0 (no cap) when none remains, and for the NN models, which carry no such cap."""
    if not isinstance(max_step, str):
        return max_step
    if max_step != "auto":
        raise capi.IonodeError("max_step must be a number (ms) or 'auto'")
    if model in (capi.MODEL_NNF, capi.MODEL_NND):
        return 0.0
    rows = rows()
    fin = np.isfinite(rows).all(axis=1)
    if not fin.any():
        return 0.0
    return grad.stable_step_cap(model, torch.from_numpy(rows[fin]), torch.as_tensor(np.asarray(protocols_v, dtype=np.float64)))


def _corner_or_starts(base, free, bounds, starts):
    """The rows a fit's "auto" step cap is taken over: the upper corner of the box -- the stiffest point the fit can visit -- when the
    upper bounds are finite, else the starting population."""
    rows = np.tile(base, (starts.shape[0], 1))
    if bounds is not None and np.isfinite(np.asarray(bounds[1], dtype=np.float64)).all():
        rows = rows[:1]
        rows[:, free] = np.asarray(bounds[1], dtype=np.float64)
    else:
        rows[:, free] = starts
    return rows


def population_sum_of_squares(candidates, protocols_v, data_i, t_eval, *, base_params, free=(0, 1, 2, 3), prot_t0=0.0,
                              prot_dt=0.1, y0=(0.0, 1.0), state_dtype=torch.float32, obs_g=1.0, obs_e=-86.0,
                              max_total_steps=1_000_000, group=None, device=None, solver=None, fused=True, cost=None,
                              model=capi.MODEL_HH2, weights=None, mlp_layers=0, mlp_width=0, weights_key=None):
    """Sum-of-squares error of every candidate over all protocols (PINTS SumOfSquaresError on a multi-output problem).

    candidates  [C, len(free)]  values of the free rate parameters (train-d0.py: p1..p4 -> free = (0, 1, 2, 3))
    protocols_v [P, Np] mV;  data_i [P, Nt] measured currents;  t_eval [Nt] ms;  base_params [8]
    Returns a [C] fp64 tensor on the device: inf where any of a candidate's solves failed (the reference's time-limit
    rule).  Under torch.distributed the candidates are sharded over the ranks and the result is all-gathered.
    fused (default): the squared residuals are accumulated inside the kernel (ionode_desc.sse_ref / sse_out) and neither states
    nor current traces are written -- the only way BASELINE configs[3] fits (65 536 candidates x 32 sweeps x 1e5 samples would be
    4.5 TB of traces); fused=False stores the traces and reduces them with torch (same values to ~1e-13, for tests).
    model / weights / mlp_layers / mlp_width: the candidate model -- HH 2-state by default (train-d0.py), or NN-f / NN-d with one
    shared set of MLP weights and per-candidate rate parameters (free = (4, 5, 6, 7) for NN-f's p5..p8); weights [C, n]: a
    population of nets, candidate c integrated with its own weight set (free may then be empty: candidates [C, 0]).
    cost (optional, [C]): predicted cost per candidate (e.g. the previous generation's step counts): the candidates are then
    cut into contiguous shards of equal cost rather than equal count (distributed.shard_bounds_by_cost).
    `solver` (tests only): a stand-in with batched.solve's signature, so the sharding / all-gather logic can run under
    gloo on a box without a GPU; the product default is the HIP solve and there is no CPU fallback.
    """
    return _population_error("sse", False, candidates, protocols_v, data_i, t_eval, base_params=base_params, free=free, prot_t0=prot_t0,
                             prot_dt=prot_dt, y0=y0, state_dtype=state_dtype, obs_g=obs_g, obs_e=obs_e, max_total_steps=max_total_steps,
                             group=group, device=device, solver=solver, fused=fused, cost=cost, model=model, weights=weights,
                             mlp_layers=mlp_layers, mlp_width=mlp_width, weights_key=weights_key)


def population_mean_abs_error(candidates, protocols_v, data_i, t_eval, *, base_params, free=(0, 1, 2, 3), prot_t0=0.0,
                              prot_dt=0.1, y0=(0.0, 1.0), state_dtype=torch.float32, obs_g=1.0, obs_e=-86.0,
                              max_total_steps=1_000_000, group=None, device=None, solver=None, fused=True, cost=None,
                              model=capi.MODEL_HH2, weights=None, mlp_layers=0, mlp_width=0, weights_key=None, per_protocol=False):
    """Mean absolute error of every candidate: the reference's prediction loss torch.mean(torch.abs(pred_yo - data)) (every --pred
    section, train-s1.py:275-353; the validation that picks the best checkpoint, train-r1.py:930-959), for a whole population.

    The sibling of population_sum_of_squares: same arguments, sharding, padding for weights [C, n], all-gather and `solver`
    stand-in.  Returns a [C] fp64 tensor on the device, the mean of |i - data| over the candidate's P * Nt samples; inf where any
    of the candidate's solves failed.  per_protocol=True: [C, P], the mean over each protocol's Nt samples (the reference sums
    per-protocol means when it ranks checkpoints, train-r1.py:953); a candidate with a failed solve is inf in every column.
    fused (default): the absolute residuals are accumulated inside the kernel (capi.dopri5(objective="sae")) and no trace is
    written; fused=False stores the current traces and reduces them with torch (for tests).  A `solver` stand-in serves either
    route: its Solution carries .sae [B] for the fused one, .i [B, Nt] for the other.
    """
    return _population_error("sae", per_protocol, candidates, protocols_v, data_i, t_eval, base_params=base_params, free=free,
                             prot_t0=prot_t0, prot_dt=prot_dt, y0=y0, state_dtype=state_dtype, obs_g=obs_g, obs_e=obs_e,
                             max_total_steps=max_total_steps, group=group, device=device, solver=solver, fused=fused, cost=cost,
                             model=model, weights=weights, mlp_layers=mlp_layers, mlp_width=mlp_width, weights_key=weights_key)


def _population_error(kind, per_protocol, candidates, protocols_v, data_i, t_eval, *, base_params, free, prot_t0, prot_dt, y0,
                      state_dtype, obs_g, obs_e, max_total_steps, group, device, solver, fused, cost, model, weights, mlp_layers,
                      mlp_width, weights_key):
    """The one body of population_sum_of_squares (kind "sse": [C] sums) and population_mean_abs_error (kind "sae": [C] means, or
    [C, P] per-protocol means): shard the candidates, solve, reduce each candidate's P sweeps, all-gather."""
    cand = np.asarray(candidates, dtype=np.float64)
    C, P = cand.shape[0], np.asarray(protocols_v).shape[0]
    rank, world, bounds = distributed.population_shards(C, cost, group, "candidates")
    lo, hi = bounds[rank]
    dev = batched._dev(device) if solver is None else torch.device(device or "cpu")
    solve = batched.solve if solver is None else solver
    mlp = {} if weights is None else dict(weights=weights, mlp_layers=mlp_layers, mlp_width=mlp_width, weights_key=weights_key)
    # a population of NETS: weights [C, n] -- candidate c has its own MLP weights (and its rate parameters).  Every candidate then
    # owns whole 16-trajectory tiles (ionode_desc.traj_per_image): its P sweeps are padded to a multiple of 16 with repeats of
    # sweep 0 whose scores are dropped.
    per_cand = weights is not None and np.asarray(weights).ndim == 2
    S = P
    if per_cand:
        if np.asarray(weights).shape[0] != C:
            raise capi.IonodeError("weights [C, n]: one weight set per candidate")
        S = 16 * ((P + 15) // 16)
        mlp.update(weights=np.asarray(weights)[lo:hi], traj_per_image=S, weights_key=None)
    cols = (P,) if per_protocol else ()
    out = torch.full((hi - lo,) + cols, float("inf"), dtype=torch.float64, device=dev)
    if hi > lo:
        params = np.tile(np.asarray(base_params, dtype=np.float64), (hi - lo, 1))
        params[:, list(free)] = cand[lo:hi]
        params = np.repeat(params, S, axis=0)                       # candidate-major: trajectory = c*S + p
        pot = np.tile(np.where(np.arange(S) < P, np.arange(S), 0).astype(np.int32), hi - lo)
        ref = torch.as_tensor(np.asarray(data_i), dtype=torch.float64, device=dev)     # [P, Nt]
        # (the squares' stand-ins return traces only, so a stand-in takes the fused route for the absolute values alone)
        if fused and (solver is None or kind == "sae"):
            sol = solve(model, params, protocols_v, torch.tensor([list(y0)], dtype=state_dtype), t_eval,
                        prot_t0=prot_t0, prot_dt=prot_dt, prot_of_traj=pot, obs_g=obs_g, obs_e=obs_e,
                        max_total_steps=max_total_steps, device=dev, sse_ref=ref.contiguous(), states=False,
                        **({} if kind == "sse" else {"objective": kind}), **mlp)
            per = getattr(sol, kind).reshape(hi - lo, S)[:, :P]     # failed solves are inf already
        else:
            sol = solve(model, params, protocols_v, torch.tensor([list(y0)], dtype=state_dtype), t_eval,
                        prot_t0=prot_t0, prot_dt=prot_dt, prot_of_traj=pot, current=True, obs_g=obs_g, obs_e=obs_e,
                        max_total_steps=max_total_steps, device=dev, **mlp)
            res = sol.i.reshape(hi - lo, S, -1)[:, :P] - ref[None]
            per = None if kind == "sse" else res.abs().sum(dim=2)
        if kind == "sse":
            err = per.sum(dim=1) if per is not None else (res ** 2).sum(dim=(1, 2))
        else:
            Nt = ref.shape[1]
            err = per / Nt if per_protocol else per.sum(dim=1) / (P * Nt)
        ok = (sol.status.reshape(hi - lo, S)[:, :P] == 0).all(dim=1)
        out = torch.where(ok[:, None] if per_protocol else ok, err, torch.full_like(err, float("inf")))
    return distributed.all_gather_shards(out, bounds, rank, group)   # (unequal shards: padded to the largest)


def population_sum_of_squares_s1(candidates, protocols_v, data_i, t_eval, *, base_params, free=(0, 1, 2, 3), prot_t0=0.0,
                                 prot_dt=0.1, y0=(0.0, 1.0), state_dtype=torch.float32, obs_g=1.0, obs_e=-86.0,
                                 obs_open_state_only=False, max_total_steps=1_000_000, max_step="auto", group=None, device=None,
                                 solver=None, cost=None, model=capi.MODEL_HH2):
    """Sum-of-squares error of every candidate AND its gradient with respect to the free parameters: the evaluateS1 counterpart
    of population_sum_of_squares (PINTS SumOfSquaresError.evaluateS1, what PINTS' gradient-based optimisers call).

    Arguments as population_sum_of_squares; model: HH 2-state (default, base_params [8]) or the 6-state model (base_params [12],
    y0 of 6 states; obs_open_state_only=True observes the open state as train-d1.py:299).  Returns (sse [C] fp64,
    dsse [C, len(free)] fp64) on the device; dsse[c, j] = d sse[c] / d candidates[c, j], the sum over the candidate's protocols of
    the free columns of dL/dp (grad.sum_of_squares: fused forward + fused backward, no trace of size [C * P, Nt] is written).
    A candidate any of whose solves failed gets sse = inf and a ZERO gradient row (the solve has no derivative there; an optimiser
    that only compares values rejects it anyway).
    max_step ("auto" by default: gradients through an uncapped solve are meaningless at equilibria, grad.solve): the "auto" cap
    is grad.stable_step_cap over the WHOLE population (its finite candidates), computed before sharding -- a per-shard cap would
    make every candidate's value depend on the world size.  Sharding as population_sum_of_squares (contiguous, or equal cost with `cost`); one
    all-gather carries [C, 1 + len(free)].  `solver` (tests only): a stand-in with grad.sum_of_squares' signature, returning a
    differentiable (sse, status), so the sharding / all-gather logic can run under gloo without a GPU.
    """
    return _population_error_s1("sse", candidates, protocols_v, data_i, t_eval, base_params=base_params, free=free, prot_t0=prot_t0,
                                prot_dt=prot_dt, y0=y0, state_dtype=state_dtype, obs_g=obs_g, obs_e=obs_e,
                                obs_open_state_only=obs_open_state_only, max_total_steps=max_total_steps, max_step=max_step, group=group,
                                device=device, solver=solver, cost=cost, model=model)


def population_mean_abs_error_s1(candidates, protocols_v, data_i, t_eval, *, base_params, free=(0, 1, 2, 3), prot_t0=0.0,
                                 prot_dt=0.1, y0=(0.0, 1.0), state_dtype=torch.float32, obs_g=1.0, obs_e=-86.0,
                                 obs_open_state_only=False, max_total_steps=1_000_000, max_step="auto", group=None, device=None,
                                 solver=None, cost=None, model=capi.MODEL_HH2):
    """Mean absolute error of every candidate AND its gradient with respect to the free parameters: the reference's loss
    torch.mean(torch.abs(pred_yo - data)) (train-s1.py:329, train-d1.py:305) differentiated through the solve, for a whole
    population -- the sibling of population_sum_of_squares_s1, as population_mean_abs_error is of population_sum_of_squares.

    Arguments, models, sharding, the population-wide "auto" step cap and the all-gather as population_sum_of_squares_s1.  Returns
    (mae [C] fp64, dmae [C, len(free)] fp64) on the device: mae[c] is the mean of |i - data| over the candidate's P * Nt samples --
    population_mean_abs_error's value -- and dmae[c, j] = d mae[c] / d candidates[c, j] (grad.sum_of_abs: fused forward + fused
    backward, sign(0) = 0, no trace of size [C * P, Nt] is written).  A candidate any of whose solves failed gets mae = inf and a ZERO
    gradient row.  `solver` (tests only): a stand-in with grad.sum_of_abs' signature, returning a differentiable (sae, status).
    """
    return _population_error_s1("sae", candidates, protocols_v, data_i, t_eval, base_params=base_params, free=free, prot_t0=prot_t0,
                                prot_dt=prot_dt, y0=y0, state_dtype=state_dtype, obs_g=obs_g, obs_e=obs_e,
                                obs_open_state_only=obs_open_state_only, max_total_steps=max_total_steps, max_step=max_step, group=group,
                                device=device, solver=solver, cost=cost, model=model)


def _population_error_s1(kind, candidates, protocols_v, data_i, t_eval, *, base_params, free, prot_t0, prot_dt, y0, state_dtype, obs_g,
                         obs_e, obs_open_state_only, max_total_steps, max_step, group, device, solver, cost, model):
    """The one body of population_sum_of_squares_s1 (kind "sse": [C] sums) and population_mean_abs_error_s1 (kind "sae": [C] means),
    each with its gradient: the population-wide step cap, shard, fused solve and sweep, reduce each candidate's P sweeps, all-gather."""
    who = "population_sum_of_squares_s1" if kind == "sse" else "population_mean_abs_error_s1"
    if model not in (capi.MODEL_HH2, capi.MODEL_MARKOV6):
        raise capi.IonodeError(f"{who}: HH 2-state and 6-state models only")
    D, npar = (6, 12) if model == capi.MODEL_MARKOV6 else (2, 8)
    free = [int(f) for f in free]
    cand = np.asarray(candidates, dtype=np.float64).reshape(-1, len(free))
    C, P = cand.shape[0], np.asarray(protocols_v).shape[0]
    base = np.asarray(base_params, dtype=np.float64)
    if base.shape != (npar,) or len(y0) != D:
        raise capi.IonodeError(f"model {model}: base_params [{npar}] and y0 of {D} states expected")
    rank, world, bounds = distributed.population_shards(C, cost, group, "candidates")
    lo, hi = bounds[rank]
    dev = batched._dev(device) if solver is None else torch.device(device or "cpu")
    solve = (grad.sum_of_squares if kind == "sse" else grad.sum_of_abs) if solver is None else solver
    params_all = np.tile(base, (C, 1))
    params_all[:, free] = cand
    max_step = _auto_max_step(max_step, model, lambda: params_all, protocols_v)
    nf = len(free)
    out = torch.empty((hi - lo, 1 + nf), dtype=torch.float64, device=dev)
    if hi > lo:
        n = hi - lo
        p = torch.from_numpy(np.repeat(params_all[lo:hi], P, axis=0)).to(dev).requires_grad_(True)   # trajectory = c * P + protocol
        pot = torch.from_numpy(np.tile(np.arange(P, dtype=np.int32), n)).to(dev)
        y0t = torch.tensor([list(y0)], dtype=state_dtype, device=dev).expand(n * P, D).contiguous()
        sse, status = solve(model, p, torch.as_tensor(np.asarray(protocols_v), dtype=torch.float64, device=dev).contiguous(), y0t,
                            torch.as_tensor(np.asarray(t_eval), dtype=torch.float64, device=dev).contiguous(),
                            torch.as_tensor(np.asarray(data_i), dtype=torch.float64, device=dev).contiguous(),
                            prot_t0=prot_t0, prot_dt=prot_dt, prot_of_traj=pot, obs_g=obs_g, obs_e=obs_e,
                            obs_open_state_only=obs_open_state_only, max_total_steps=max_total_steps, max_step=max_step)
        (gp,) = torch.autograd.grad(sse, p, grad_outputs=torch.ones_like(sse))
        ok = (status.reshape(n, P) == 0).all(dim=1)
        err = sse.detach().reshape(n, P).sum(dim=1)
        gc = gp.reshape(n, P, npar).sum(dim=1)[:, free]
        if kind == "sae":   # the mean over the candidate's P * Nt samples, and its gradient
            n_samples = P * np.asarray(data_i).shape[1]
            err, gc = err / n_samples, gc / n_samples
        out[:, 0] = torch.where(ok, err, torch.full_like(err, float("inf")))
        out[:, 1:] = torch.where(ok[:, None], gc, torch.zeros_like(gc))
    out = distributed.all_gather_shards(out, bounds, rank, group)
    return out[:, 0].contiguous(), out[:, 1:].contiguous()


def population_gauss_newton(candidates, protocols_v, data_i, t_eval, *, base_params, free=(0, 1, 2, 3), log_parameters=False, prot_t0=0.0,
                            prot_dt=0.1, y0=(0.0, 1.0), state_dtype=torch.float32, obs_g=1.0, obs_e=-86.0, obs_open_state_only=False,
                            max_total_steps=1_000_000, max_step="auto", group=None, device=None, solver=None, cost=None,
                            model=capi.MODEL_HH2, weights=None, mlp_layers=0, mlp_width=0, weights_key=None):
    """Sum-of-squares error of every candidate with its gradient AND its Gauss-Newton Hessian in the free parameters: what a
    Gauss-Newton / Levenberg-Marquardt step or a Fisher-information estimate needs, from forward sensitivities
    (sensitivity.gauss_newton: PINTS ForwardModelS1.simulateS1 contracted in the kernel, no trace of size [C * P, Nt] is written).

    Arguments, models, sharding, the population-wide "auto" step cap and the all-gather as population_sum_of_squares_s1.  Returns
    (sse [C], g [C, len(free)], H [C, len(free), len(free)]) fp64 on the device, summed over the candidate's protocols: with the
    residuals r and the Jacobian J = dr/d(free parameters), g = 2 J^T r -- population_sum_of_squares_s1's gradient by another route --
    and H = 2 J^T J.  log_parameters=True: derivatives with respect to log p_j (the reference's pints.LogTransformation,
    train-d0.py:511), g_j p_j and H_jl p_j p_l.  A candidate any of whose solves failed gets sse = inf and ZERO g and H.
    `solver` (tests only): a stand-in with sensitivity.gauss_newton's signature, so the sharding / all-gather logic can run without a
    GPU.  The optimiser built on these sums is population_fit (fit.py: Levenberg-Marquardt with the reduction, the damping, the
    step and its acceptance in one kernel); no y0 sensitivities, no absolute-error variant (sensitivity's module docstring).
    NN models (NN-f, NN-d): with weights [n] -- ONE flat state dict shared by the population --, mlp_layers, mlp_width and weights_key
    they are served through sensitivity.py's NN route, `free` indexing their 8 rate parameters (NN-f: 4..7 only: it has no p1..p4);
    max_step "auto" resolves as everywhere in this module for them: no cap.  Without weights they are refused, and so is a weight set
    per candidate, weights [C, n]: the tangent sweep differentiates one weight set.
    """
    who = "population_gauss_newton"
    from . import sensitivity
    if model not in (capi.MODEL_HH2, capi.MODEL_MARKOV6, capi.MODEL_NNF, capi.MODEL_NND):
        raise capi.IonodeError(f"{who}: unknown model (HH 2-state and 6-state models, NN-f and NN-d with weights)")
    free = [int(f) for f in free]
    mlp = sensitivity.nn_route(who, model, weights, mlp_layers, mlp_width, free)
    if mlp:
        mlp["weights_key"] = weights_key
    D, npar = capi.n_state(model), capi.n_params(model)
    cand = np.asarray(candidates, dtype=np.float64).reshape(-1, len(free))
    C, P = cand.shape[0], np.asarray(protocols_v).shape[0]
    base = np.asarray(base_params, dtype=np.float64)
    if base.shape != (npar,) or len(y0) != D:
        raise capi.IonodeError(f"model {model}: base_params [{npar}] and y0 of {D} states expected")
    rank, world, bounds = distributed.population_shards(C, cost, group, "candidates")
    lo, hi = bounds[rank]
    dev = batched._dev(device) if solver is None else torch.device(device or "cpu")
    solve = sensitivity.gauss_newton if solver is None else solver
    params_all = np.tile(base, (C, 1))
    params_all[:, free] = cand
    max_step = _auto_max_step(max_step, model, lambda: params_all, protocols_v)
    nf = len(free)
    out = torch.empty((hi - lo, 1 + nf + nf * nf), dtype=torch.float64, device=dev)
    if hi > lo:
        n = hi - lo
        p = torch.from_numpy(np.repeat(params_all[lo:hi], P, axis=0)).to(dev)   # trajectory = c * P + protocol
        pot = torch.from_numpy(np.tile(np.arange(P, dtype=np.int32), n)).to(dev)
        y0t = torch.tensor([list(y0)], dtype=state_dtype, device=dev).expand(n * P, D).contiguous()
        sse, jtr, jtj, status = solve(model, p, torch.as_tensor(np.asarray(protocols_v), dtype=torch.float64, device=dev).contiguous(), y0t,
                                      torch.as_tensor(np.asarray(t_eval), dtype=torch.float64, device=dev).contiguous(),
                                      torch.as_tensor(np.asarray(data_i), dtype=torch.float64, device=dev).contiguous(),
                                      prot_t0=prot_t0, prot_dt=prot_dt, prot_of_traj=pot, obs_g=obs_g, obs_e=obs_e,
                                      obs_open_state_only=obs_open_state_only, max_total_steps=max_total_steps, max_step=max_step, **mlp)
        ok = (status.reshape(n, P) == 0).all(dim=1)
        err = sse.reshape(n, P).sum(dim=1)
        g = 2.0 * jtr.reshape(n, P, npar).sum(dim=1)[:, free]
        H = 2.0 * jtj.reshape(n, P, npar, npar).sum(dim=1)[:, free][:, :, free]
        if log_parameters:   # d/d log p_j = p_j d/dp_j
            pf = torch.from_numpy(params_all[lo:hi][:, free]).to(dev)
            g, H = g * pf, H * pf[:, :, None] * pf[:, None, :]
        out[:, 0] = torch.where(ok, err, torch.full_like(err, float("inf")))
        out[:, 1:1 + nf] = torch.where(ok[:, None], g, torch.zeros_like(g))
        out[:, 1 + nf:] = torch.where(ok[:, None], H.reshape(n, nf * nf), torch.zeros((), dtype=torch.float64, device=dev))
    out = distributed.all_gather_shards(out, bounds, rank, group)
    return out[:, 0].contiguous(), out[:, 1:1 + nf].contiguous(), out[:, 1 + nf:].reshape(-1, nf, nf).contiguous()


def population_fit(candidates, protocols_v, data_i, t_eval, *, base_params, free=(0, 1, 2, 3), log_parameters=True, bounds=None, prot_t0=0.0,
                   prot_dt=0.1, y0=(0.0, 1.0), state_dtype=torch.float32, obs_g=1.0, obs_e=-86.0, obs_open_state_only=False,
                   max_total_steps=1_000_000, max_step="auto", rtol=1e-7, atol=1e-9, group=None, device=None, solver=None, cost=None,
                   model=capi.MODEL_HH2, max_iter=50, gtol=1e-8, xtol=1e-8, ftol=1e-8, lam_init=1e-3, compact_every=4, weights=None,
                   mlp_layers=0, mlp_width=0, weights_key=None):
    """Multi-start Levenberg-Marquardt: every candidate is the start of a fit of the free parameters to data_i, all of them iterated
    together (fit.levenberg_marquardt: one sensitivity.gauss_newton evaluation and one ionode_lm_step launch per iteration, one read
    of the stop flags every compact_every iterations).

    candidates [C, len(free)] starting points; the other arguments as population_gauss_newton, plus bounds = (lo, hi) in the
    parameters (None: unbounded), the solve's rtol / atol, and the stopping rule (max_iter evaluations per candidate, gtol, xtol, ftol,
    lam_init: include/ionode.h "Levenberg-Marquardt step").  log_parameters (default, the reference's pints.LogTransformation,
    train-d0.py:511): the search runs in log p.  Returns (x [C, len(free)], sse [C], flag [C] int32, iterations [C, 2] int32 =
    (evaluations, accepted)) on the device: the best accepted point of every start, its sum of squares (inf where the start could not
    be evaluated), why it stopped (capi.LM_*: never 0) and what it cost.
    max_step "auto" is resolved ONCE, before the loop and before sharding: grad.stable_step_cap at the upper corner of the box --
    the stiffest point the fit can visit -- or, without bounds, over the starting population; the cap is then held, so the function
    being minimised is the same in every iteration and on every rank.
    Sharding as population_sum_of_squares_s1 (contiguous, or equal cost with `cost`); the fits of a shard need nothing from the
    others, so there is no communication during the fit and one all-gather of [C, len(free) + 4] at its end.  A candidate's result
    does not depend on the shard it ran in.  `solver` (tests only): a stand-in with sensitivity.gauss_newton's signature on CPU
    tensors -- the step then runs as ionode_lm_step_host and the loop, the compaction and the all-gather need no GPU.
    NN models (NN-f, NN-d -- the hybrid model's HH rates around a trained net are what train-d0.py fits): with weights [n] (ONE flat
    state dict shared by every start), mlp_layers, mlp_width and weights_key as population_gauss_newton; `free` indexes their 8 rate
    parameters (NN-f: 4..7 only); max_step "auto" is no cap for them, as in population_cmaes.  Without weights they are refused, and so
    is a weight set per candidate [C, n].
    Out of scope: CMA-ES (population_cmaes / cmaes.py, which also takes a population of nets), sensitivities with
    respect to y0.  A noise model and the posterior around a fit are population_mcmc / mcmc.py and population_mala / mala.py.
    """
    who = "population_fit"
    from . import fit, sensitivity
    if model not in (capi.MODEL_HH2, capi.MODEL_MARKOV6, capi.MODEL_NNF, capi.MODEL_NND):
        raise capi.IonodeError(f"{who}: unknown model (HH 2-state and 6-state models, NN-f and NN-d with weights)")
    free = [int(f) for f in free]
    sensitivity.nn_route(who, model, weights, mlp_layers, mlp_width, free)
    D, npar = capi.n_state(model), capi.n_params(model)
    nf = len(free)
    cand = np.asarray(candidates, dtype=np.float64).reshape(-1, nf)
    C = cand.shape[0]
    base = np.asarray(base_params, dtype=np.float64)
    if base.shape != (npar,) or len(y0) != D:
        raise capi.IonodeError(f"model {model}: base_params [{npar}] and y0 of {D} states expected")
    rank, world, bounds_r = distributed.population_shards(C, cost, group, "candidates")
    lo, hi = bounds_r[rank]
    dev = batched._dev(device) if solver is None else torch.device(device or "cpu")
    max_step = _auto_max_step(max_step, model, lambda: _corner_or_starts(base, free, bounds, cand), protocols_v)
    x, sse, flag, iters = fit.levenberg_marquardt(model, cand[lo:hi], protocols_v, data_i, t_eval, base_params=base, free=free,
                                                  log_parameters=log_parameters, bounds=bounds, prot_t0=prot_t0, prot_dt=prot_dt, y0=y0,
                                                  state_dtype=state_dtype, obs_g=obs_g, obs_e=obs_e, obs_open_state_only=obs_open_state_only,
                                                  max_total_steps=max_total_steps, max_step=float(max_step), rtol=rtol, atol=atol, device=dev,
                                                  solver=solver, max_iter=max_iter, gtol=gtol, xtol=xtol, ftol=ftol, lam_init=lam_init,
                                                  compact_every=compact_every, weights=weights, mlp_layers=mlp_layers, mlp_width=mlp_width,
                                                  weights_key=weights_key)
    out = torch.cat([x, sse[:, None], flag.double()[:, None], iters.double()], dim=1)   # [n, nf + 4]
    out = distributed.all_gather_shards(out, bounds_r, rank, group)
    return out[:, :nf].contiguous(), out[:, nf].contiguous(), out[:, nf + 1].to(torch.int32), out[:, nf + 2:].to(torch.int32).contiguous()


def population_cmaes(starts, protocols_v, data_i, t_eval, *, base_params, free=(0, 1, 2, 3), log_parameters=True, bounds=None, objective="sse",
                     popsize=None, sigma0=0.1, scale=None, seed=0, max_iter=1000, unchanged_iters=100, unchanged_threshold=1e-3, tolx=1e-11,
                     compact_every=4, prot_t0=0.0, prot_dt=0.1, y0=(0.0, 1.0), state_dtype=torch.float32, obs_g=1.0, obs_e=-86.0,
                     obs_open_state_only=False, max_total_steps=1_000_000, max_step="auto", rtol=1e-7, atol=1e-9, group=None, device=None,
                     solver=None, cost=None, model=capi.MODEL_HH2, weights=None, mlp_layers=0, mlp_width=0, weights_key=None):
    """Batched CMA-ES (the reference's optimiser: PINTS' CMA-ES under a LogTransformation, train-d0.py:508-540): every row of starts
    [K, len(free)] is the initial mean of an independent run, all of them advanced together (cmaes.minimise: one fused forward solve
    of K * lambda * P trajectories and one ionode_cmaes_step launch per generation, one read of the stop flags every compact_every
    generations).

    All four models and both objective kinds ("sse": the reference's SumOfSquaresError; "sae": sums of absolute residuals); the NN
    models take one shared weight set and `free` indexes their 8 rate parameters (NN-d's HH rates around a trained net are what
    train-d0.py fits).  bounds = (lo, hi) in the parameters (the reference: p0 * 0.1 .. p0 * 10) or None; sigma0 = 0.1 with scale 1
    in log parameters is the reference's sigma0 = 0.1 * p0; unchanged_iters = 100 at unchanged_threshold = 1e-3 is its stopping rule.
    Returns (x [K, len(free)], value [K], flag [K] int32, iterations [K, 2] int32 = (generations, evaluations)) on the device: the
    best point each run evaluated, its value (inf if none was finite), why it stopped (capi.CMAES_*: never 0) and what it cost.
    max_step "auto" is resolved ONCE, as population_fit resolves it: grad.stable_step_cap at the upper corner of the box, or without
    bounds over the starts; the NN models carry no such cap and take 0.
    Sharding as population_fit (contiguous, or equal cost with `cost`); the runs of a shard need nothing from the others -- a run's
    random numbers depend on (seed, its index among all K runs, generation, candidate, coordinate, attempt) only -- so there is no
    communication during the fit and one all-gather of [K, len(free) + 4] at its end, padded to the largest shard as the population
    errors are.  A run's result does not depend on the shard it ran in.  `solver` (tests only): a stand-in with batched.solve's
    signature on CPU tensors; the step then runs as ionode_cmaes_step_host.
    """
    from . import cmaes
    D, npar = capi.n_state(model), capi.n_params(model)
    free = [int(f) for f in free]
    nf = len(free)
    cand = np.asarray(starts, dtype=np.float64).reshape(-1, nf)
    K = cand.shape[0]
    base = np.asarray(base_params, dtype=np.float64)
    if base.shape != (npar,) or len(y0) != D:
        raise capi.IonodeError(f"model {model}: base_params [{npar}] and y0 of {D} states expected")
    rank, world, bounds_r = distributed.population_shards(K, cost, group, "runs")
    lo, hi = bounds_r[rank]
    dev = batched._dev(device) if solver is None else torch.device(device or "cpu")
    max_step = _auto_max_step(max_step, model, lambda: _corner_or_starts(base, free, bounds, cand), protocols_v)
    x, val, flag, iters = cmaes.minimise(model, cand[lo:hi], protocols_v, data_i, t_eval, base_params=base, free=free, log_parameters=log_parameters,
                                         bounds=bounds, objective=objective, popsize=popsize, sigma0=sigma0, scale=scale, seed=seed,
                                         max_iter=max_iter, unchanged_iters=unchanged_iters, unchanged_threshold=unchanged_threshold, tolx=tolx,
                                         compact_every=compact_every, weights=weights, mlp_layers=mlp_layers, mlp_width=mlp_width,
                                         weights_key=weights_key, prot_t0=prot_t0, prot_dt=prot_dt, y0=y0, state_dtype=state_dtype, obs_g=obs_g,
                                         obs_e=obs_e, obs_open_state_only=obs_open_state_only, max_total_steps=max_total_steps,
                                         max_step=float(max_step), rtol=rtol, atol=atol, device=dev, solver=solver, run_offset=lo)
    out = torch.cat([x, val[:, None], flag.double()[:, None], iters.double()], dim=1)   # [n, nf + 4]
    out = distributed.all_gather_shards(out, bounds_r, rank, group)
    return out[:, :nf].contiguous(), out[:, nf].contiguous(), out[:, nf + 1].to(torch.int32), out[:, nf + 2:].to(torch.int32).contiguous()


def population_mcmc(starts, protocols_v, data_i, t_eval, *, base_params, free=(0, 1, 2, 3), log_parameters=True, bounds, sigma=None,
                    sigma_bounds=None, scale=None, seed=0, max_iter=10000, adapt_start=200, thin=1, eta=0.6, target_accept=0.234,
                    epsilon=1e-12, compact_every=64, prot_t0=0.0, prot_dt=0.1, y0=(0.0, 1.0), state_dtype=torch.float32, obs_g=1.0, obs_e=-86.0,
                    obs_open_state_only=False, max_total_steps=1_000_000, max_step="auto", rtol=1e-7, atol=1e-9, group=None, device=None,
                    solver=None, cost=None, model=capi.MODEL_HH2, weights=None, mlp_layers=0, mlp_width=0, weights_key=None):
    """Batched adaptive Metropolis (what follows a fit of noisy data in the reference's workflow: the posterior under a Gaussian noise
    model): every row of starts [K, len(free)] (or [K, len(free) + 1], the last column sigma's start, when sigma is sampled) is the
    start of an independent chain, all of them advanced together (mcmc.sample: one fused forward solve of K * P trajectories and one
    ionode_mcmc_step launch per iteration, one read of the stop flags every compact_every iterations).

    All four models; the NN models take one shared weight set and `free` indexes their 8 rate parameters.  bounds = (lo, hi) in the
    parameters, required and finite: the prior is uniform over the box in the search space -- LOG-UNIFORM in the parameters with
    log_parameters (the default).  Exactly one of sigma (fixed noise level) and sigma_bounds (sigma sampled, log-uniform within them).
    Returns (samples [K, R, n + 1], accept_rate [K], flag [K] int32, iterations [K, 2] int32 = (iterations, accepted)) on the device,
    as mcmc.sample does; mcmc.rhat turns the samples into Gelman and Rubin's R-hat.
    max_step "auto" is resolved ONCE, as population_cmaes resolves it: grad.stable_step_cap at the upper corner of the box; the NN
    models carry no such cap and take 0.
    Sharding as population_cmaes (contiguous, or equal cost with `cost`); the chains of a shard need nothing from the others -- a
    chain's random numbers depend on (seed, its index among all K chains, iteration, purpose, coordinate) only -- so there is no
    communication during the run and one all-gather at its end, padded to the largest shard.  A chain's samples do not depend on
    the shard it ran in.  `solver` (tests only): a stand-in with batched.solve's signature on CPU tensors; the step then runs as
    ionode_mcmc_step_host.
    """
    from . import mcmc
    D, npar = capi.n_state(model), capi.n_params(model)
    free = [int(f) for f in free]
    nf = len(free)
    n = nf + int(sigma is None)
    cand = np.asarray(starts, dtype=np.float64)
    if cand.ndim != 2:
        cand = cand.reshape(-1, nf)
    K = cand.shape[0]
    base = np.asarray(base_params, dtype=np.float64)
    if base.shape != (npar,) or len(y0) != D:
        raise capi.IonodeError(f"model {model}: base_params [{npar}] and y0 of {D} states expected")
    if bounds is None:
        raise capi.IonodeError("population_mcmc: bounds = (lo, hi) are required: the box is the prior")
    if (sigma is None) == (sigma_bounds is None):
        raise capi.IonodeError("population_mcmc: exactly one of sigma (fixed noise) and sigma_bounds (sampled noise) must be given")
    rank, world, bounds_r = distributed.population_shards(K, cost, group, "chains")
    lo, hi = bounds_r[rank]
    dev = batched._dev(device) if solver is None else torch.device(device or "cpu")
    def corner():
        rows = base[None].copy()
        rows[:, free] = np.asarray(bounds[1], dtype=np.float64)
        return rows
    max_step = _auto_max_step(max_step, model, corner, protocols_v)
    smp, rate, flag, iters = mcmc.sample(model, cand[lo:hi], protocols_v, data_i, t_eval, base_params=base, free=free, log_parameters=log_parameters,
                                         bounds=bounds, sigma=sigma, sigma_bounds=sigma_bounds, scale=scale, seed=seed, max_iter=max_iter,
                                         adapt_start=adapt_start, thin=thin, eta=eta, target_accept=target_accept, epsilon=epsilon,
                                         compact_every=compact_every, weights=weights, mlp_layers=mlp_layers, mlp_width=mlp_width,
                                         weights_key=weights_key, prot_t0=prot_t0, prot_dt=prot_dt, y0=y0, state_dtype=state_dtype, obs_g=obs_g,
                                         obs_e=obs_e, obs_open_state_only=obs_open_state_only, max_total_steps=max_total_steps,
                                         max_step=float(max_step), rtol=rtol, atol=atol, device=dev, solver=solver, chain_offset=lo)
    R = smp.shape[1]
    out = torch.cat([smp.reshape(hi - lo, R * (n + 1)), rate[:, None], flag.double()[:, None], iters.double()], dim=1)   # [chains, R (n + 1) + 4]
    out = distributed.all_gather_shards(out, bounds_r, rank, group)
    w = R * (n + 1)
    return (out[:, :w].reshape(-1, R, n + 1).contiguous(), out[:, w].contiguous(), out[:, w + 1].to(torch.int32),
            out[:, w + 2:].to(torch.int32).contiguous())


def population_mala(starts, protocols_v, data_i, t_eval, *, base_params, free=(0, 1, 2, 3), log_parameters=True, bounds, sigma=None,
                    sigma_bounds=None, eps0=1.0, ridge=2.0 ** -20, seed=0, max_iter=1000, thin=1, eta=0.6, target_accept=0.574,
                    compact_every=64, prot_t0=0.0, prot_dt=0.1, y0=(0.0, 1.0), state_dtype=torch.float32, obs_g=1.0, obs_e=-86.0,
                    obs_open_state_only=False, max_total_steps=1_000_000, max_step="auto", rtol=1e-7, atol=1e-9, group=None, device=None,
                    solver=None, cost=None, model=capi.MODEL_HH2, weights=None, mlp_layers=0, mlp_width=0, weights_key=None):
    """Batched manifold MALA (the sampler that uses what the fit computes: the Gauss-Newton matrix J^T J / sigma^2 is the proposal's
    metric, from iteration 0, with nothing to learn but the step size): every row of starts [K, len(free)] (or [K, len(free) + 1],
    the last column sigma's start, when sigma is sampled) -- typically population_fit's optimum -- is the start of an independent
    chain, all of them advanced together (mala.sample: one sensitivity.gauss_newton evaluation of K * P trajectories and one
    ionode_mala_step launch per iteration, one read of the stop flags every compact_every iterations).

    HH 2-state and 6-state, and -- with weights [n] (ONE flat state dict shared by every chain), mlp_layers, mlp_width, weights_key as
    population_gauss_newton -- NN-f and NN-d (`free` indexes their 8 rate parameters, NN-f: 4..7 only; "auto" is no cap for them).
    An NN model without weights is refused (population_mcmc needs them as well), and so is a weight set per chain [K, n].
    Target, prior, bounds, sigma /
    sigma_bounds and the returned (samples [K, R, n + 1], accept_rate [K], flag [K] int32, iterations [K, 2] int32) are
    population_mcmc's; mcmc.rhat serves both samplers.  max_step "auto" is resolved ONCE: grad.stable_step_cap at the upper corner of
    the box.  Sharding as population_mcmc (contiguous, or equal cost with `cost`): a chain's random numbers depend on (seed, its
    index among all K chains, iteration, purpose, coordinate) only, so there is no communication during the run and one all-gather
    at its end; a chain's samples do not depend on the shard it ran in.  `solver` (tests only): a stand-in with
    sensitivity.gauss_newton's signature on CPU tensors; the step then runs as ionode_mala_step_host.
    """
    from . import mala, sensitivity
    free = [int(f) for f in free]
    sensitivity.nn_route("population_mala", model, weights, mlp_layers, mlp_width, free)
    D, npar = capi.n_state(model), capi.n_params(model)
    nf = len(free)
    n = nf + int(sigma is None)
    cand = np.asarray(starts, dtype=np.float64)
    if cand.ndim != 2:
        cand = cand.reshape(-1, nf)
    K = cand.shape[0]
    base = np.asarray(base_params, dtype=np.float64)
    if base.shape != (npar,) or len(y0) != D:
        raise capi.IonodeError(f"model {model}: base_params [{npar}] and y0 of {D} states expected")
    if bounds is None:
        raise capi.IonodeError("population_mala: bounds = (lo, hi) are required: the box is the prior")
    if (sigma is None) == (sigma_bounds is None):
        raise capi.IonodeError("population_mala: exactly one of sigma (fixed noise) and sigma_bounds (sampled noise) must be given")
    rank, world, bounds_r = distributed.population_shards(K, cost, group, "chains")
    lo, hi = bounds_r[rank]
    dev = batched._dev(device) if solver is None else torch.device(device or "cpu")
    def corner():
        rows = base[None].copy()
        rows[:, free] = np.asarray(bounds[1], dtype=np.float64)
        return rows
    max_step = _auto_max_step(max_step, model, corner, protocols_v)
    smp, rate, flag, iters = mala.sample(model, cand[lo:hi], protocols_v, data_i, t_eval, base_params=base, free=free, log_parameters=log_parameters,
                                         bounds=bounds, sigma=sigma, sigma_bounds=sigma_bounds, eps0=eps0, ridge=ridge, seed=seed, max_iter=max_iter,
                                         thin=thin, eta=eta, target_accept=target_accept, compact_every=compact_every, prot_t0=prot_t0,
                                         prot_dt=prot_dt, y0=y0, state_dtype=state_dtype, obs_g=obs_g, obs_e=obs_e,
                                         obs_open_state_only=obs_open_state_only, max_total_steps=max_total_steps, max_step=float(max_step),
                                         rtol=rtol, atol=atol, device=dev, solver=solver, chain_offset=lo, weights=weights, mlp_layers=mlp_layers,
                                         mlp_width=mlp_width, weights_key=weights_key)
    R = smp.shape[1]
    out = torch.cat([smp.reshape(hi - lo, R * (n + 1)), rate[:, None], flag.double()[:, None], iters.double()], dim=1)   # [chains, R (n + 1) + 4]
    out = distributed.all_gather_shards(out, bounds_r, rank, group)
    w = R * (n + 1)
    return (out[:, :w].reshape(-1, R, n + 1).contiguous(), out[:, w].contiguous(), out[:, w + 1].to(torch.int32),
            out[:, w + 2:].to(torch.int32).contiguous())


def population_ensemble(starts, protocols_v, data_i, t_eval, *, base_params, free=(0, 1, 2, 3), log_parameters=True, bounds, sigma=None,
                        sigma_bounds=None, move="stretch", a=2.0, gamma=None, jitter=1e-5, walkers=None, spread=1e-3, seed=0, max_iter=1000,
                        thin=1, prot_t0=0.0, prot_dt=0.1, y0=(0.0, 1.0), state_dtype=torch.float32, obs_g=1.0, obs_e=-86.0,
                        obs_open_state_only=False, max_total_steps=1_000_000, max_step="auto", rtol=1e-7, atol=1e-9, group=None, device=None,
                        solver=None, cost=None, model=capi.MODEL_HH2, weights=None, mlp_layers=0, mlp_width=0, weights_key=None):
    """Batched affine-invariant ensemble sampling (the sampler whose proposals come from the other walkers' current positions: nothing
    to tune, nothing to learn, indifferent to the posterior's scales and tilt): starts [E, W, len(free)] (or [E, W, len(free) + 1],
    the last column sigma's start, when sigma is sampled) are the walkers of E independent ensembles; or [E, len(free)] (+ 1) centres
    -- typically population_fit's optimum -- with walkers=W and spread (ensemble.spread_starts).  All ensembles advance together
    (ensemble.sample: per half-iteration one fused forward solve of E * W / 2 * P trajectories and one ionode_ensemble_step launch,
    no host read in the loop).  move "stretch" (Goodman and Weare 2010) or "de" (ter Braak 2006).

    Models, bounds, sigma / sigma_bounds, max_step "auto" and the NN models' weights: as population_mcmc.  max_iter counts full
    iterations.  Returns (samples [E, W, R, n + 1], acceptance [E, W], flag [E] int32, iterations [E, 2] int32 = (calls, full
    iterations)) on the device, as ensemble.sample does; mcmc.rhat on samples.reshape(E * W, R, n + 1) is R-hat over all walkers --
    the walkers of one ensemble are not independent chains.
    Sharding as population_mcmc, by ENSEMBLE (contiguous, or equal cost with `cost` [E]); an ensemble's random numbers depend on
    (seed, its index among all E ensembles, walker, call, role) only, so there is no communication during the run and one all-gather
    at its end; an ensemble's samples do not depend on the shard it ran in.  `solver` (tests only): a stand-in with batched.solve's
    signature on CPU tensors; the step then runs as ionode_ensemble_step_host.
    """
    from . import ensemble
    D, npar = capi.n_state(model), capi.n_params(model)
    free = [int(f) for f in free]
    nf = len(free)
    n = nf + int(sigma is None)
    cand = np.asarray(starts, dtype=np.float64)
    if cand.ndim not in (2, 3):
        raise capi.IonodeError(f"population_ensemble: starts [E, W, {nf}] or centres [E, {nf}] with walkers= expected, got {tuple(cand.shape)}")
    E = cand.shape[0]
    base = np.asarray(base_params, dtype=np.float64)
    if base.shape != (npar,) or len(y0) != D:
        raise capi.IonodeError(f"model {model}: base_params [{npar}] and y0 of {D} states expected")
    if bounds is None:
        raise capi.IonodeError("population_ensemble: bounds = (lo, hi) are required: the box is the prior")
    if (sigma is None) == (sigma_bounds is None):
        raise capi.IonodeError("population_ensemble: exactly one of sigma (fixed noise) and sigma_bounds (sampled noise) must be given")
    rank, world, bounds_r = distributed.population_shards(E, cost, group, "ensembles")
    lo, hi = bounds_r[rank]
    dev = batched._dev(device) if solver is None else torch.device(device or "cpu")
    def corner():
        rows = base[None].copy()
        rows[:, free] = np.asarray(bounds[1], dtype=np.float64)
        return rows
    max_step = _auto_max_step(max_step, model, corner, protocols_v)
    smp, rate, flag, iters = ensemble.sample(model, cand[lo:hi], protocols_v, data_i, t_eval, base_params=base, free=free,
                                             log_parameters=log_parameters, bounds=bounds, sigma=sigma, sigma_bounds=sigma_bounds, move=move, a=a,
                                             gamma=gamma, jitter=jitter, walkers=walkers, spread=spread, seed=seed, max_iter=max_iter, thin=thin,
                                             weights=weights, mlp_layers=mlp_layers, mlp_width=mlp_width, weights_key=weights_key, prot_t0=prot_t0,
                                             prot_dt=prot_dt, y0=y0, state_dtype=state_dtype, obs_g=obs_g, obs_e=obs_e,
                                             obs_open_state_only=obs_open_state_only, max_total_steps=max_total_steps, max_step=float(max_step),
                                             rtol=rtol, atol=atol, device=dev, solver=solver, ensemble_offset=lo)
    W, R = smp.shape[1], smp.shape[2]
    w = W * R * (n + 1)
    out = torch.cat([smp.reshape(hi - lo, w), rate, flag.double()[:, None], iters.double()], dim=1)   # [ensembles, W R (n + 1) + W + 3]
    out = distributed.all_gather_shards(out, bounds_r, rank, group)
    return (out[:, :w].reshape(-1, W, R, n + 1).contiguous(), out[:, w:w + W].contiguous(), out[:, w + W].to(torch.int32),
            out[:, w + W + 1:].to(torch.int32).contiguous())


def population_predictive(draws, protocols_v, t_eval, *, base_params, free=(0, 1, 2, 3), log_parameters=True, coordinates="parameters", sigma=None,
                          quantiles=(0.025, 0.5, 0.975), noise=False, seed=0, chunk_bytes=1 << 30, budget_bytes=32 << 30, prot_t0=0.0,
                          prot_dt=0.1, y0=(0.0, 1.0), state_dtype=torch.float32, obs_g=1.0, obs_e=-86.0, obs_open_state_only=False,
                          max_total_steps=1_000_000, max_step="auto", rtol=1e-7, atol=1e-9, group=None, device=None, solver=None,
                          model=capi.MODEL_HH2, weights=None, mlp_layers=0, mlp_width=0, weights_key=None):
    """Posterior predictive bands of the current over parameter draws (predictive.draws of a sampler's output): per protocol and
    output sample the mean, the standard deviation, the extremes and exact quantiles of i(t) -- of i(t) + sigma z with noise=True --
    over draws [S, len(free)] (or [S, len(free) + 1], sigma last).  predictive.bands does the work: the draws are solved in chunks,
    one fused forward solve with the current epilogue and one ionode_predictive_accumulate launch each, no host read between them,
    and one ionode_predictive_quantiles launch at the end.  Returns predictive.Bands.

    All four models; the NN models take one shared weight set and `free` indexes their 8 rate parameters.  max_step "auto" is
    resolved ONCE, before sharding, to grad.stable_step_cap over all draws (non-finite rows left out), so that every rank integrates
    the same function; the NN models carry no such cap and take 0.
    Sharding: contiguous shards of equal count; a rank's noise is a function of a draw's index among ALL draws, so the values do not
    depend on the shard.  The moments merge across the ranks by the pairwise Welford merge IN RANK ORDER -- n = n_a + n_b,
    d = mean_b - mean_a, mean = mean_a + d n_b / n, m2 = m2_a + m2_b + d^2 n_a n_b / n -- after one all-gather: every rank returns
    the same Bands, equal to the single-rank ones up to that merge's rounding (not bit for bit).  Exact quantiles need every draw of
    a column on one device: with a group of more than one rank they are REFUSED (pass quantiles=None for the moments, or run the
    quantiles on one rank); gathering the column stores is out of scope.
    `solver` (tests only): a stand-in with batched.solve's signature on CPU tensors; the passes then run as the host mirrors."""
    from . import predictive
    npar = capi.n_params(model)
    free = [int(f) for f in free]
    base = np.asarray(base_params, dtype=np.float64)
    if base.shape != (npar,):
        raise capi.IonodeError(f"model {model}: base_params [{npar}] expected")
    x, _ = predictive.parameters(draws, len(free), log_parameters=log_parameters, coordinates=coordinates)
    d = np.asarray(draws.detach().cpu() if isinstance(draws, torch.Tensor) else draws, dtype=np.float64)
    S = d.shape[0]
    rank, world, bounds_r = distributed.population_shards(S, None, group, "draws")
    q = tuple(quantiles) if quantiles is not None else ()
    if world > 1 and q:
        raise capi.IonodeError(f"population_predictive: exact quantiles need all draws of a column on one device and the group has {world} "
                               "ranks: pass quantiles=None for the moments, or run the quantiles on one rank")
    def rows():
        r = np.tile(base, (S, 1))
        r[:, free] = x
        return r
    max_step = _auto_max_step(max_step, model, rows, protocols_v)
    lo, hi = bounds_r[rank]
    dev = batched._dev(device) if solver is None else torch.device(device or "cpu")
    P, Nt = np.asarray(protocols_v).shape[0], np.asarray(t_eval).shape[0]
    if hi > lo:
        b = predictive.bands(model, d[lo:hi], protocols_v, t_eval, base_params=base, free=free, log_parameters=log_parameters,
                             coordinates=coordinates, sigma=sigma, quantiles=q, noise=noise, seed=seed, chunk_bytes=chunk_bytes,
                             budget_bytes=budget_bytes, solver=solver, draw_offset=lo, weights=weights, mlp_layers=mlp_layers, mlp_width=mlp_width,
                             weights_key=weights_key, prot_t0=prot_t0, prot_dt=prot_dt, y0=y0, state_dtype=state_dtype, obs_g=obs_g, obs_e=obs_e,
                             obs_open_state_only=obs_open_state_only, max_total_steps=max_total_steps, max_step=float(max_step), rtol=rtol,
                             atol=atol, device=dev)
        if world == 1:
            return b
        st = {"mean": torch.nan_to_num(b.mean, nan=0.0), "m2": b.m2, "min": torch.nan_to_num(b.min, nan=float("inf")),
              "max": torch.nan_to_num(b.max, nan=float("-inf")), "count": b.count}
    else:
        st = predictive.new_state(P, Nt, 1, dev, store=False)
    import torch.distributed as dist
    mine = torch.cat([torch.stack([st["mean"], st["m2"], st["min"], st["max"]]).reshape(4, P * Nt),
                      st["count"].double()[None, :].expand(4, P)], dim=1).contiguous()   # [4, P Nt + P]: the counts ride along (exact in fp64)
    parts = [torch.empty_like(mine) for _ in range(world)]
    dist.all_gather(parts, mine, group=group)
    acc = None
    for part in parts:   # rank order
        mom, n_b = part[:, :P * Nt].reshape(4, P, Nt), part[0, P * Nt:][:, None]
        if acc is None:
            acc, n_a = mom.clone(), n_b.clone()
            continue
        n = n_a + n_b
        dlt = mom[0] - acc[0]
        safe = n.clamp(min=1.0)
        acc[0] = torch.where(n_b > 0, acc[0] + dlt * n_b / safe, acc[0])
        acc[1] = torch.where(n_b > 0, acc[1] + mom[1] + dlt * dlt * n_a * n_b / safe, acc[1])
        acc[2], acc[3] = torch.minimum(acc[2], mom[2]), torch.maximum(acc[3], mom[3])
        n_a = n
    merged = {"mean": acc[0], "m2": acc[1], "min": acc[2], "max": acc[3], "count": n_a[:, 0].to(torch.int64)}
    return predictive.finish(merged, (), S)
