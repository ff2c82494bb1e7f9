"""Batched CMA-ES: many independent runs of Hansen's (mu/mu_w, lambda)-CMA-ES advanced together (all four models, either objective).

Reference: the candidate-model fits (train-d0.py:508-540: PINTS' CMA-ES on SumOfSquaresError under a LogTransformation, the box
p0 * 0.1 .. p0 * 10, sigma0 = 0.1 * p0, stopping after 100 unchanged iterations at a threshold of 1e-3, one candidate at a time over a
process pool).  Here every run -- a restart, a cell, a start point, a seed -- owns lambda candidates per generation, and one generation
of ALL runs is two library calls on one stream:

  batched.solve            on the trial tensor [n_active * lambda * P, NPAR] with the fused objective (sse_ref=..., states=False,
                           objective="sse" | "sae"): one value and one status per trajectory, no trace written;
  ionode_cmaes_step        (csrc/ionode_cmaes.hpp, include/ionode.h): the tell of that generation -- protocol sums, ranking, mean,
                           paths, step size, covariance, its eigen-decomposition by cyclic Jacobi, best point, stop flags -- and the
                           ask of the next, written into the trial tensor in place.

Between the two there is no torch arithmetic and no host synchronisation.  Every `compact_every` generations the flags are read once
and the runs still going are packed into the front launch slots (the step's `active` list).  The random numbers are a pure function
of (seed, run, generation, candidate, coordinate pair, attempt), so a run's iterates do not depend on the others: compaction, the
batch around it and the sharding of objective.population_cmaes leave its bits alone, and the host mirror (ionode_cmaes_step_host)
equals the kernel bit for bit.

The derivative-based sibling is fit.py (Levenberg-Marquardt: HH 2-state and 6-state, sum of squares only).
Out of scope: bit-compatibility with PINTS or the cma package (boundary transform, penalties), negative weights, restarts with a
growing population, variants for more than 12 variables, fitting MLP weights.  A noise model and the posterior around a fit are mcmc.py
(adaptive Metropolis on the same fused sums: ionode_mcmc_step, objective.population_mcmc).
"""
import numpy as np
import torch

from . import capi, steploop

FLAG_TEXT = capi.CMAES_FLAG_TEXT


def cmaes_desc(n_run, popsize, n_prot, n_params, free, base_params, *, log_parameters, lo, hi, max_iter, unchanged_iters=100,
               unchanged_threshold=1e-3, tolx=1e-11, seed=0):
    """ionode_cmaes_desc for a fit: lo / hi [nf] in the parameters (None: no bound; with log_parameters a missing lower bound is the
    smallest normal number, the step refuses non-positive bounds).  popsize None: 4 + floor(3 ln nf)."""
    nf = len(free)
    lam = capi.cmaes_default_lambda(max(nf, 1)) if popsize is None else int(popsize)
    d = capi.IonodeCmaesDesc(n_run=int(n_run), n_active=int(n_run), n_prot=int(n_prot), n_params=int(n_params), n_free=nf,
                             log_parameters=int(bool(log_parameters)), max_iter=int(max_iter), unchanged_iters=int(unchanged_iters),
                             unchanged_threshold=float(unchanged_threshold), tolx=float(tolx), seed=int(seed))
    setattr(d, "lambda", lam)
    return steploop.fill_box(d, free, base_params, lo, hi)


def cmaes_init(x0, desc, sigma0=0.1, scale=None):
    """(state [K, cmaes_state_doubles(nf, lambda)] fp64, flag [K] int32, iters [K, 2] int32, trial [K * lambda * P, NPAR] fp64) of a fit
    whose runs start at x0 [K, nf]: m = u0 (log x0 with log_parameters), sigma = sigma0, C = diag(scale^2) (scale [nf] or None: 1 --
    the reference's sigma0 = 0.1 * p0 under the log transform), B = I, best x = x0, best f = +inf.  The trial rows hold x0: the first
    step overwrites them.  numpy arrays."""
    x0 = np.ascontiguousarray(np.asarray(x0, dtype=np.float64))
    K, nf = x0.shape
    lam = getattr(desc, "lambda")
    state = np.zeros((K, capi.cmaes_state_doubles(nf, lam)))
    v = capi.cmaes_state_views(state, nf, lam)
    s = np.ones(nf) if scale is None else np.asarray(scale, dtype=np.float64).reshape(nf)
    with np.errstate(all="ignore"):
        u0 = np.log(x0) if desc.log_parameters else x0
    v["sigma"][:], v["sigma_old"][:], v["best_f"][:], v["f_sig"][:] = float(sigma0), float(sigma0), np.inf, np.inf
    v["m"][:], v["m_old"][:], v["best_x"][:], v["D"][:] = u0, u0, x0, s
    v["C"][:], v["B"][:] = np.diag(s * s), np.eye(nf)
    return state, np.zeros(K, dtype=np.int32), np.zeros((K, 2), dtype=np.int32), steploop.trial_rows(desc, x0, lam * desc.n_prot)


def cmaes_step(desc, active, value, status, state, flag, iters, trial):
    """One ionode_cmaes_step on torch tensors: on the current stream for device tensors, ionode_cmaes_step_host for CPU tensors (the
    same phases, bit for bit).  desc.n_active is set from `active` (int32 [n_active] or None: every run, slot = run)."""
    nf, P, npar, lam = desc.n_free, desc.n_prot, desc.n_params, getattr(desc, "lambda")
    n_active = desc.n_run if active is None else int(active.shape[0])
    desc.n_active = n_active
    rows = n_active * lam * P
    want = (("value", value, torch.float64, (rows,)), ("status", status, torch.int32, (rows,)),
            ("state", state, torch.float64, (desc.n_run, capi.cmaes_state_doubles(nf, lam))), ("flag", flag, torch.int32, (desc.n_run,)),
            ("iters", iters, torch.int32, (desc.n_run, 2)), ("trial", trial, torch.float64, (rows, npar))) \
        + ((("active", active, torch.int32, (n_active,)),) if active is not None else ())
    steploop.step_call("cmaes", desc, state.device, want, (active, value, status, state, flag, iters, trial))


def minimise(model, x0, protocols_v, data_i, t_eval, *, base_params, free=(0, 1, 2, 3), log_parameters=True, bounds=None, objective="sse",
             popsize=None, sigma0=0.1, scale=None, seed=0, max_iter=1000, unchanged_iters=100, unchanged_threshold=1e-3, tolx=1e-11,
             compact_every=4, weights=None, mlp_layers=0, mlp_width=0, weights_key=None, prot_t0=0.0, prot_dt=0.1, y0=(0.0, 1.0),
             state_dtype=torch.float32, obs_g=1.0, obs_e=-86.0, obs_open_state_only=False, max_total_steps=1_000_000, max_step=0.0, rtol=1e-7,
             atol=1e-9, device=None, solver=None, callback=None, run_offset=0):
    """Minimise the fused objective over the free rate parameters with K independent CMA-ES runs on one device: x0 [K, nf], one run
    per row (its initial mean).

    model: any of the four; the NN models take one shared weight set (weights / mlp_layers / mlp_width / weights_key as
    batched.solve) and `free` indexes the 8 rate parameters.  protocols_v [P, Np], data_i [P, Nt], t_eval [Nt], base_params [8 | 12];
    bounds = (lo [nf], hi [nf]) in the parameters or None; log_parameters: search in log x (the reference's LogTransformation).
    objective "sse" | "sae": what a trajectory contributes (batched.solve); a run's value is the sum over its P protocols.
    popsize None: 4 + floor(3 ln nf).  sigma0 / scale: initial step size and per-coordinate scale in the search space (0.1 and 1: the
    reference's sigma0 = 0.1 * p0 in log parameters).  seed, and run_offset (the index of x0's first row among all runs: sharding),
    fix every random number.  Stops: max_iter generations, unchanged_iters / unchanged_threshold (PINTS' rule), tolx, the condition
    limit, non-finite evaluations (include/ionode.h "CMA-ES step").  max_step is a NUMBER here (ms, 0: no cap);
    objective.population_cmaes resolves "auto".  compact_every: generations between two reads of the flags (None or 0: never -- the
    loop then runs max_iter + 1 steps).  callback(generation, state, flag, iters) (tests, traces) sees the live tensors after every step.
    Returns (x [K, nf] fp64, value [K] fp64, flag [K] int32 (capi.CMAES_*, FLAG_TEXT), iterations [K, 2] int32 = (generations,
    evaluations)) on the device: the best point every run has evaluated.
    `solver` (tests only): a stand-in with batched.solve's signature on CPU tensors; the step is then ionode_cmaes_step_host and nothing
    needs a GPU.  The product default has no CPU path."""
    from . import batched
    kind = capi.objective_kind(objective)
    if model not in (capi.MODEL_HH2, capi.MODEL_MARKOV6, capi.MODEL_NNF, capi.MODEL_NND):
        raise capi.IonodeError(f"cmaes.minimise: unknown model {model}")
    D, npar = capi.n_state(model), capi.n_params(model)
    free = [int(f) for f in free]
    nf = len(free)
    if not 1 <= nf <= capi.LM_MAX_FREE:
        raise capi.IonodeError(f"cmaes.minimise: 1 .. {capi.LM_MAX_FREE} free parameters, got {nf}")
    x0 = np.asarray(x0, dtype=np.float64).reshape(-1, nf)
    base = np.asarray(base_params, dtype=np.float64)
    if base.shape != (npar,) or len(y0) != D:
        raise capi.IonodeError(f"model {model}: base_params [{npar}] and y0 of {D} states expected")
    if isinstance(max_step, str):
        raise capi.IonodeError("cmaes.minimise: max_step must be a number (objective.population_cmaes resolves 'auto' once)")
    K, P = x0.shape[0], np.asarray(protocols_v).shape[0]
    dev = batched._dev(device) if solver is None else torch.device(device or "cpu")
    solve = batched.solve if solver is None else solver
    lo, hi = (None, None) if bounds is None else bounds
    desc = cmaes_desc(max(K, 1), popsize, P, npar, free, base, log_parameters=log_parameters, lo=lo, hi=hi, max_iter=max_iter,
                      unchanged_iters=unchanged_iters, unchanged_threshold=unchanged_threshold, tolx=tolx, seed=seed)
    lam = getattr(desc, "lambda")
    if K == 0:
        return steploop.empty_result((nf,), dev)
    desc.run_base = int(run_offset)   # the generator's run index: a shard's runs draw what they draw in the whole population
    state, flag, iters, trial = (torch.from_numpy(a).to(dev) for a in cmaes_init(x0, desc, sigma0, scale))
    pv, te, ref, pot, y0t = steploop.problem_tensors(protocols_v, t_eval, data_i, y0, K * lam * P, state_dtype, dev)
    mlp = {} if weights is None else dict(weights=weights, mlp_layers=mlp_layers, mlp_width=mlp_width, weights_key=weights_key)
    active, n_act = None, K
    every = int(compact_every or 0)
    value = torch.zeros((K * lam * P,), dtype=torch.float64, device=dev)      # the first step reads nothing of these
    status = torch.zeros((K * lam * P,), dtype=torch.int32, device=dev)
    for it in range(int(max_iter) + 1):
        cmaes_step(desc, active, value, status, state, flag, iters, trial)
        if callback is not None:
            callback(it, state, flag, iters)
        if every and it % every == 0 and it:   # the one read: who is still running
            left = steploop.compact(flag, active, n_act, trial, capi.CMAES_RUNNING)
            if left is None:
                break
            active, n_act, trial = left
        if it == int(max_iter):
            break
        rows = n_act * lam * P
        sol = solve(model, trial, pv, y0t[:rows], te, prot_t0=prot_t0, prot_dt=prot_dt, prot_of_traj=pot[:rows], obs_g=obs_g, obs_e=obs_e,
                    obs_open_state_only=obs_open_state_only, max_total_steps=max_total_steps, max_step=max_step, rtol=rtol, atol=atol,
                    device=dev, sse_ref=ref, states=False, objective=objective, **mlp)
        value = (sol.sse if kind == capi.OBJECTIVE_SSE else sol.sae).contiguous()
        status = sol.status.to(torch.int32).contiguous()
    v = capi.cmaes_state_views(state, nf, lam)
    return v["best_x"].contiguous(), v["best_f"].contiguous(), flag, iters
