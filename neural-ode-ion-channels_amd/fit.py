"""Multi-start Levenberg-Marquardt for a whole population of candidates (closed-form HH 2-state and 6-state models; NN-f / NN-d with weights).

Reference: the candidate-model fits (train-d0.py:508-540: a PINTS optimiser on SumOfSquaresError under a LogTransformation, one
candidate at a time over a process pool).  Here every candidate of a population is a start of a damped Gauss-Newton iteration,
and one iteration of ALL of them is two library calls on one stream:

  sensitivity.gauss_newton   on the trial tensor [n_active * P, NPAR]: the checkpointed forward with the fused sum of squares, and
                             the tangent sweep's J^T r and J^T J;
  ionode_lm_step             (csrc/ionode_lm.hpp, include/ionode.h): reduces each candidate's P protocols, decides about the trial
                             point (gain ratio, Nielsen's damping update), sets the stop flags, solves the damped system by
                             Cholesky, projects the step into the box and writes the next trial tensor in place.

Between the two there is no torch arithmetic and the step adds no host synchronisation (the evaluation's own check of its
checkpoint buffer's size is the one read that remains in an iteration).  Every `compact_every` iterations the flags are read once
and the candidates still running are packed into the front launch slots (the step's `active` list), so a stopped candidate costs no
solve after at most `compact_every` further iterations.  A candidate's iterates do not depend on the others: compaction, the batch
around it and the sharding of objective.population_fit leave its bits alone.

NN models: NN-f and NN-d are fitted too when their weights are given (one shared weight set; sensitivity.py's NN route); without
weights they are refused as before.  Out of scope: CMA-ES -- cmaes.py, the derivative-free sibling --, a weight set per candidate,
sensitivities with respect to y0.  A noise model (the fit minimises the plain sum of squares) and the posterior around a fit
are mcmc.py: adaptive Metropolis, objective.population_mcmc.
"""
import numpy as np
import torch

from . import capi, steploop

FLAG_TEXT = capi.LM_FLAG_TEXT


def lm_desc(n_cand, n_prot, n_params, free, base_params, *, log_parameters, lo, hi, max_iter, gtol, xtol, ftol, rho_accept=1e-4,
            lam_max=1e16):
    """ionode_lm_desc for a fit: lo / hi [nf] in the parameters (None: no bound; with log_parameters a missing lower bound is the
    smallest normal number, the step refuses non-positive bounds)."""
    nf = len(free)
    d = capi.IonodeLmDesc(n_cand=int(n_cand), n_active=int(n_cand), n_prot=int(n_prot), n_params=int(n_params), n_free=nf,
                          log_parameters=int(bool(log_parameters)), max_iter=int(max_iter), gtol=float(gtol), xtol=float(xtol),
                          ftol=float(ftol), rho_accept=float(rho_accept), lam_max=float(lam_max))
    return steploop.fill_box(d, free, base_params, lo, hi)


def lm_init(x0, desc, lam_init):
    """(state [C, lm_state_doubles(nf)] fp64, flag [C] int32, iters [C, 2] int32, trial [C * P, NPAR] fp64) of a fit that starts at
    x0 [C, nf]: f = +inf, so the first step accepts the evaluation of the starts themselves.  numpy arrays."""
    x0 = np.ascontiguousarray(np.asarray(x0, dtype=np.float64))
    n, nf = x0.shape
    state = np.zeros((n, capi.lm_state_doubles(nf)))
    v = capi.lm_state_views(state, nf)
    v["f"][:], v["lam"][:], v["nu"][:] = np.inf, float(lam_init), 2.0
    with np.errstate(all="ignore"):
        u0 = np.log(x0) if desc.log_parameters else x0
    v["u"][:], v["ut"][:], v["x"][:], v["xt"][:] = u0, u0, x0, x0
    return state, np.zeros(n, dtype=np.int32), np.zeros((n, 2), dtype=np.int32), steploop.trial_rows(desc, x0, desc.n_prot)


def lm_step(desc, active, sse, jtr, jtj, status, state, flag, iters, trial):
    """One ionode_lm_step on torch tensors: on the current stream for device tensors, ionode_lm_step_host for CPU tensors (the same
    routine, bit for bit).  desc.n_active is set from `active` (int32 [n_active] or None: every candidate, slot = candidate)."""
    nf, P, npar = desc.n_free, desc.n_prot, desc.n_params
    n_active = desc.n_cand if active is None else int(active.shape[0])
    desc.n_active = n_active
    rows = n_active * P
    want = (("sse", sse, torch.float64, (rows,)), ("jtr", jtr, torch.float64, (rows, npar)), ("jtj", jtj, torch.float64, (rows, npar, npar)),
            ("status", status, torch.int32, (rows,)), ("state", state, torch.float64, (desc.n_cand, capi.lm_state_doubles(nf))),
            ("flag", flag, torch.int32, (desc.n_cand,)), ("iters", iters, torch.int32, (desc.n_cand, 2)),
            ("trial", trial, torch.float64, (rows, npar))) + ((("active", active, torch.int32, (n_active,)),) if active is not None else ())
    steploop.step_call("lm", desc, state.device, want, (active, sse, jtr, jtj, status, state, flag, iters, trial))


def levenberg_marquardt(model, x0, protocols_v, data_i, t_eval, *, base_params, free=(0, 1, 2, 3), log_parameters=True, bounds=None,
                        prot_t0=0.0, prot_dt=0.1, y0=(0.0, 1.0), state_dtype=torch.float32, obs_g=1.0, obs_e=-86.0,
                        obs_open_state_only=False, max_total_steps=1_000_000, max_step=0.0, rtol=1e-7, atol=1e-9, device=None, solver=None,
                        max_iter=50, gtol=1e-8, xtol=1e-8, ftol=1e-8, lam_init=1e-3, compact_every=4, callback=None, weights=None,
                        mlp_layers=0, mlp_width=0, weights_key=None):
    """Fit one batch of candidates on one device: x0 [n, nf] starting values of the free rate parameters, one fit each.

    protocols_v [P, Np], data_i [P, Nt], t_eval [Nt] (uniform: sensitivity.gauss_newton's rule), base_params [8 | 12]; bounds =
    (lo [nf], hi [nf]) in the parameters or None; log_parameters: search in log x (the reference's LogTransformation).  max_step is a
    NUMBER here (ms, 0: no cap) and is the same in every iteration, so the function being minimised does not change under the fit;
    objective.population_fit resolves "auto".  max_iter bounds the evaluations of a candidate; gtol / xtol / ftol / lam_init as
    include/ionode.h states them; compact_every: iterations between two reads of the flags (None or 0: never -- the loop then runs
    max_iter iterations).  callback(iteration, state, flag, iters) (tests, traces) sees the live tensors after every step.
    Returns (x [n, nf] fp64, sse [n] fp64, flag [n] int32 (capi.LM_*, FLAG_TEXT), iterations [n, 2] int32 = (evaluations, accepted))
    on the device: the best accepted point of every start; sse = inf and flag LM_NONFINITE where the start itself could not be
    evaluated.  `solver` (tests only): a stand-in with sensitivity.gauss_newton's signature on CPU tensors; the step is then
    ionode_lm_step_host and nothing needs a GPU.  The product default has no CPU path.
    NN models (NN-f, NN-d): with weights [n] (one flat state dict shared by every candidate), mlp_layers, mlp_width and weights_key
    (sensitivity.gauss_newton's) they are fitted like the others, `free` indexing their 8 rate parameters (NN-f: 4..7 only); without
    weights they are refused, and so is a weight set per candidate [C, n].
    Out of scope: CMA-ES and NN models without weights (cmaes.minimise), y0 sensitivities (module docstring); a noise model is mcmc.sample."""
    from . import batched, sensitivity
    if model not in (capi.MODEL_HH2, capi.MODEL_MARKOV6, capi.MODEL_NNF, capi.MODEL_NND):
        raise capi.IonodeError("fit.levenberg_marquardt: unknown model (HH 2-state and 6-state models, NN-f and NN-d with weights)")
    free = [int(f) for f in free]
    mlp = sensitivity.nn_route("fit.levenberg_marquardt", model, weights, mlp_layers, mlp_width, free)
    if mlp:
        mlp["weights_key"] = weights_key
    D, npar = capi.n_state(model), capi.n_params(model)
    nf = len(free)
    x0 = np.asarray(x0, dtype=np.float64).reshape(-1, nf) if nf else np.zeros((0, 0))
    base = np.asarray(base_params, dtype=np.float64)
    if base.shape != (npar,) or len(y0) != D:
        raise capi.IonodeError(f"model {model}: base_params [{npar}] and y0 of {D} states expected")
    if isinstance(max_step, str):
        raise capi.IonodeError("fit.levenberg_marquardt: max_step must be a number (objective.population_fit resolves 'auto' once)")
    n, P = x0.shape[0], np.asarray(protocols_v).shape[0]
    dev = batched._dev(device) if solver is None else torch.device(device or "cpu")
    solve = sensitivity.gauss_newton if solver is None else solver
    lo, hi = (None, None) if bounds is None else bounds
    desc = lm_desc(max(n, 1), P, npar, free, base, log_parameters=log_parameters, lo=lo, hi=hi, max_iter=max_iter, gtol=gtol, xtol=xtol,
                   ftol=ftol)
    if n == 0:
        return steploop.empty_result((nf,), dev)
    state, flag, iters, trial = (torch.from_numpy(a).to(dev) for a in lm_init(x0, desc, lam_init))
    pv, te, ref, pot, y0t = steploop.problem_tensors(protocols_v, t_eval, data_i, y0, n * P, state_dtype, dev)
    active, n_act = None, n
    every = int(compact_every or 0)
    for it in range(int(max_iter)):
        rows = n_act * P
        sse, jtr, jtj, status = solve(model, trial, pv, y0t[:rows], te, ref, prot_t0=prot_t0, prot_dt=prot_dt, prot_of_traj=pot[:rows],
                                      obs_g=obs_g, obs_e=obs_e, obs_open_state_only=obs_open_state_only, max_total_steps=max_total_steps,
                                      max_step=max_step, rtol=rtol, atol=atol, **mlp)
        lm_step(desc, active, sse.contiguous(), jtr.contiguous(), jtj.contiguous(), status.to(torch.int32).contiguous(), state, flag, iters,
                trial)
        if callback is not None:
            callback(it, state, flag, iters)
        if every and (it + 1) % every == 0:   # the one read: who is still running
            left = steploop.compact(flag, active, n_act, trial, capi.LM_RUNNING)
            if left is None:
                break
            active, n_act, trial = left
    v = capi.lm_state_views(state, nf)
    return v["x"].contiguous(), v["f"].contiguous(), flag, iters
