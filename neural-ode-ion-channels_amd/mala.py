"""Batched manifold MALA: many independent chains sampling the posterior of the free rate parameters (and, optionally, of the noise
level) under a Gaussian noise model, advanced together, with the Gauss-Newton matrix the library already sums as the proposal's
metric (HH 2-state and 6-state, and NN-f / NN-d with their weights: the models with a tangent sweep).

mcmc.py's adaptive Metropolis learns the shape of the posterior from its own history.  Under the Gaussian noise model J^T J / sigma^2
is the expected Fisher information -- the local metric of the posterior, at every point, from iteration 0 -- and
sensitivity.gauss_newton returns it with no trace written.  A Metropolis-adjusted Langevin step preconditioned by that metric is the
"simplified manifold MALA" of Girolami and Calderhead (2011).  One iteration of ALL chains is Levenberg-Marquardt's (fit.py):

  sensitivity.gauss_newton   on the trial tensor [n_active * P, NPAR]: the checkpointed forward with the fused sum of squares, and
                             the tangent sweep's J^T r and J^T J;
  ionode_mala_step           (csrc/ionode_mala.hpp, include/ionode.h): the tell of that evaluation -- protocol sums, log-posterior,
                             gradient, metric and its Cholesky factor, the Metropolis-Hastings decision, the step size's adaptation, a
                             recorded sample, the stop flags -- and the proposal of the next, written into the trial tensor in place.

Target and prior are mcmc.py's: a Gaussian likelihood with one noise level sigma, fixed (`sigma`) or sampled as log sigma
(`sigma_bounds`), and a prior uniform over the finite box IN THE SEARCH SPACE.  The only thing adapted is the step size (towards
target_accept = 0.574, the optimum of MALA); there is no covariance to learn.

Between the two calls there is no torch arithmetic and the step adds no host synchronisation.  Every `compact_every` iterations the
flags are read once and the chains still going are packed into the front launch slots.  The random numbers are a pure function of
(seed, chain, iteration, purpose, coordinate pair): compaction, the batch around a chain and the sharding of
objective.population_mala leave its bits alone, and the host mirror (ionode_mala_step_host) equals the kernel bit for bit.

Out of scope: HMC / NUTS, the full manifold MALA with the metric's derivatives, tempering, NN models without weights or with a weight
set per chain (sensitivity.py's NN route takes one weight set), priors other than the box, per-protocol noise, bit-compatibility with PINTS.
"""
import numpy as np
import torch

from . import capi, steploop
from .mcmc import rhat  # noqa: F401  (Gelman and Rubin's R-hat serves both samplers)

FLAG_TEXT = capi.MALA_FLAG_TEXT


def mala_desc(n_chain, n_prot, n_params, free, base_params, *, log_parameters, lo, hi, n_samples, max_iter, sigma=None, sigma_bounds=None,
              thin=1, sample_cap=None, eta=0.6, target_accept=0.574, ridge=2.0 ** -20, seed=0, chain_base=0):
    """ionode_mala_desc for a run: lo / hi [nf] in the parameters (finite; the step refuses anything else), n_samples = P * Nt
    residuals behind a chain's sum of squares.  Exactly one of sigma (fixed noise level) and sigma_bounds = (lo, hi) (sigma is
    sampled, the last coordinate).  sample_cap None: max_iter // thin + 1 rows, the start and every thin-th iteration."""
    if (sigma is None) == (sigma_bounds is None):
        raise capi.IonodeError("mala: exactly one of sigma (fixed noise) and sigma_bounds (sampled noise) must be given")
    nf = len(free)
    cap = int(max_iter) // max(int(thin), 1) + 1 if sample_cap is None else int(sample_cap)
    d = capi.IonodeMalaDesc(n_chain=int(n_chain), n_active=int(n_chain), n_prot=int(n_prot), n_params=int(n_params), n_free=nf,
                            log_parameters=int(bool(log_parameters)), sample_sigma=int(sigma is None), max_iter=int(max_iter),
                            thin=int(thin), sample_cap=cap, chain_base=int(chain_base), seed=int(seed), n_samples=float(n_samples),
                            eta=float(eta), target_accept=float(target_accept), ridge=float(ridge))
    if sigma is None:
        d.sigma_lo, d.sigma_hi = float(sigma_bounds[0]), float(sigma_bounds[1])
    else:
        d.sigma = float(sigma)
    return steploop.fill_box(d, free, base_params, lo, hi)


def mala_init(x0, desc, eps0=1.0):
    """(state [K, mala_state_doubles(n)] fp64, flag [K] int32, iters [K, 2] int32, trial [K * P, NPAR] fp64, samples [K, sample_cap,
    n + 1] fp64) of chains that start at x0 [K, n] in the parameters (n = nf, plus sigma's start as the last column when it is
    sampled; x0 [K, nf] then starts sigma at the geometric mean of its bounds): u = ut = the start in the search space, x = xt = x0,
    log_eps = log eps0.  The trial rows hold x0: the first step's evaluation is the start's.  Rows of samples that are never recorded
    stay NaN.  numpy arrays."""
    nf, ss = desc.n_free, int(desc.sample_sigma != 0)
    n = nf + ss
    x0 = np.asarray(x0, dtype=np.float64)
    if x0.ndim != 2:
        x0 = x0.reshape(-1, nf)
    if ss and x0.shape[1] == nf:
        x0 = np.concatenate([x0, np.full((x0.shape[0], 1), np.sqrt(desc.sigma_lo * desc.sigma_hi))], axis=1)
    if x0.shape[1] != n:
        raise capi.IonodeError(f"mala_init: x0 [K, {n}] expected, got {tuple(x0.shape)}")
    if not float(eps0) > 0.0 or not np.isfinite(float(eps0)):
        raise capi.IonodeError(f"mala_init: eps0 = {eps0} must be positive and finite")
    x0 = np.ascontiguousarray(x0)
    K = x0.shape[0]
    state = np.zeros((K, capi.mala_state_doubles(n)))
    v = capi.mala_state_views(state, nf, ss)
    with np.errstate(all="ignore"):
        u0 = x0.copy()
        if desc.log_parameters:
            u0[:, :nf] = np.log(x0[:, :nf])
        if ss:
            u0[:, nf] = np.log(x0[:, nf])
    v["u"][:], v["ut"][:], v["x"][:], v["xt"][:] = u0, u0, x0, x0
    v["log_eps"][:] = np.log(float(eps0))
    samples = np.full((K, max(int(desc.sample_cap), 0), n + 1), np.nan)
    return state, np.zeros(K, dtype=np.int32), np.zeros((K, 2), dtype=np.int32), steploop.trial_rows(desc, x0, desc.n_prot), samples


def mala_step(desc, active, sse, jtr, jtj, status, state, flag, iters, trial, samples=None):
    """One ionode_mala_step on torch tensors: on the current stream for device tensors, ionode_mala_step_host for CPU tensors (the same
    routine, bit for bit).  desc.n_active is set from `active` (int32 [n_active] or None: every chain, slot = chain).  samples
    [n_chain, sample_cap, n + 1] or None: nothing is recorded."""
    nf, P, npar = desc.n_free, desc.n_prot, desc.n_params
    n = nf + int(desc.sample_sigma != 0)
    n_active = desc.n_chain if active is None else int(active.shape[0])
    desc.n_active = n_active
    rows = n_active * P
    want = (("sse", sse, torch.float64, (rows,)), ("jtr", jtr, torch.float64, (rows, npar)), ("jtj", jtj, torch.float64, (rows, npar, npar)),
            ("status", status, torch.int32, (rows,)),
            ("state", state, torch.float64, (desc.n_chain, capi.mala_state_doubles(n))), ("flag", flag, torch.int32, (desc.n_chain,)),
            ("iters", iters, torch.int32, (desc.n_chain, 2)), ("trial", trial, torch.float64, (rows, npar))) \
        + ((("active", active, torch.int32, (n_active,)),) if active is not None else ()) \
        + ((("samples", samples, torch.float64, (desc.n_chain, desc.sample_cap, n + 1)),) if samples is not None else ())
    steploop.step_call("mala", desc, state.device, want, (active, sse, jtr, jtj, status, state, flag, iters, trial, samples))


def sample(model, x0, protocols_v, data_i, t_eval, *, base_params, free=(0, 1, 2, 3), log_parameters=True, bounds, sigma=None,
           sigma_bounds=None, eps0=1.0, ridge=2.0 ** -20, seed=0, max_iter=1000, thin=1, eta=0.6, target_accept=0.574, compact_every=64,
           prot_t0=0.0, prot_dt=0.1, y0=(0.0, 1.0), state_dtype=torch.float32, obs_g=1.0, obs_e=-86.0, obs_open_state_only=False,
           max_total_steps=1_000_000, max_step=0.0, rtol=1e-7, atol=1e-9, device=None, solver=None, callback=None, chain_offset=0,
           weights=None, mlp_layers=0, mlp_width=0, weights_key=None):
    """Sample the posterior of the free rate parameters given data_i with K independent manifold-MALA chains on one device: x0 [K, nf]
    (or [K, nf + 1] with sigma's start as the last column when sigma is sampled), one chain per row -- typically fit.py's optimum.

    model: HH 2-state or 6-state, or -- with weights [n] (one flat state dict shared by every chain), mlp_layers, mlp_width and
    weights_key (sensitivity.gauss_newton's) -- NN-f or NN-d, `free` indexing their 8 rate parameters (NN-f: 4..7 only); an NN model
    without weights is refused (objective.population_mcmc needs them as well), and so is a weight set per chain.  protocols_v [P, Np],
    data_i [P, Nt], t_eval [Nt] (uniform: sensitivity.gauss_newton's rule), base_params [8 | 12].  bounds = (lo [nf], hi [nf]) in the
    parameters, finite: the box is the prior -- uniform in the search space, so LOG-UNIFORM in the parameters with log_parameters.
    Exactly one of sigma (the fixed noise level of the Gaussian likelihood) and sigma_bounds = (lo, hi) (sigma is sampled as log
    sigma, log-uniform within them).  eps0: the initial step size (1 is the Langevin step of a Gaussian target in its own metric);
    it adapts as log_eps += (t + 1)^-eta (alpha - target_accept), and nothing else adapts.  ridge: the relative Marquardt diagonal
    added to the metric.  thin: every thin-th iteration is recorded.  seed, and chain_offset (the index of x0's first row among all
    chains: sharding), fix every random number.  max_step is a NUMBER here (ms, 0: no cap); objective.population_mala resolves
    "auto".  compact_every: iterations between two reads of the flags (None or 0: never).  callback(iteration, state, flag, iters)
    (tests, traces) sees the live tensors after every step.
    Returns what mcmc.sample returns: (samples [K, R, n + 1] fp64, accept_rate [K] fp64, flag [K] int32 (capi.MALA_*, FLAG_TEXT),
    iters [K, 2] int32 = (iterations, accepted)) on the device; R = max_iter // thin + 1, row r holds (x [nf], sigma if sampled,
    log-posterior) after iteration r * thin (row 0: the start); rows a stopped chain never reached are NaN.
    `solver` (tests only): a stand-in with sensitivity.gauss_newton's signature on CPU tensors; the step is then
    ionode_mala_step_host and nothing needs a GPU.  The product default has no CPU path."""
    from . import batched, sensitivity
    if model not in (capi.MODEL_HH2, capi.MODEL_MARKOV6, capi.MODEL_NNF, capi.MODEL_NND):
        raise capi.IonodeError(f"mala.sample: unknown model {model}")
    free = [int(f) for f in free]
    mlp = sensitivity.nn_route("mala.sample", model, weights, mlp_layers, mlp_width, free)
    if mlp:
        mlp["weights_key"] = weights_key
    D, npar = capi.n_state(model), capi.n_params(model)
    nf = len(free)
    if not 1 <= nf <= capi.LM_MAX_FREE:
        raise capi.IonodeError(f"mala.sample: 1 .. {capi.LM_MAX_FREE} free parameters, got {nf}")
    if (sigma is None) == (sigma_bounds is None):
        raise capi.IonodeError("mala.sample: exactly one of sigma (fixed noise) and sigma_bounds (sampled noise) must be given")
    if bounds is None:
        raise capi.IonodeError("mala.sample: bounds = (lo, hi) are required: the box is the prior")
    n = nf + int(sigma is None)
    x0 = np.asarray(x0, dtype=np.float64)
    if x0.ndim != 2:
        x0 = x0.reshape(-1, nf)
    if x0.shape[1] not in (nf, n):
        raise capi.IonodeError(f"mala.sample: x0 [K, {nf}]{' or [K, %d]' % n if n > nf else ''} expected, got {tuple(x0.shape)}")
    base = np.asarray(base_params, dtype=np.float64)
    if base.shape != (npar,) or len(y0) != D:
        raise capi.IonodeError(f"model {model}: base_params [{npar}] and y0 of {D} states expected")
    if isinstance(max_step, str):
        raise capi.IonodeError("mala.sample: max_step must be a number (objective.population_mala resolves 'auto' once)")
    K, P, Nt = x0.shape[0], np.asarray(protocols_v).shape[0], np.asarray(t_eval).shape[0]
    dev = batched._dev(device) if solver is None else torch.device(device or "cpu")
    solve = sensitivity.gauss_newton if solver is None else solver
    desc = mala_desc(max(K, 1), P, npar, free, base, log_parameters=log_parameters, lo=bounds[0], hi=bounds[1], n_samples=P * Nt,
                     max_iter=max_iter, sigma=sigma, sigma_bounds=sigma_bounds, thin=thin, eta=eta, target_accept=target_accept, ridge=ridge,
                     seed=seed, chain_base=chain_offset)
    if K == 0:
        return steploop.empty_result((desc.sample_cap, n + 1), dev)
    state, flag, iters, trial, samples = (torch.from_numpy(a).to(dev) for a in mala_init(x0, desc, eps0))
    pv, te, ref, pot, y0t = steploop.problem_tensors(protocols_v, t_eval, data_i, y0, K * P, state_dtype, dev)
    active, n_act = None, K
    every = int(compact_every or 0)
    for it in range(int(max_iter) + 1):
        rows = n_act * P
        sse, jtr, jtj, status = solve(model, trial, pv, y0t[:rows], te, ref, prot_t0=prot_t0, prot_dt=prot_dt, prot_of_traj=pot[:rows],
                                      obs_g=obs_g, obs_e=obs_e, obs_open_state_only=obs_open_state_only, max_total_steps=max_total_steps,
                                      max_step=max_step, rtol=rtol, atol=atol, **mlp)
        mala_step(desc, active, sse.contiguous(), jtr.contiguous(), jtj.contiguous(), status.to(torch.int32).contiguous(), state, flag, iters,
                  trial, samples)
        if callback is not None:
            callback(it, state, flag, iters)
        if every and it % every == 0 and it and it < int(max_iter):   # the one read: who is still running
            left = steploop.compact(flag, active, n_act, trial, capi.MALA_RUNNING)
            if left is None:
                break
            active, n_act, trial = left
    rate = iters[:, 1].double() / iters[:, 0].clamp(min=1).double()
    return samples, rate, flag, iters
