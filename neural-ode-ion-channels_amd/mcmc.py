"""Batched adaptive Metropolis: many independent chains sampling the posterior of the free rate parameters (and, optionally, of the
noise level) under a Gaussian noise model, advanced together (all four models).

Reference: what follows a CMA-ES fit of noisy data in the candidate-model workflow (train-d0.py:487-492 adds noise_sigma = 0.1 to the
synthetic data; the fits of cmaes.py and fit.py end at a point estimate).  Here every chain -- a restart for R-hat, a start point, a
seed -- owns P trajectories, and one iteration of ALL chains is two library calls on one stream:

  batched.solve            on the trial tensor [n_active * P, NPAR] with the fused objective (sse_ref=..., states=False,
                           objective="sse"): one sum of squares and one status per trajectory, no trace written;
  ionode_mcmc_step         (csrc/ionode_mcmc.hpp, include/ionode.h): the tell of that evaluation -- protocol sums, log-posterior,
                           the Metropolis decision, the adaptation of mean, covariance and scale, a recorded sample, the stop flags --
                           and the proposal of the next, written into the trial tensor in place.

The sampler is adaptive Metropolis with global adaptive scaling (Haario, Saksman, Tamminen 2001; Andrieu and Thoms 2008, Algorithm 4).
The likelihood is Gaussian with one noise level sigma for all samples, fixed (`sigma`) or sampled as log sigma (`sigma_bounds`); the
prior is uniform over the box IN THE SEARCH SPACE: with log_parameters it is log-uniform in the parameters, and it is log-uniform in a
sampled sigma.  The box must be finite, so the posterior is proper.

Between the two calls there is no torch arithmetic and no host synchronisation.  Every `compact_every` iterations the flags are read
once and the chains still going are packed into the front launch slots (the step's `active` list).  The random numbers are a pure
function of (seed, chain, iteration, purpose, coordinate pair), so a chain's samples do not depend on the others: compaction, the batch
around it and the sharding of objective.population_mcmc leave its bits alone, and the host mirror (ionode_mcmc_step_host) equals the
kernel bit for bit.

Out of scope: other samplers (DE-MC, DREAM, HMC on the existing gradients, tempering), a Laplace likelihood on the "sae" sums, priors
other than the box, per-protocol or per-sample noise, sampling MLP weights, bit-compatibility with PINTS, diagnostics beyond R-hat.
"""
import numpy as np
import torch

from . import capi, steploop

FLAG_TEXT = capi.MCMC_FLAG_TEXT


def mcmc_desc(n_chain, n_prot, n_params, free, base_params, *, log_parameters, lo, hi, n_samples, max_iter, sigma=None, sigma_bounds=None,
              adapt_start=200, thin=1, sample_cap=None, eta=0.6, target_accept=0.234, epsilon=1e-12, seed=0, chain_base=0):
    """ionode_mcmc_desc for a run: lo / hi [nf] in the parameters (finite; the step refuses anything else), n_samples = P * Nt
    residuals behind a chain's sum of squares.  Exactly one of sigma (fixed noise level) and sigma_bounds = (lo, hi) (sigma is
    sampled, the last coordinate).  sample_cap None: max_iter // thin + 1 rows, the start and every thin-th iteration."""
    if (sigma is None) == (sigma_bounds is None):
        raise capi.IonodeError("mcmc: exactly one of sigma (fixed noise) and sigma_bounds (sampled noise) must be given")
    nf = len(free)
    cap = int(max_iter) // max(int(thin), 1) + 1 if sample_cap is None else int(sample_cap)
    d = capi.IonodeMcmcDesc(n_chain=int(n_chain), n_active=int(n_chain), n_prot=int(n_prot), n_params=int(n_params), n_free=nf,
                            log_parameters=int(bool(log_parameters)), sample_sigma=int(sigma is None), max_iter=int(max_iter),
                            adapt_start=int(adapt_start), thin=int(thin), sample_cap=cap, chain_base=int(chain_base), seed=int(seed),
                            n_samples=float(n_samples), eta=float(eta), target_accept=float(target_accept), epsilon=float(epsilon))
    if sigma is None:
        d.sigma_lo, d.sigma_hi = float(sigma_bounds[0]), float(sigma_bounds[1])
    else:
        d.sigma = float(sigma)
    return steploop.fill_box(d, free, base_params, lo, hi)


def mcmc_init(x0, desc, scale=None):
    """(state [K, mcmc_state_doubles(n)] fp64, flag [K] int32, iters [K, 2] int32, trial [K * P, NPAR] fp64, samples [K, sample_cap,
    n + 1] fp64) of chains that start at x0 [K, n] in the parameters (n = nf, plus sigma's start as the last column when it is
    sampled; x0 [K, nf] then starts sigma at the geometric mean of its bounds): u = ut = mu = the start in the search space,
    x = xt = x0, C = diag(scale^2) (scale [n] or a number or None: 1), log_lambda = 0.  The trial rows hold x0: the first step's
    evaluation is the start's.  Rows of samples that are never recorded stay NaN.  numpy arrays."""
    nf, ss = desc.n_free, int(desc.sample_sigma != 0)
    n = nf + ss
    x0 = np.asarray(x0, dtype=np.float64)
    if x0.ndim != 2:
        x0 = x0.reshape(-1, nf)
    if ss and x0.shape[1] == nf:
        x0 = np.concatenate([x0, np.full((x0.shape[0], 1), np.sqrt(desc.sigma_lo * desc.sigma_hi))], axis=1)
    if x0.shape[1] != n:
        raise capi.IonodeError(f"mcmc_init: x0 [K, {n}] expected, got {tuple(x0.shape)}")
    x0 = np.ascontiguousarray(x0)
    K = x0.shape[0]
    state = np.zeros((K, capi.mcmc_state_doubles(n)))
    v = capi.mcmc_state_views(state, nf, ss)
    s = np.ones(n) * (1.0 if scale is None else np.asarray(scale, dtype=np.float64))
    with np.errstate(all="ignore"):
        u0 = x0.copy()
        if desc.log_parameters:
            u0[:, :nf] = np.log(x0[:, :nf])
        if ss:
            u0[:, nf] = np.log(x0[:, nf])
    v["u"][:], v["ut"][:], v["mu"][:], v["x"][:], v["xt"][:] = u0, u0, u0, x0, x0
    v["C"][:] = np.diag(s * s)
    samples = np.full((K, max(int(desc.sample_cap), 0), n + 1), np.nan)
    return state, np.zeros(K, dtype=np.int32), np.zeros((K, 2), dtype=np.int32), steploop.trial_rows(desc, x0, desc.n_prot), samples


def mcmc_step(desc, active, value, status, state, flag, iters, trial, samples=None):
    """One ionode_mcmc_step on torch tensors: on the current stream for device tensors, ionode_mcmc_step_host for CPU tensors (the same
    routine, bit for bit).  desc.n_active is set from `active` (int32 [n_active] or None: every chain, slot = chain).  samples
    [n_chain, sample_cap, n + 1] or None: nothing is recorded."""
    nf, P, npar = desc.n_free, desc.n_prot, desc.n_params
    n = nf + int(desc.sample_sigma != 0)
    n_active = desc.n_chain if active is None else int(active.shape[0])
    desc.n_active = n_active
    rows = n_active * P
    want = (("value", value, torch.float64, (rows,)), ("status", status, torch.int32, (rows,)),
            ("state", state, torch.float64, (desc.n_chain, capi.mcmc_state_doubles(n))), ("flag", flag, torch.int32, (desc.n_chain,)),
            ("iters", iters, torch.int32, (desc.n_chain, 2)), ("trial", trial, torch.float64, (rows, npar))) \
        + ((("active", active, torch.int32, (n_active,)),) if active is not None else ()) \
        + ((("samples", samples, torch.float64, (desc.n_chain, desc.sample_cap, n + 1)),) if samples is not None else ())
    steploop.step_call("mcmc", desc, state.device, want, (active, value, status, state, flag, iters, trial, samples))


def sample(model, x0, protocols_v, data_i, t_eval, *, base_params, free=(0, 1, 2, 3), log_parameters=True, bounds, sigma=None,
           sigma_bounds=None, scale=None, seed=0, max_iter=10000, adapt_start=200, thin=1, eta=0.6, target_accept=0.234, epsilon=1e-12,
           compact_every=64, weights=None, mlp_layers=0, mlp_width=0, weights_key=None, prot_t0=0.0, prot_dt=0.1, y0=(0.0, 1.0),
           state_dtype=torch.float32, obs_g=1.0, obs_e=-86.0, obs_open_state_only=False, max_total_steps=1_000_000, max_step=0.0, rtol=1e-7,
           atol=1e-9, device=None, solver=None, callback=None, chain_offset=0):
    """Sample the posterior of the free rate parameters given data_i with K independent adaptive-Metropolis chains on one device:
    x0 [K, nf] (or [K, nf + 1] with sigma's start as the last column when sigma is sampled), one chain per row.

    model: any of the four; the NN models take one shared weight set (weights / mlp_layers / mlp_width / weights_key as
    batched.solve) and `free` indexes the 8 rate parameters.  protocols_v [P, Np], data_i [P, Nt], t_eval [Nt], base_params [8 | 12].
    bounds = (lo [nf], hi [nf]) in the parameters, finite: the box is the prior -- uniform in the search space, so LOG-UNIFORM in the
    parameters with log_parameters (the default, the reference's LogTransformation).  Exactly one of sigma (the fixed noise level of
    the Gaussian likelihood) and sigma_bounds = (lo, hi) (sigma is sampled as log sigma, log-uniform within them).
    scale [n] | number | None: the initial proposal's standard deviations in the search space (None: 1); from adapt_start on the
    mean, the covariance and the global scale adapt with gamma = (t - adapt_start + 2)^-eta towards target_accept.  thin: every
    thin-th iteration is recorded.  seed, and chain_offset (the index of x0's first row among all chains: sharding), fix every
    random number.  max_step is a NUMBER here (ms, 0: no cap); objective.population_mcmc resolves "auto".  compact_every:
    iterations between two reads of the flags (None or 0: never).  callback(iteration, state, flag, iters) (tests, traces) sees the
    live tensors after every step.
    Returns (samples [K, R, n + 1] fp64, accept_rate [K] fp64, flag [K] int32 (capi.MCMC_*, FLAG_TEXT), iters [K, 2] int32 =
    (iterations, accepted)) on the device; R = max_iter // thin + 1, row r holds (x [nf], sigma if sampled, log-posterior) after
    iteration r * thin (row 0: the start); rows a stopped chain never reached are NaN.
    `solver` (tests only): a stand-in with batched.solve's signature on CPU tensors; the step is then ionode_mcmc_step_host and
    nothing needs a GPU.  The product default has no CPU path."""
    from . import batched
    if model not in (capi.MODEL_HH2, capi.MODEL_MARKOV6, capi.MODEL_NNF, capi.MODEL_NND):
        raise capi.IonodeError(f"mcmc.sample: unknown model {model}")
    D, npar = capi.n_state(model), capi.n_params(model)
    free = [int(f) for f in free]
    nf = len(free)
    if not 1 <= nf <= capi.LM_MAX_FREE:
        raise capi.IonodeError(f"mcmc.sample: 1 .. {capi.LM_MAX_FREE} free parameters, got {nf}")
    if (sigma is None) == (sigma_bounds is None):
        raise capi.IonodeError("mcmc.sample: exactly one of sigma (fixed noise) and sigma_bounds (sampled noise) must be given")
    if bounds is None:
        raise capi.IonodeError("mcmc.sample: bounds = (lo, hi) are required: the box is the prior")
    n = nf + int(sigma is None)
    x0 = np.asarray(x0, dtype=np.float64)
    if x0.ndim != 2:
        x0 = x0.reshape(-1, nf)
    if x0.shape[1] not in (nf, n):
        raise capi.IonodeError(f"mcmc.sample: x0 [K, {nf}]{' or [K, %d]' % n if n > nf else ''} expected, got {tuple(x0.shape)}")
    base = np.asarray(base_params, dtype=np.float64)
    if base.shape != (npar,) or len(y0) != D:
        raise capi.IonodeError(f"model {model}: base_params [{npar}] and y0 of {D} states expected")
    if isinstance(max_step, str):
        raise capi.IonodeError("mcmc.sample: max_step must be a number (objective.population_mcmc resolves 'auto' once)")
    K, P, Nt = x0.shape[0], np.asarray(protocols_v).shape[0], np.asarray(t_eval).shape[0]
    dev = batched._dev(device) if solver is None else torch.device(device or "cpu")
    solve = batched.solve if solver is None else solver
    desc = mcmc_desc(max(K, 1), P, npar, free, base, log_parameters=log_parameters, lo=bounds[0], hi=bounds[1], n_samples=P * Nt,
                     max_iter=max_iter, sigma=sigma, sigma_bounds=sigma_bounds, adapt_start=adapt_start, thin=thin, eta=eta,
                     target_accept=target_accept, epsilon=epsilon, seed=seed, chain_base=chain_offset)
    if K == 0:
        return steploop.empty_result((desc.sample_cap, n + 1), dev)
    state, flag, iters, trial, samples = (torch.from_numpy(a).to(dev) for a in mcmc_init(x0, desc, scale))
    pv, te, ref, pot, y0t = steploop.problem_tensors(protocols_v, t_eval, data_i, y0, K * P, state_dtype, dev)
    mlp = {} if weights is None else dict(weights=weights, mlp_layers=mlp_layers, mlp_width=mlp_width, weights_key=weights_key)
    active, n_act = None, K
    every = int(compact_every or 0)
    for it in range(int(max_iter) + 1):
        rows = n_act * P
        sol = solve(model, trial, pv, y0t[:rows], te, prot_t0=prot_t0, prot_dt=prot_dt, prot_of_traj=pot[:rows], obs_g=obs_g, obs_e=obs_e,
                    obs_open_state_only=obs_open_state_only, max_total_steps=max_total_steps, max_step=max_step, rtol=rtol, atol=atol,
                    device=dev, sse_ref=ref, states=False, objective="sse", **mlp)
        mcmc_step(desc, active, sol.sse.contiguous(), sol.status.to(torch.int32).contiguous(), state, flag, iters, trial, samples)
        if callback is not None:
            callback(it, state, flag, iters)
        if every and it % every == 0 and it and it < int(max_iter):   # the one read: who is still running
            left = steploop.compact(flag, active, n_act, trial, capi.MCMC_RUNNING)
            if left is None:
                break
            active, n_act, trial = left
    rate = iters[:, 1].double() / iters[:, 0].clamp(min=1).double()
    return samples, rate, flag, iters


def kept(samples, flag=None, burn=0.5):
    """The part of sampler output [K, R, n + 1] (numpy or torch) that diagnostics and predictions use, numpy [m, r, n]: the chains
    whose flag is MCMC_MAXITER (flag None: all), the rows after the first `burn` fraction, the log-posterior column left out.  One
    selection for rhat and predictive.draws."""
    s = samples.detach().cpu().numpy() if isinstance(samples, torch.Tensor) else np.asarray(samples)
    if flag is not None:
        f = flag.detach().cpu().numpy() if isinstance(flag, torch.Tensor) else np.asarray(flag)
        s = s[f == capi.MCMC_MAXITER]
    return s[:, int(np.floor(float(burn) * s.shape[1])):, :-1]


def rhat(samples, flag=None, burn=0.5):
    """Gelman and Rubin's potential scale reduction per coordinate: samples [K, R, n + 1] as `sample` returns them (numpy or torch; the
    last column, the log-posterior, is left out), over the chains whose flag is MCMC_MAXITER (flag None: all), after dropping the
    first `burn` fraction of the rows.  With m chains of r rows, W the mean of the chains' variances and B / r the variance of their
    means: sqrt(((r - 1) / r W + B / r) / W).  numpy [n]; NaN with fewer than two chains or two rows."""
    s = kept(samples, flag, burn)
    m, r = s.shape[0], s.shape[1]
    if m < 2 or r < 2:
        return np.full(s.shape[2], np.nan)
    W = s.var(axis=1, ddof=1).mean(axis=0)
    B_over_r = s.mean(axis=1).var(axis=0, ddof=1)
    with np.errstate(all="ignore"):
        return np.sqrt(((r - 1.0) / r * W + B_over_r) / W)
