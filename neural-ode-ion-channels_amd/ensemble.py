"""Batched affine-invariant ensemble sampling: E independent ensembles of W walkers sampling the posterior of the free rate parameters
(and, optionally, of the noise level) under a Gaussian noise model (all four models).

mcmc.py and mala.py run every chain alone: a chain learns the posterior's shape from its own history, or from a local metric.  Here a
walker's proposal is built from the current positions of the other walkers of its ensemble -- Goodman and Weare's stretch move (2010;
emcee's default) or ter Braak's differential-evolution move (2006), both as PINTS ships them beside the samplers this project already
has.  Nothing is tuned or adapted, and both moves are invariant under affine maps of the search space: a long, narrow, tilted
posterior costs them what a round one does.  Walkers are nearly free on this device (the fused forward solve is latency-bound), history
is not; this is the sampler that spends the former.

The walkers of an ensemble are two halves.  One HALF-iteration of ALL ensembles is two library calls on one stream:

  batched.solve            on the first E * W / 2 * P rows of the trial tensor with the fused objective (sse_ref=..., states=False,
                           objective="sse"): one sum of squares and one status per trajectory, no trace written;
  ionode_ensemble_step     (csrc/ionode_ensemble.hpp, include/ionode.h): the tell of that evaluation for the half that moved -- protocol
                           sums, log-posterior, the Metropolis-Hastings decision, after the second half a recorded sample -- and, behind
                           a workgroup barrier, the ask of the other half against the positions just told, into the trial tensor.

Likelihood, prior, box and sigma are mcmc.py's: Gaussian with one noise level, fixed (`sigma`) or sampled as log sigma
(`sigma_bounds`); uniform over the finite box IN THE SEARCH SPACE.  Between the two calls there is no torch arithmetic, and inside the
loop no host read: nothing stops early, so there are no flags to look at.  The random numbers are a pure function of (seed, ensemble,
walker, call, role), so an ensemble's samples do not depend on the others: the sharding of objective.population_ensemble leaves its
bits alone, and the host mirror (ionode_ensemble_step_host) equals the kernel bit for bit.

The W walkers of one ensemble are NOT independent chains: they share their proposals' raw material.  R-hat over all E * W walkers
(mcmc.rhat on samples.reshape(E * W, R, n + 1)) is still what the tests bound, but between-ensemble agreement is the independent
evidence; standard errors come from the E ensemble means.

Out of scope: snooker updates, mixtures of moves, parallel tempering, gradients.
"""
import ctypes as C
import math

import numpy as np
import torch

from . import capi, steploop

FLAG_TEXT = capi.ENSEMBLE_FLAG_TEXT


def ensemble_desc(n_ens, n_walkers, n_prot, n_params, free, base_params, *, log_parameters, lo, hi, n_samples, max_iter, sigma=None,
                  sigma_bounds=None, move="stretch", a=2.0, gamma=None, jitter=1e-5, thin=1, sample_cap=None, seed=0, ensemble_base=0):
    """ionode_ensemble_desc for a run: lo / hi [nf] in the parameters (finite; the step refuses anything else), n_samples = P * Nt
    residuals behind a walker's sum of squares.  Exactly one of sigma (fixed noise level) and sigma_bounds = (lo, hi) (sigma is
    sampled, the last coordinate).  move "stretch" | "de" (or capi.ENSEMBLE_*); gamma None: ter Braak's 2.38 / sqrt(2 n).
    sample_cap None: max_iter // thin + 1 rows, the start and every thin-th full iteration."""
    if (sigma is None) == (sigma_bounds is None):
        raise capi.IonodeError("ensemble: exactly one of sigma (fixed noise) and sigma_bounds (sampled noise) must be given")
    nf = len(free)
    n = nf + int(sigma is None)
    mv = capi.ENSEMBLE_MOVES.get(move, move) if isinstance(move, str) else int(move)
    if isinstance(mv, str):
        raise capi.IonodeError(f"ensemble: unknown move {move!r} (one of {sorted(capi.ENSEMBLE_MOVES)})")
    cap = int(max_iter) // max(int(thin), 1) + 1 if sample_cap is None else int(sample_cap)
    d = capi.IonodeEnsembleDesc(n_ens=int(n_ens), n_walkers=int(n_walkers), n_prot=int(n_prot), n_params=int(n_params), n_free=nf,
                                log_parameters=int(bool(log_parameters)), sample_sigma=int(sigma is None), max_iter=int(max_iter),
                                thin=int(thin), sample_cap=cap, ensemble_base=int(ensemble_base), move=mv, seed=int(seed),
                                n_samples=float(n_samples), a=float(a), gamma=2.38 / math.sqrt(2.0 * n) if gamma is None else float(gamma),
                                jitter=float(jitter))
    if sigma is None:
        d.sigma_lo, d.sigma_hi = float(sigma_bounds[0]), float(sigma_bounds[1])
    else:
        d.sigma = float(sigma)
    return steploop.fill_box(d, free, base_params, lo, hi)


def _box(desc):
    """(ulo, uhi, xlo, xhi, is_log) [n] of a descriptor: the free parameters' box, then sigma's when it is sampled; the logarithms
    are libm's, as the library forms them."""
    nf, ss = desc.n_free, int(desc.sample_sigma != 0)
    xlo, xhi = list(desc.lo[:nf]), list(desc.hi[:nf])
    is_log = [bool(desc.log_parameters)] * nf
    if ss:
        xlo, xhi, is_log = xlo + [desc.sigma_lo], xhi + [desc.sigma_hi], is_log + [True]
    with np.errstate(all="ignore"):
        ulo = np.array([math.log(v) if lg and v > 0 else (v if not lg else -np.inf) for v, lg in zip(xlo, is_log)])
        uhi = np.array([math.log(v) if lg and v > 0 else (v if not lg else -np.inf) for v, lg in zip(xhi, is_log)])
    return ulo, uhi, np.array(xlo), np.array(xhi), np.array(is_log)


def _with_sigma(x, desc):
    """starts [..., nf] -> [..., n]: sigma's start, when it is sampled and not given, is the geometric mean of its bounds."""
    nf, ss = desc.n_free, int(desc.sample_sigma != 0)
    if ss and x.shape[-1] == nf:
        x = np.concatenate([x, np.full(x.shape[:-1] + (1,), math.sqrt(desc.sigma_lo * desc.sigma_hi))], axis=-1)
    if x.shape[-1] != nf + ss:
        raise capi.IonodeError(f"ensemble: starts with {nf + ss} columns expected, got {tuple(x.shape)}")
    return x


def spread_starts(centres, desc, walkers, spread):
    """starts [E, W, n] around centres [E, nf | n] (in the parameters): walker k of ensemble e sits, IN THE SEARCH SPACE, at the centre
    plus spread (a number or [n]) times the box width times a standard normal deviate per coordinate -- the step's own counter-based
    generator under role ENSEMBLE_ROLE_SPREAD: counter (ensemble_base + e, 0, k, pair + 65536 * 3), so a walker's start does not
    depend on E or on the shard -- clipped into the box."""
    c = _with_sigma(np.asarray(centres, dtype=np.float64), desc)
    E, n = c.shape
    W = int(walkers)
    ulo, uhi, xlo, xhi, is_log = _box(desc)
    with np.errstate(all="ignore"):
        cu = np.where(is_log, np.log(c), c)
    width = np.asarray(spread, dtype=np.float64) * (uhi - ulo)
    z = np.empty((E, W, 2 * ((n + 1) // 2)))
    words, pair = (C.c_uint32 * 4)(), (C.c_double * 2)()
    draw = capi.lib().ionode_cmaes_draw_host
    for e in range(E):
        for k in range(W):
            for jp in range((n + 1) // 2):
                draw(int(desc.seed), int(desc.ensemble_base) + e, 0, k, jp, capi.ENSEMBLE_ROLE_SPREAD, C.byref(words), C.byref(pair))
                z[e, k, 2 * jp], z[e, k, 2 * jp + 1] = pair[0], pair[1]
    u = np.minimum(np.maximum(cu[:, None, :] + width * z[:, :, :n], ulo), uhi)
    return np.minimum(np.maximum(np.where(is_log, np.exp(u), u), xlo), xhi)


def ensemble_init(starts, desc):
    """(state [E, W, ensemble_state_doubles(n)] fp64, flag [E] int32, iters [E, 2] int32, accepted [E, W] int32, trial [E * W * P, NPAR]
    fp64, samples [E, W, sample_cap, n + 1] fp64) of ensembles whose walkers start at starts [E, W, n] in the parameters (n = nf, plus
    sigma's start as the last column when it is sampled; [E, W, nf] then starts every sigma at the geometric mean of its bounds --
    which no move can leave: give sigma a spread): u = ut = the starts in the search space, x = xt = the starts, the trial rows hold
    them: the first step's evaluation is the starts'.  Rows of samples that are never recorded stay NaN.  numpy arrays.
    A start on the box's edge is moved inside by the rounding of its own logarithm, never out."""
    nf, ss = desc.n_free, int(desc.sample_sigma != 0)
    n = nf + ss
    x0 = np.asarray(starts, dtype=np.float64)
    if x0.ndim != 3:
        raise capi.IonodeError(f"ensemble_init: starts [E, W, {n}] expected, got {tuple(x0.shape)}")
    x0 = np.ascontiguousarray(_with_sigma(x0, desc))
    E, W = x0.shape[:2]
    ulo, uhi, xlo, xhi, is_log = _box(desc)
    with np.errstate(all="ignore"):
        u0 = np.where(is_log, np.log(x0), x0)
    edge = (x0 >= xlo) & (x0 <= xhi)
    u0 = np.where(edge, np.minimum(np.maximum(u0, ulo), uhi), u0)
    state = np.zeros((E, W, capi.ensemble_state_doubles(n)))
    v = capi.ensemble_state_views(state, nf, ss)
    v["u"][:], v["ut"][:], v["x"][:], v["xt"][:] = u0, u0, x0, x0
    samples = np.full((E, W, max(int(desc.sample_cap), 0), n + 1), np.nan)
    return (state, np.zeros(E, dtype=np.int32), np.zeros((E, 2), dtype=np.int32), np.zeros((E, W), dtype=np.int32),
            steploop.trial_rows(desc, x0.reshape(E * W, n), desc.n_prot), samples)


def check_spans(starts, desc):
    """Refuse starts [E, W, n] of which a half does not affinely span the search space: the differences of a half's points, each
    coordinate measured in box widths, must have rank n.  Both moves keep every walker in the affine hull of its own half's and its
    partners' points for ever -- W equal walkers are a fixed point."""
    x = _with_sigma(np.asarray(starts, dtype=np.float64), desc)
    E, W, n = x.shape
    ulo, uhi, _, _, is_log = _box(desc)
    with np.errstate(all="ignore"):
        u = np.where(is_log, np.log(x), x)
    with np.errstate(all="ignore"):
        width = np.where(np.isfinite(uhi - ulo) & (uhi > ulo), uhi - ulo, 1.0)   # (a box the step will refuse is not judged here)
    for e in range(E):
        for h in range(2):
            pts = u[e, h * (W // 2):(h + 1) * (W // 2)]
            if not np.isfinite(pts).all():
                continue   # (the step flags it: IONODE_ENSEMBLE_NONFINITE)
            distinct = len(np.unique(pts, axis=0))
            rank = np.linalg.matrix_rank((pts[1:] - pts[0]) / width) if len(pts) > 1 else 0
            if distinct < n + 1 or rank < n:
                raise capi.IonodeError(f"ensemble: half {h} of ensemble {e} is degenerate: {distinct} distinct points of rank {rank}, "
                                       f"{n + 1} affinely independent ones are needed (walkers=, spread=: a cloud around one start)")


def ensemble_step(desc, value, status, state, flag, iters, accepted, trial, samples=None):
    """One ionode_ensemble_step on torch tensors: on the current stream for device tensors, ionode_ensemble_step_host for CPU tensors
    (the same routine, bit for bit).  value / status: E * W * P rows at an ensemble's first call, E * W / 2 * P after (either length
    is accepted here: the caller knows which call it is).  samples [E, W, sample_cap, n + 1] or None: nothing is recorded."""
    nf, P, npar, E, W = desc.n_free, desc.n_prot, desc.n_params, desc.n_ens, desc.n_walkers
    n = nf + int(desc.sample_sigma != 0)
    rows = int(value.shape[0]) if isinstance(value, torch.Tensor) and value.dim() == 1 else -1
    if rows not in (E * W * P, E * (W // 2) * P):
        raise capi.IonodeError(f"ensemble_step: value: {E * W * P} rows (the starts) or {E * (W // 2) * P} (a half) expected")
    want = (("value", value, torch.float64, (rows,)), ("status", status, torch.int32, (rows,)),
            ("state", state, torch.float64, (E, W, capi.ensemble_state_doubles(n))), ("flag", flag, torch.int32, (E,)),
            ("iters", iters, torch.int32, (E, 2)), ("accepted", accepted, torch.int32, (E, W)), ("trial", trial, torch.float64, (E * W * P, npar))) \
        + ((("samples", samples, torch.float64, (E, W, desc.sample_cap, n + 1)),) if samples is not None else ())
    steploop.step_call("ensemble", desc, state.device, want, (value, status, state, flag, iters, accepted, trial, samples))


def sample(model, starts, protocols_v, data_i, t_eval, *, base_params, free=(0, 1, 2, 3), log_parameters=True, bounds, sigma=None,
           sigma_bounds=None, move="stretch", a=2.0, gamma=None, jitter=1e-5, walkers=None, spread=1e-3, seed=0, max_iter=1000, thin=1,
           weights=None, mlp_layers=0, mlp_width=0, weights_key=None, prot_t0=0.0, prot_dt=0.1, y0=(0.0, 1.0), state_dtype=torch.float32,
           obs_g=1.0, obs_e=-86.0, obs_open_state_only=False, max_total_steps=1_000_000, max_step=0.0, rtol=1e-7, atol=1e-9, device=None,
           solver=None, callback=None, ensemble_offset=0):
    """Sample the posterior of the free rate parameters given data_i with E independent ensembles of W walkers on one device.

    starts [E, W, nf] (or [E, W, nf + 1] with sigma's start as the last column when sigma is sampled): every walker's start; or
    [E, nf] (or [E, nf + 1]) with walkers=W: one centre per ensemble, its walkers spread around it by spread_starts (spread: a
    number or [n], in box widths of the search space).  W is even and at least 2 (n + 1); a start whose half does not affinely span
    the search space is refused (check_spans).
    model, protocols_v, data_i, t_eval, base_params, free, log_parameters, bounds, sigma / sigma_bounds, the NN models' weights, the
    solve's settings and `solver`: as mcmc.sample.  move "stretch" (a: the stretch scale, 2) or "de" (gamma: None is 2.38 /
    sqrt(2 n); jitter: the added noise's standard deviation in the search space, 0 allowed).  max_iter counts FULL iterations (both
    halves move once): 2 max_iter + 1 solves, the first of E W P trajectories, the others of E W / 2 P.  seed, and ensemble_offset
    (the index of starts' first ensemble among all ensembles: sharding), fix every random number.  callback(call, state, flag, iters,
    accepted) (tests, traces) sees the live tensors after every step.
    Returns (samples [E, W, R, n + 1] fp64, acceptance [E, W] fp64, flag [E] int32 (capi.ENSEMBLE_*, FLAG_TEXT), iters [E, 2] int32 =
    (calls, full iterations)) on the device; R = max_iter // thin + 1, row r holds (x [nf], sigma if sampled, log-posterior) after
    full iteration r * thin (row 0: the start); the rows of an ensemble that was flagged at its start stay NaN after row 0.
    mcmc.rhat(samples.reshape(E * W, R, n + 1)) is Gelman and Rubin's R-hat over all walkers -- which, within an ensemble, are not
    independent chains."""
    from . import batched
    if model not in (capi.MODEL_HH2, capi.MODEL_MARKOV6, capi.MODEL_NNF, capi.MODEL_NND):
        raise capi.IonodeError(f"ensemble.sample: unknown model {model}")
    D, npar = capi.n_state(model), capi.n_params(model)
    free = [int(f) for f in free]
    nf = len(free)
    if not 1 <= nf <= capi.LM_MAX_FREE:
        raise capi.IonodeError(f"ensemble.sample: 1 .. {capi.LM_MAX_FREE} free parameters, got {nf}")
    if (sigma is None) == (sigma_bounds is None):
        raise capi.IonodeError("ensemble.sample: exactly one of sigma (fixed noise) and sigma_bounds (sampled noise) must be given")
    if bounds is None:
        raise capi.IonodeError("ensemble.sample: bounds = (lo, hi) are required: the box is the prior")
    n = nf + int(sigma is None)
    x0 = np.asarray(starts, dtype=np.float64)
    if x0.ndim == 2 and walkers is None:
        raise capi.IonodeError("ensemble.sample: starts [E, nf] are centres and need walkers=W; or give every walker's start [E, W, nf]")
    if x0.ndim not in (2, 3) or x0.shape[-1] not in (nf, n):
        raise capi.IonodeError(f"ensemble.sample: starts [E, W, {nf}]{' or [E, W, %d]' % n if n > nf else ''} (or centres [E, .] with walkers=) "
                               f"expected, got {tuple(x0.shape)}")
    E = x0.shape[0]
    W = int(walkers) if x0.ndim == 2 else x0.shape[1]
    if walkers is not None and x0.ndim == 3 and int(walkers) != W:
        raise capi.IonodeError(f"ensemble.sample: walkers = {walkers} but starts hold {W} per ensemble")
    base = np.asarray(base_params, dtype=np.float64)
    if base.shape != (npar,) or len(y0) != D:
        raise capi.IonodeError(f"model {model}: base_params [{npar}] and y0 of {D} states expected")
    if isinstance(max_step, str):
        raise capi.IonodeError("ensemble.sample: max_step must be a number (objective.population_ensemble resolves 'auto' once)")
    if W < 2 * (n + 1) or W % 2:
        raise capi.IonodeError(f"ensemble.sample: {W} walkers: an even number of at least 2 (n + 1) = {2 * (n + 1)} is needed")
    P, Nt = np.asarray(protocols_v).shape[0], np.asarray(t_eval).shape[0]
    dev = batched._dev(device) if solver is None else torch.device(device or "cpu")
    solve = batched.solve if solver is None else solver
    desc = ensemble_desc(max(E, 1), W, P, npar, free, base, log_parameters=log_parameters, lo=bounds[0], hi=bounds[1], n_samples=P * Nt,
                         max_iter=max_iter, sigma=sigma, sigma_bounds=sigma_bounds, move=move, a=a, gamma=gamma, jitter=jitter, thin=thin,
                         seed=seed, ensemble_base=ensemble_offset)
    if E == 0:
        smp, _, flag, iters = steploop.empty_result((W, desc.sample_cap, n + 1), dev)
        return smp, torch.zeros((0, W), dtype=torch.float64, device=dev), flag, iters
    if x0.ndim == 2:
        x0 = spread_starts(x0, desc, W, spread)
    check_spans(x0, desc)
    state, flag, iters, accepted, trial, samples = (torch.from_numpy(a_).to(dev) for a_ in ensemble_init(x0, desc))
    pv, te, ref, pot, y0t = steploop.problem_tensors(protocols_v, t_eval, data_i, y0, E * W * P, state_dtype, dev)
    mlp = {} if weights is None else dict(weights=weights, mlp_layers=mlp_layers, mlp_width=mlp_width, weights_key=weights_key)
    half = E * (W // 2) * P
    for call in range(2 * int(max_iter) + 1):
        rows = E * W * P if call == 0 else half
        sol = solve(model, trial[:rows], pv, y0t[:rows], te, prot_t0=prot_t0, prot_dt=prot_dt, prot_of_traj=pot[:rows], obs_g=obs_g, obs_e=obs_e,
                    obs_open_state_only=obs_open_state_only, max_total_steps=max_total_steps, max_step=max_step, rtol=rtol, atol=atol,
                    device=dev, sse_ref=ref, states=False, objective="sse", **mlp)
        ensemble_step(desc, sol.sse.contiguous(), sol.status.to(torch.int32).contiguous(), state, flag, iters, accepted, trial, samples)
        if callback is not None:
            callback(call, state, flag, iters, accepted)
    rate = accepted.double() / iters[:, 1:2].clamp(min=1).double()
    return samples, rate, flag, iters
