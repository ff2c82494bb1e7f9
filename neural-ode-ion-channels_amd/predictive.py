"""Posterior predictive bands of the current: per protocol and per output sample, the mean, the spread and exact quantiles of i(t)
over parameter draws -- and, with sigma, of i(t) + noise: the prediction band one draws over the data.

Reference: the candidate-model workflow ends at a point estimate (train-d0.py:487-540); mcmc.sample, mala.sample and ensemble.sample
give draws of the posterior, and this module is their consumer.  The draws are solved in chunks, and of each chunk's current traces
[n * P, Nt] only running moments [P, Nt] and -- for quantiles -- one column of draws per (protocol, sample) stay:

  batched.solve                  on the chunk's rows [n * P, NPAR] (candidate-major: row = draw * P + protocol, the trial tensors'
                                 layout) with current=True, states=False (and the fused objective against a zero reference, whose
                                 sum is not used: the solve stores states unless that objective is on);
  ionode_predictive_accumulate   (csrc/ionode_predictive.hpp, include/ionode.h) on the same stream: Welford's update of mean and m2,
                                 min, max, the surviving draws' count per protocol, and the chunk's values transposed into the column
                                 store cols [P, Nt, S];
  ionode_predictive_quantiles    once, at the end: every column sorted in LDS, the requested order statistics interpolated.

There is no host read in the loop.  A draw whose solve fails (status != 0) is left out of its protocol's moments and count; its slot
of the column store sorts behind every value.  Every element walks its draws in ascending index and the noise is a function of
(seed, draw, protocol, sample), so the result does not depend on chunk_bytes, bit for bit, and the host mirrors
(ionode_predictive_*_host, CPU tensors) equal the kernels bit for bit.

Out of scope: weighted draws, approximate (sketch) quantiles above capi.PREDICTIVE_MAX_DRAWS draws, bands of the states, posteriors
over MLP weights.
"""
import ctypes as C
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from . import capi, mcmc


@dataclass
class Bands:
    mean: torch.Tensor                   # [P, Nt] fp64; NaN where count is 0
    sd: torch.Tensor                     # [P, Nt] sqrt(m2 / (count - 1)); NaN where count < 2
    min: torch.Tensor                    # [P, Nt]
    max: torch.Tensor                    # [P, Nt]
    quantiles: Optional[torch.Tensor]    # [P, Q, Nt], or None when none was asked for
    count: torch.Tensor                  # [P] int64: the draws whose solve of protocol p succeeded
    n_draws: int                         # draws given
    q: tuple                             # the Q probabilities
    m2: torch.Tensor                     # [P, Nt] sum of squared deviations from the mean (what merges across shards)


def draws(samples, flag=None, burn=0.5, thin=1, max_draws=None):
    """Pool sampler output samples [K, R, n + 1] (mcmc.sample, mala.sample; ensemble.sample's reshaped to [E * W, R, n + 1]) into draws
    [S, n] (numpy): mcmc.kept's selection -- the chains whose flag is the iteration cap (flag None: all), the rows after the first
    `burn` fraction, the log-posterior column dropped: what mcmc.rhat judges -- then every thin-th row of each chain, chain after
    chain, rows with a NaN (a stopped chain's tail) dropped, and with max_draws an evenly spaced subset of at most that many.  The
    rows are what the samplers record: the free PARAMETERS, then sigma when it was sampled."""
    if int(thin) < 1:
        raise capi.IonodeError(f"predictive.draws: thin = {thin} < 1")
    s = mcmc.kept(samples, flag, burn)[:, ::int(thin)]
    s = s.reshape(-1, s.shape[2])
    s = s[~np.isnan(s).any(axis=1)]
    if max_draws is not None and s.shape[0] > int(max_draws):
        if int(max_draws) < 1:
            raise capi.IonodeError(f"predictive.draws: max_draws = {max_draws} < 1")
        s = s[np.floor(np.arange(int(max_draws)) * (s.shape[0] / int(max_draws))).astype(np.int64)]
    return np.ascontiguousarray(s)


# ---- the two passes on torch tensors ----

def new_state(n_prot, n_out, s_cap, device, store=True):
    """Fresh state of an accumulation: dict of mean, m2 (zeros), min (+inf), max (-inf) [P, Nt] fp64, count [P] int64 and, with
    `store`, cols [P, Nt, s_cap] fp64 (+inf: an unwritten slot sorts last)."""
    dev = torch.device(device)
    z = lambda v: torch.full((n_prot, n_out), v, dtype=torch.float64, device=dev)
    return {"mean": z(0.0), "m2": z(0.0), "min": z(float("inf")), "max": z(float("-inf")),
            "count": torch.zeros(n_prot, dtype=torch.int64, device=dev), "s_cap": int(s_cap),
            "cols": torch.full((n_prot, n_out, int(s_cap)), float("inf"), dtype=torch.float64, device=dev) if store else None}


def _check(name, what, t, dtype, shape, dev):
    if not isinstance(t, torch.Tensor) or t.dtype != dtype or tuple(t.shape) != shape or not t.is_contiguous() or t.device != dev:
        raise capi.IonodeError(f"{name}: {what}: expected a contiguous {dtype} tensor {shape} on {dev}")


def accumulate(state, trace, status, *, draw_base, sigma=None, noise=False, seed=0, draw_offset=0):
    """One ionode_predictive_accumulate: fold trace [n * P, Nt] fp64 with status [n * P] int32 (row = draw * P + protocol) into
    `state` (new_state), as the draws draw_base .. draw_base + n - 1.  sigma: None, a number, or an fp64 tensor [>= draw_base + n] of
    per-draw noise levels indexed by draw; noise=True accumulates and stores i + sigma z.  draw_offset: the index of draw 0 among all
    draws of a sharded run (the generator's counter).  On the current stream for device tensors, the host mirror for CPU tensors."""
    P, Nt = state["mean"].shape
    dev = state["mean"].device
    if trace.dim() != 2 or trace.shape[1] != Nt or trace.shape[0] % P or trace.shape[0] == 0:
        raise capi.IonodeError(f"predictive.accumulate: trace [n * {P}, {Nt}] expected, got {tuple(trace.shape)}")
    n = trace.shape[0] // P
    _check("predictive.accumulate", "trace", trace, torch.float64, (n * P, Nt), dev)
    _check("predictive.accumulate", "status", status, torch.int32, (n * P,), dev)
    d = capi.IonodePredictiveDesc(n_prot=P, n_out=Nt, n_draw=n, s_cap=state["s_cap"], draw_base=int(draw_base), draw_offset=int(draw_offset),
                                  noise=int(bool(noise)), seed=int(seed), sigma=float("nan"))
    sig = None
    if isinstance(sigma, torch.Tensor):
        if sigma.dtype != torch.float64 or sigma.dim() != 1 or sigma.shape[0] < int(draw_base) + n or not sigma.is_contiguous() or sigma.device != dev:
            raise capi.IonodeError(f"predictive.accumulate: sigma: expected a contiguous fp64 tensor of at least {int(draw_base) + n} draws on {dev}")
        sig = sigma
    elif sigma is not None:
        d.sigma = float(sigma)
    args = [trace, status, sig, state["mean"], state["m2"], state["min"], state["max"], state["count"], state["cols"]]
    ptrs = [None if t is None else C.c_void_p(t.data_ptr()) for t in args]
    if dev.type == "cuda":
        rc = capi.lib().ionode_predictive_accumulate(C.byref(d), *ptrs, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    else:
        rc = capi.lib().ionode_predictive_accumulate_host(C.byref(d), *ptrs)
    if rc != 0:
        raise capi.IonodeError(f"ionode_predictive_accumulate failed ({rc}): {capi.lib().ionode_grad_last_error().decode()}")


def quantile_pass(state, q):
    """One ionode_predictive_quantiles: quant [P, Q, Nt] fp64 of the state's column store and count."""
    P, Nt = state["mean"].shape
    dev = state["mean"].device
    if state["cols"] is None:
        raise capi.IonodeError("predictive.quantile_pass: the state has no column store (new_state(store=False))")
    qa = (C.c_double * len(q))(*[float(x) for x in q])
    quant = torch.empty((P, len(q), Nt), dtype=torch.float64, device=dev)
    ptrs = [C.c_void_p(state["count"].data_ptr()), C.c_void_p(state["cols"].data_ptr()), C.c_void_p(quant.data_ptr())]
    head = (P, Nt, state["s_cap"], len(q), C.cast(qa, C.c_void_p))
    if dev.type == "cuda":
        rc = capi.lib().ionode_predictive_quantiles(*head, *ptrs, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    else:
        rc = capi.lib().ionode_predictive_quantiles_host(*head, *ptrs)
    if rc != 0:
        raise capi.IonodeError(f"ionode_predictive_quantiles failed ({rc}): {capi.lib().ionode_grad_last_error().decode()}")
    return quant


def finish(state, q, n_draws, quant=None):
    """Bands of an accumulated state: sd = sqrt(m2 / (count - 1)), NaN below two surviving draws; mean, min and max NaN for none."""
    nan = torch.full_like(state["mean"], float("nan"))
    cnt = state["count"][:, None]
    some = cnt > 0
    sd = torch.where(cnt > 1, torch.sqrt(state["m2"] / (cnt - 1).clamp(min=1).double()), nan)
    return Bands(mean=torch.where(some, state["mean"], nan), sd=sd, min=torch.where(some, state["min"], nan),
                 max=torch.where(some, state["max"], nan), quantiles=quant, count=state["count"], n_draws=int(n_draws), q=tuple(q),
                 m2=state["m2"])


def parameters(draws, n_free, *, log_parameters=True, coordinates="parameters"):
    """(x [S, n_free], sigma [S] or None) in the parameters from draws [S, n_free] or [S, n_free + 1] (sigma last).  coordinates
    "parameters": the rows are what the samplers record, x and sigma themselves; "search": the samplers' search space, u = log x
    under log_parameters, log sigma always -- converted with exp, as the steps convert a proposal."""
    d = np.asarray(draws.detach().cpu() if isinstance(draws, torch.Tensor) else draws, dtype=np.float64)
    if d.ndim != 2 or d.shape[1] not in (n_free, n_free + 1):
        raise capi.IonodeError(f"predictive: draws [S, {n_free}] or [S, {n_free + 1}] (sigma last) expected for {n_free} free parameters, "
                               f"got {tuple(d.shape)}")
    if coordinates not in ("parameters", "search"):
        raise capi.IonodeError("predictive: coordinates must be 'parameters' or 'search'")
    x, sig = d[:, :n_free], (d[:, n_free] if d.shape[1] > n_free else None)
    if coordinates == "search":
        x = np.exp(x) if log_parameters else x
        sig = None if sig is None else np.exp(sig)
    return np.ascontiguousarray(x), sig


def bands(model, draws, protocols_v, t_eval, *, base_params, free=(0, 1, 2, 3), log_parameters=True, coordinates="parameters", sigma=None,
          quantiles=(0.025, 0.5, 0.975), noise=False, seed=0, chunk_bytes=1 << 30, budget_bytes=32 << 30, solver=None, draw_offset=0,
          weights=None, mlp_layers=0, mlp_width=0, weights_key=None, prot_t0=0.0, prot_dt=0.1, y0=(0.0, 1.0), state_dtype=torch.float32,
          obs_g=1.0, obs_e=-86.0, obs_open_state_only=False, max_total_steps=1_000_000, max_step=0.0, rtol=1e-7, atol=1e-9, device=None):
    """Posterior predictive bands of the current over draws [S, nf] (or [S, nf + 1], the last column each draw's sigma), on one device.

    model, protocols_v [P, Np], t_eval [Nt], base_params, free and the solve keywords: as mcmc.sample.  The draws are rows of
    predictive.draws -- the free parameters as the samplers record them; coordinates="search" takes the samplers' search space instead
    (log x under log_parameters, log sigma) -- and row s becomes the trial rows s * P .. s * P + P - 1: base_params with the free columns
    replaced, exactly as the samplers' trial tensor is laid out.  sigma: a number for all draws when the draws carry none.
    noise=True gives the bands of i + sigma z (refused without any sigma); seed fixes z.  quantiles: probabilities in [0, 1], at most
    capi.PREDICTIVE_MAX_Q (None or empty: moments only, no column store and no cap on S).  With quantiles S is at most
    capi.PREDICTIVE_MAX_DRAWS and the column store 8 P Nt S bytes at most budget_bytes: both refused by name (capi.predictive_plan).
    chunk_bytes: the draws are solved in chunks whose current trace [n * P, Nt] fp64 stays within it (at least one draw a chunk).  A
    solve's time is set by the length of a trajectory far more than by their number, so a chunk costs about one solve whatever its
    size (profiles/predictive.md): the default of 1 GiB keeps the chunks few; lower it where memory is short.
    max_step is a NUMBER here; objective.population_predictive resolves "auto".  draw_offset: index of draws[0] among all draws of a
    sharded run.  Returns Bands (tensors on the device).
    `solver` (tests only): a stand-in with batched.solve's signature on CPU tensors; the passes then run as the host mirrors."""
    from . import batched
    if model not in (capi.MODEL_HH2, capi.MODEL_MARKOV6, capi.MODEL_NNF, capi.MODEL_NND):
        raise capi.IonodeError(f"predictive.bands: unknown model {model}")
    D, npar = capi.n_state(model), capi.n_params(model)
    free = [int(f) for f in free]
    base = np.asarray(base_params, dtype=np.float64)
    if base.shape != (npar,) or len(y0) != D:
        raise capi.IonodeError(f"model {model}: base_params [{npar}] and y0 of {D} states expected")
    if isinstance(max_step, str):
        raise capi.IonodeError("predictive.bands: max_step must be a number (objective.population_predictive resolves 'auto' once)")
    x, sig = parameters(draws, len(free), log_parameters=log_parameters, coordinates=coordinates)
    if sig is not None and sigma is not None:
        raise capi.IonodeError("predictive.bands: the draws carry sigma as their last column and `sigma` is given too: one of them")
    if noise and sig is None and sigma is None:
        raise capi.IonodeError("predictive.bands: noise without sigma: give `sigma` or draws with sigma as their last column")
    q = tuple(float(v) for v in (quantiles if quantiles is not None else ()))
    if any(not 0.0 <= v <= 1.0 for v in q):
        raise capi.IonodeError(f"predictive.bands: quantiles {q}: every q must lie in [0, 1]")
    if len(q) > capi.PREDICTIVE_MAX_Q:
        raise capi.IonodeError(f"predictive.bands: {len(q)} quantiles, at most {capi.PREDICTIVE_MAX_Q}")
    S, P, Nt = x.shape[0], np.asarray(protocols_v).shape[0], np.asarray(t_eval).shape[0]
    if S < 1:
        raise capi.IonodeError("predictive.bands: no draws")
    if q:
        capi.predictive_plan(P, Nt, S, budget_bytes)   # refuses S above the cap and a store above the budget, before anything is allocated
    dev = batched._dev(device) if solver is None else torch.device(device or "cpu")
    solve = batched.solve if solver is None else solver
    rows = np.tile(base, (S, 1))
    rows[:, free] = x
    params = torch.from_numpy(rows).to(dev)
    sig_t = None if sig is None else torch.from_numpy(np.ascontiguousarray(sig)).to(dev)
    pv = torch.as_tensor(np.asarray(protocols_v), dtype=torch.float64, device=dev).contiguous()
    te = torch.as_tensor(np.asarray(t_eval), dtype=torch.float64, device=dev).contiguous()
    n_chunk = int(max(1, min(S, int(chunk_bytes) // (8 * P * Nt))))
    pot = torch.from_numpy(np.tile(np.arange(P, dtype=np.int32), n_chunk)).to(dev)
    y0t = torch.tensor([list(y0)], dtype=state_dtype, device=dev).expand(n_chunk * P, len(y0)).contiguous()
    mlp = {} if weights is None else dict(weights=weights, mlp_layers=mlp_layers, mlp_width=mlp_width, weights_key=weights_key)
    # the solve writes a trajectory's states unless the fused objective is on: a zero reference turns it on -- one unused sum of i^2 a
    # trajectory -- and spares the [n * P, Nt, D] state trace, twice the bytes of the current trace this loop is after
    zero_ref = torch.zeros((P, Nt), dtype=torch.float64, device=dev)
    state = new_state(P, Nt, S, dev, store=bool(q))
    for lo in range(0, S, n_chunk):
        n = min(n_chunk, S - lo)
        sol = solve(model, params[lo:lo + n].repeat_interleave(P, dim=0), pv, y0t[:n * P], te, prot_t0=prot_t0, prot_dt=prot_dt,
                    prot_of_traj=pot[:n * P], obs_g=obs_g, obs_e=obs_e, obs_open_state_only=obs_open_state_only,
                    max_total_steps=max_total_steps, max_step=max_step, rtol=rtol, atol=atol, device=dev, current=True, states=False, sse_ref=zero_ref, **mlp)
        accumulate(state, sol.i.contiguous(), sol.status.to(torch.int32).contiguous(), draw_base=lo, sigma=sig_t if sig_t is not None else sigma,
                   noise=noise, seed=seed, draw_offset=draw_offset)
    return finish(state, q, S, quantile_pass(state, q) if q else None)
