"""Batched multi-exponential fits of a(t) segments: every constant-voltage segment of a protocol, each restarted a few times, fitted by
CMA-ES runs that advance together.

Reference: the real-data route (train-r1.py / train-r2.py) fits a tri- or bi-exponential per segment (train-r1.py:427-451, :487-494:
f = sqrt(mean((model - a)^2)), scipy's simplex) and hands its hardest segments, the -90 mV steps, to PINTS' CMA-ES
(`pints.fmin(f, x02, method=pints.CMAES)`, train-r1.py:553-555, :641 with max_iter 1000; train-r2.py:595, :671) -- in the parameters
themselves, no transformation, no box.  Here a run is (segment, restart); one generation of ALL runs is two library calls on one
stream:

  ionode_multi_exp_objective   (csrc/ionode_expfit.hpp, include/ionode.h "Multi-exponential fits"): the RMSE of every row of the
                               trial tensor [n_active * lambda, n_params] against its run's segment, one 256-lane workgroup per row;
  cmaes.cmaes_step             ionode_cmaes_step with n_prot = 1, n_free = n_params, log_parameters = 0: the tell of that
                               generation and the ask of the next, written into the trial tensor in place.

Between the two there is no torch arithmetic and no host read.  Every `compact_every` generations the flags are read once and the
runs still going are packed into the front launch slots (steploop.compact).  A run's random numbers are a function of (seed, its
run index, generation, candidate, ...), and the objective of a row depends on that row and its segment only: a run's iterates do
not depend on compaction or on the runs around it, and the CPU path (device="cpu": the host mirrors, for tests) equals the GPU's
bit for bit.

This project's choices, not PINTS' (its fmin defaults cannot be checked here; bit-compatibility with PINTS is out of scope as in
cmaes.py): sigma0 = 1/6 with the per-coordinate scale |x0| (a zero coordinate: 1), i.e. an initial standard deviation of a sixth of
each start value; stops after unchanged_iters = 200 generations without an improvement of more than unchanged_threshold = 1e-11,
at a step size below tolx = 1e-11, at the step's condition limit, or after max_iter = 1000 generations (train-r1.py:641's).
Out of scope: splines and smoothing (preprocess.py), more than three exponentials, fits across segment boundaries, bounds or a log
transform for these fits.
"""
import ctypes as C

import numpy as np
import torch

from . import capi, cmaes, steploop

FLAG_TEXT = capi.CMAES_FLAG_TEXT


def _device(device):
    if device is not None and torch.device(device).type == "cpu":
        return torch.device("cpu")
    from . import batched
    return batched._dev(device)


def _stream(dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _check(rc, name):
    if rc != 0:
        raise capi.IonodeError(f"{name} failed ({rc}): {capi.lib().ionode_grad_last_error().decode()}")


def _ragged(arrays):
    """(offsets int64 [len + 1], the arrays concatenated fp64)."""
    arrays = [np.asarray(x, dtype=np.float64).reshape(-1) for x in arrays]
    off = np.zeros(len(arrays) + 1, dtype=np.int64)
    np.cumsum([x.size for x in arrays], out=off[1:])
    return off, (np.concatenate(arrays) if arrays else np.zeros(0))


def objective(n_run, lam, n_params, active, seg_of_run, seg_off, t_rel, a, trial, value, status):
    """One ionode_multi_exp_objective on torch tensors: on the current stream for device tensors, the host mirror for CPU tensors.
    active int32 [n_active] or None; trial [n_active * lam, n_params] fp64; value fp64 / status int32 [n_active * lam] are written."""
    dev = trial.device
    n_active = n_run if active is None else int(active.shape[0])
    rows = n_active * lam
    want = (("seg_of_run", seg_of_run, torch.int32, (n_run,)), ("seg_off", seg_off, torch.int64, None), ("t_rel", t_rel, torch.float64, None),
            ("a", a, torch.float64, tuple(t_rel.shape)), ("trial", trial, torch.float64, (rows, n_params)), ("value", value, torch.float64, (rows,)),
            ("status", status, torch.int32, (rows,))) + ((("active", active, torch.int32, (n_active,)),) if active is not None else ())
    for what, t, dtype, shape in want:
        if not isinstance(t, torch.Tensor) or t.dtype != dtype or (shape is not None and tuple(t.shape) != shape) or not t.is_contiguous() \
                or t.device != dev:
            raise capi.IonodeError(f"multi_exp_objective: {what}: expected a contiguous {dtype} tensor {shape or ''} on {dev}")
    ptrs = [None if t is None else C.c_void_p(t.data_ptr()) for t in (active, seg_of_run, seg_off, t_rel, a, trial, value, status)]
    if dev.type == "cuda":
        rc = capi.lib().ionode_multi_exp_objective(n_run, n_active, lam, n_params, *ptrs, _stream(dev))
    else:
        rc = capi.lib().ionode_multi_exp_objective_host(n_run, n_active, lam, n_params, *ptrs)
    _check(rc, "ionode_multi_exp_objective")


def fit_runs(t_list, a_list, seg_of_run, starts, *, scale=None, seed=0, run_offset=0, popsize=None, sigma0=1.0 / 6.0, max_iter=1000,
             unchanged_iters=200, unchanged_threshold=1e-11, tolx=1e-11, compact_every=4, device=None):
    """K CMA-ES runs over S segments: run r minimises the RMSE of the multi-exponential against segment seg_of_run[r] (t_list[g] the
    times measured from the segment's first sample, a_list[g] its samples) from the initial mean starts[r] ([K, 7] tri-exponential or
    [K, 5] bi-exponential; all runs of a call share the kind).  scale [n_params]: the per-coordinate scale of the initial
    distribution (None: 1).  run_offset: the index of starts' first row among all runs of a fit -- with seed it fixes a run's random
    numbers, so a run computes the same bits alone (run_offset = its index) as among the others.  Returns numpy arrays
    (x [K, n_params], rmse [K], flag [K] int32 (capi.CMAES_*, FLAG_TEXT), iters [K, 2] int32 = (generations, evaluations)): the best
    point every run has evaluated."""
    starts = np.ascontiguousarray(np.asarray(starts, dtype=np.float64))
    if starts.ndim != 2 or starts.shape[1] not in (5, 7):
        raise capi.IonodeError("expfit: starts [K, 5] (bi-exponential) or [K, 7] (tri-exponential) expected")
    K, n = starts.shape
    seg = np.ascontiguousarray(np.asarray(seg_of_run, dtype=np.int32).reshape(-1))
    if len(t_list) != len(a_list) or any(np.size(t) != np.size(a) for t, a in zip(t_list, a_list)):
        raise capi.IonodeError("expfit: t_list and a_list must pair up, segment by segment")
    if seg.shape != (K,) or (K and (seg.min() < 0 or seg.max() >= len(t_list))):
        raise capi.IonodeError(f"expfit: seg_of_run [{K}] with entries in 0 .. {len(t_list) - 1} expected")
    if K == 0:
        return np.zeros((0, n)), np.zeros(0), np.zeros(0, dtype=np.int32), np.zeros((0, 2), dtype=np.int32)
    dev = _device(device)
    desc = cmaes.cmaes_desc(K, popsize, 1, n, list(range(n)), np.zeros(n), log_parameters=False, lo=None, hi=None, max_iter=max_iter,
                            unchanged_iters=unchanged_iters, unchanged_threshold=unchanged_threshold, tolx=tolx, seed=seed)
    desc.run_base = int(run_offset)
    lam = getattr(desc, "lambda")
    state, flag, iters, trial = (torch.from_numpy(x).to(dev) for x in cmaes.cmaes_init(starts, desc, sigma0, scale))
    off, tt = _ragged(t_list)
    _, aa = _ragged(a_list)
    seg_d, off_d, tt_d, aa_d = (torch.from_numpy(x).to(dev) for x in (seg, off, tt, aa))
    value = torch.zeros((K * lam,), dtype=torch.float64, device=dev)      # the first step reads nothing of these
    status = torch.zeros((K * lam,), dtype=torch.int32, device=dev)
    active, n_act = None, K
    every = int(compact_every or 0)
    for it in range(int(max_iter) + 1):
        rows = n_act * lam
        cmaes.cmaes_step(desc, active, value[:rows], status[:rows], state, flag, iters, trial)
        if every and it % every == 0 and it:   # the one read: who is still running
            left = steploop.compact(flag, active, n_act, trial, capi.CMAES_RUNNING)
            if left is None:
                break
            active, n_act, trial = left
            rows = n_act * lam
        if it == int(max_iter):
            break
        objective(K, lam, n, active, seg_d, off_d, tt_d, aa_d, trial, value[:rows], status[:rows])
    v = capi.cmaes_state_views(state, n, lam)
    return (v["best_x"].cpu().numpy().copy(), v["best_f"].cpu().numpy().copy(), flag.cpu().numpy(), iters.cpu().numpy())


def fit_segments(t_list, a_list, x0, *, restarts=4, seed=0, popsize=None, sigma0=1.0 / 6.0, max_iter=1000, unchanged_iters=200,
                 unchanged_threshold=1e-11, tolx=1e-11, compact_every=4, device=None):
    """Fit S segments of one kind in one call: x0 [7] (tri-exponential) or [5] (bi-exponential), t_list[g] the sample times measured
    from segment g's first fitted sample, a_list[g] its samples.  K = S (restarts + 1) runs, run g (restarts + 1) + i = restart i of
    segment g: restart 0 starts at x0, restart i > 0 at x0 exp(N(0, 0.5)) from numpy's default_rng(seed), drawn restart after restart
    as preprocess.fit_multi_exp draws them (every segment gets the same starts, as with one fit_multi_exp call per segment).  The
    search runs in the parameters themselves, no box (the reference's pints.fmin(f, x02, method=pints.CMAES)), with the
    per-coordinate scale |x0| (zeros: 1) and sigma0; the stopping rule and its defaults: the module's head.  popsize None:
    4 + floor(3 ln n_params) = 9 / 8.  device None: the current HIP device; "cpu": the host mirrors (tests; needs no GPU).
    Returns numpy arrays (x [S, n_params], rmse [S], flag [S, restarts + 1] int32, iters [S, restarts + 1, 2] int32): per segment the
    best restart by RMSE (ties: the lowest restart index), flag and iters of all its runs."""
    x0 = np.asarray(x0, dtype=np.float64).reshape(-1)
    if x0.size not in (5, 7):
        raise capi.IonodeError("expfit.fit_segments: x0 of 5 (bi-exponential) or 7 (tri-exponential) parameters expected")
    S, R = len(t_list), int(restarts) + 1
    rng = np.random.default_rng(seed)
    per_segment = np.stack([x0] + [x0 * np.exp(rng.normal(0.0, 0.5, x0.size)) for _ in range(R - 1)])
    scale = np.where(x0 == 0.0, 1.0, np.abs(x0))
    x, f, flag, iters = fit_runs(t_list, a_list, np.repeat(np.arange(S, dtype=np.int32), R), np.tile(per_segment, (S, 1)), scale=scale, seed=seed,
                                 popsize=popsize, sigma0=sigma0, max_iter=max_iter, unchanged_iters=unchanged_iters,
                                 unchanged_threshold=unchanged_threshold, tolx=tolx, compact_every=compact_every, device=device)
    f = f.reshape(S, R)
    best = np.argmin(f, axis=1)   # (the first of equal values; the step has turned every NaN into +inf)
    pick = np.arange(S)
    return x.reshape(S, R, -1)[pick, best], f[pick, best], flag.reshape(S, R), iters.reshape(S, R, 2)


def evaluate(x, t_full_list, device=None):
    """The fitted curves on the segments' full grids through ionode_multi_exp_eval: x [S, 7 | 5], t_full_list[g] segment g's times
    measured from its first FITTED sample.  Returns three lists of numpy arrays (a_fit, dadt, d2adt2), one array per segment."""
    x = np.ascontiguousarray(np.asarray(x, dtype=np.float64))
    if x.ndim != 2 or x.shape[1] not in (5, 7) or x.shape[0] != len(t_full_list):
        raise capi.IonodeError("expfit.evaluate: x [S, 5 | 7] with one row per entry of t_full_list expected")
    S, n = x.shape
    off, tt = _ragged(t_full_list)
    if S == 0:
        return [], [], []
    dev = _device(device)
    x_d, off_d, tt_d = (torch.from_numpy(v).to(dev) for v in (x, off, tt))
    out = [torch.zeros_like(tt_d) for _ in range(3)]
    ptrs = [C.c_void_p(t.data_ptr()) for t in (x_d, off_d, tt_d, *out)]
    if dev.type == "cuda":
        rc = capi.lib().ionode_multi_exp_eval(S, n, *ptrs, _stream(dev))
    else:
        rc = capi.lib().ionode_multi_exp_eval_host(S, n, *ptrs)
    _check(rc, "ionode_multi_exp_eval")
    return tuple([o.cpu().numpy()[off[g]:off[g + 1]].copy() for g in range(S)] for o in out)
