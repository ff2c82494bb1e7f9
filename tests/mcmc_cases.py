"""Shared inputs of the adaptive-Metropolis tests (test_mcmc_host.py, test_mcmc_driver_host.py, test_gpu_mcmc.py) and a plain numpy
statement of the algorithm of include/ionode.h "Adaptive Metropolis step": the generator of tests/cmaes_cases.py (Philox4x32-10, the
step's logarithm, AS241 PPND16 -- the library's bit for bit), the same formulas (Andrieu and Thoms 2008, Algorithm 4), and
numpy.linalg.cholesky, numpy.exp and numpy.log where the library runs its own.  It is the checker: no sampling package is assumed."""
import importlib
import math
from types import SimpleNamespace

import numpy as np
import torch

import cmaes_cases as L

EPS = L.EPS
CALLS = 6            # consecutive calls of a drawn case: the start's evaluation and five tells
ADAPT_START = 3      # ... which cross the start of the adaptation
DIMS = [(n, ss) for n in (1, 4, 12, 13) for ss in (0, 1) if 1 <= n - ss <= 12]   # (coordinates, sigma sampled): nf = n - ss is 1 .. 12
same_bits = L.same_bits


def mods():
    ion = importlib.import_module("neural-ode-ion-channels_amd")
    return ion.capi, importlib.import_module("neural-ode-ion-channels_amd.mcmc")


# ---- the algorithm ----

def acceptance_uniform(seed, chain, t):
    w = L.draw_words(seed, chain, t, 1, 0, 0)
    return L.uniform(w[0], w[1])


def log_posterior(S, ls, N):
    return -N * ls - 0.5 * S * math.exp(-2.0 * ls) if S < math.inf else -math.inf


def box(case):
    """(ulo, uhi, xlo, xhi) [n] of a case: the free parameters' box, then sigma's when it is sampled."""
    nf, ss = case["nf"], case["ss"]
    xlo, xhi = np.array(case["lo"], dtype=float), np.array(case["hi"], dtype=float)
    ulo, uhi = (np.log(xlo), np.log(xhi)) if case["log"] else (xlo.copy(), xhi.copy())
    if ss:
        xlo, xhi = np.append(xlo, case["sigma_bounds"][0]), np.append(xhi, case["sigma_bounds"][1])
        ulo, uhi = np.append(ulo, math.log(case["sigma_bounds"][0])), np.append(uhi, math.log(case["sigma_bounds"][1]))
    assert len(ulo) == nf + ss
    return ulo, uhi, xlo, xhi


def to_x(case, u):
    """The parameters of a point of the search space, clamped into the box as the library clamps them."""
    _, _, xlo, xhi = box(case)
    x = np.array(u, dtype=float)
    if case["log"]:
        x[:case["nf"]] = np.exp(x[:case["nf"]])
    if case["ss"]:
        x[case["nf"]] = math.exp(x[case["nf"]])
    return np.minimum(np.maximum(x, xlo), xhi)


def values(case, ev):
    """S [K] from an evaluation's arrays, as the header states it: protocols in order, a status or a NaN makes +inf."""
    K, P = case["K"], case["P"]
    v, s = ev["value"].reshape(K, P), ev["status"].reshape(K, P)
    S = np.zeros(K)
    for p in range(P):
        S = S + v[:, p]
    return np.where((s != 0).any(axis=1) | ~(S < np.inf), np.inf, S)


def step(case, st, chain, t, S, d=None):
    """One call for one running chain in numpy: st = dict(u, ut, x, xt, mu, C, lp, log_lambda, outside) before, S the evaluation's sum.
    Returns (the dict after, info): info has alpha, accept, margin (|log w - (lp_t - lp)|, None at t = 0), flag."""
    capi, _ = mods()
    d = case["desc"] if d is None else d
    n, nf, ss = case["n"], case["nf"], case["ss"]
    ulo, uhi, _, _ = box(case)
    new = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in st.items()}
    info = dict(alpha=None, accept=False, margin=None, flag=capi.MCMC_RUNNING)
    point = st["u"] if t == 0 else st["ut"]
    ls = point[nf] if ss else math.log(d.sigma)
    lp_t = log_posterior(S, ls, d.n_samples)
    if t == 0:
        new["lp"] = lp_t
        if not (((st["u"] >= ulo) & (st["u"] <= uhi)).all() and np.isfinite(lp_t)):
            info["flag"] = capi.MCMC_NONFINITE
    else:
        diff = lp_t - st["lp"]
        alpha = 0.0 if (st["outside"] or not np.isfinite(lp_t)) else math.exp(min(diff, 0.0))
        logw = math.log(acceptance_uniform(d.seed, d.chain_base + chain, t))
        accept = alpha > 0.0 and logw < diff
        info.update(alpha=alpha, accept=accept, margin=abs(logw - diff) if alpha > 0.0 else math.inf, lp_t=lp_t)
        if accept:
            new["u"], new["x"], new["lp"] = st["ut"].copy(), st["xt"].copy(), lp_t
        if t >= d.adapt_start:
            gamma = math.exp(-d.eta * math.log(t - d.adapt_start + 2))
            new["mu"] = st["mu"] + gamma * (new["u"] - st["mu"])
            dd = new["u"] - new["mu"]
            new["C"] = st["C"] + gamma * (np.outer(dd, dd) - st["C"])
            new["log_lambda"] = st["log_lambda"] + gamma * (alpha - d.target_accept)
    if info["flag"] == capi.MCMC_RUNNING:
        A = math.exp(new["log_lambda"]) * (new["C"] + d.epsilon * np.eye(n))
        try:
            if not (np.isfinite(A).all() and np.isfinite(new["log_lambda"])):
                raise np.linalg.LinAlgError
            Lf = np.linalg.cholesky(A)
        except np.linalg.LinAlgError:
            info["flag"] = capi.MCMC_DEGENERATE
        else:
            new["L"] = Lf
            if t >= d.max_iter:
                info["flag"] = capi.MCMC_MAXITER
    if info["flag"] == capi.MCMC_RUNNING:
        z = L.normals(d.seed, d.chain_base + chain, t + 1, 0, n, 0)
        ut = new["u"] + new["L"] @ z
        inside = bool(((ut >= ulo) & (ut <= uhi)).all())
        new["ut"], new["outside"], info["z"] = ut, not inside, z
        new["xt"] = to_x(case, ut) if inside else new["x"].copy()
    return new, info


def state_dict(views, c):
    return dict(u=views["u"][c].copy(), ut=views["ut"][c].copy(), x=views["x"][c].copy(), xt=views["xt"][c].copy(), mu=views["mu"][c].copy(),
                C=views["C"][c].copy(), L=views["L"][c].copy(), lp=float(views["lp"][c]), log_lambda=float(views["log_lambda"][c]),
                outside=bool(views["outside"][c] != 0.0))


def reference_chain(fn, x0, *, case, chain, iters, scale):
    """The whole algorithm on one chain in numpy: fn(x) is the sum of squares of the parameters x [nf].  Returns the recorded rows
    [iters + 1, n + 1] and the accepted count."""
    n, nf = case["n"], case["nf"]
    u0 = np.array(x0, dtype=float)
    if case["log"]:
        u0[:nf] = np.log(u0[:nf])
    if case["ss"]:
        u0[nf] = math.log(u0[nf])
    st = dict(u=u0.copy(), ut=u0.copy(), x=np.array(x0, dtype=float), xt=np.array(x0, dtype=float), mu=u0.copy(),
              C=np.diag((np.ones(n) * scale) ** 2), lp=0.0, log_lambda=0.0, outside=False)
    rows, accepted = [], 0
    for t in range(iters + 1):
        S = fn((st["x"] if t == 0 else st["xt"])[:nf])
        st, info = step(case, st, chain, t, S)
        accepted += int(info["accept"])
        rows.append(np.append(st["x"], st["lp"]))
        if info["flag"] != 0:
            break
    return np.array(rows), accepted


# ---- seeded cases for the step itself ----

def draw(seed, K, n, P, *, log, ss, scale=0.1, **desc_kw):
    """One drawn case: starts x0 [K, n], a descriptor, and the value / status arrays of CALLS consecutive calls (the first is the
    start's evaluation).  Values are seeded and carry a failed status and a NaN."""
    capi, mc = mods()
    rng = np.random.default_rng(seed)
    nf = n - ss
    npar = 12 if nf > 8 else (8 if seed % 2 == 0 else 12)
    free = L.free_columns(nf, npar)
    base = rng.uniform(0.5, 2.0, npar)
    x0 = rng.uniform(0.5, 2.0, (K, n))
    if ss:
        x0[:, nf] = rng.uniform(0.8, 1.25, K)
    lo, hi = np.full(nf, 0.1), np.full(nf, 10.0)
    sigma_bounds = (0.05, 20.0) if ss else None
    kw = dict(max_iter=50, adapt_start=ADAPT_START, thin=1, seed=1234 + seed, epsilon=1e-12, n_samples=10.0 * P)
    kw.update(desc_kw)
    desc = mc.mcmc_desc(K, P, npar, free, base, log_parameters=log, lo=lo, hi=hi, sigma=None if ss else 1.0, sigma_bounds=sigma_bounds, **kw)
    evals = []
    for g in range(CALLS):
        value = rng.uniform(1.0, 5.0, K * P) / P
        status = np.zeros(K * P, dtype=np.int32)
        if g == 2:
            status.reshape(K, P)[K // 2, P - 1] = 3      # a failure whose value is finite: the status alone decides
        if g == 4:
            value.reshape(K, P)[0, 0] = np.nan           # ... and a NaN counts as one
        evals.append(dict(value=value, status=status))
    return dict(K=K, n=n, nf=nf, ss=ss, P=P, npar=npar, free=free, base=base, x0=x0, log=log, lo=lo, hi=hi, sigma_bounds=sigma_bounds,
                desc=desc, evals=evals, seed=kw["seed"], scale=scale)


def start(case, scale=None):
    _, mc = mods()
    return [torch.from_numpy(a) for a in mc.mcmc_init(case["x0"], case["desc"], case["scale"] if scale is None else scale)]


def with_desc(case, **fields):
    d = mods()[0].IonodeMcmcDesc.from_buffer_copy(case["desc"])
    for k, val in fields.items():
        setattr(d, k, val)
    return dict(case, desc=d)


def run_sequence(case, device=None, active=None, evals=None, scale=None, samples=True):
    """The case's consecutive calls through mcmc.mcmc_step on `device` (None or "cpu": the host mirror; a HIP device: the kernel).
    Returns after every call numpy copies of (state, flag, iters, trial, samples)."""
    capi, mc = mods()
    device = "cpu" if device is None else device
    desc = capi.IonodeMcmcDesc.from_buffer_copy(case["desc"])
    state, flag, iters, trial, smp = (t.to(device) for t in start(case, scale))
    if not samples:
        smp = None
    P = case["P"]
    act, rows = None, None
    if active is not None:
        act = torch.tensor(list(active), dtype=torch.int32, device=device)
        rows = L.slot_rows(active, P)
        trial = trial[torch.from_numpy(rows).to(device)].contiguous()
    evals = case["evals"] if evals is None else evals
    out = []
    for ev in evals:
        pick = (lambda a: a) if rows is None else (lambda a: a[rows])
        value = torch.from_numpy(np.ascontiguousarray(pick(ev["value"]))).to(device)
        status = torch.from_numpy(np.ascontiguousarray(pick(ev["status"]))).to(device)
        assert value.shape[0] == trial.shape[0]
        mc.mcmc_step(desc, act, value, status, state, flag, iters, trial, smp)
        out.append(tuple(None if x is None else x.cpu().numpy().copy() for x in (state, flag, iters, trial, smp)))
    return out


def path_cases():
    """The sequences of test_mcmc_host.py's path tests, by name: (case, keyword arguments of run_sequence).  test_gpu_mcmc.py runs the
    same on the device and compares with the mirror."""
    case = draw(11, 5, 5, 3, log=True, ss=1)
    out = {"plain": (case, {}), "max_iter_2": (with_desc(case, max_iter=2), {}), "no_samples": (case, dict(samples=False)),
           "thin_2_cap_2": (with_desc(case, thin=2, sample_cap=2), {})}
    ev = [dict(value=e["value"].copy(), status=e["status"].copy()) for e in case["evals"]]
    ev[0]["status"].reshape(5, 3)[2, 1] = 2           # chain 2: its start cannot be evaluated
    ev[0]["value"].reshape(5, 3)[3, 0] = np.inf       # chain 3: an infinite sum
    out["bad_start"] = (case, dict(evals=ev))
    outside = dict(case, x0=case["x0"].copy())
    outside["x0"][4, 0] = 0.05                        # chain 4 starts outside the box
    out["start_outside"] = (outside, {})
    out["degenerate"] = (with_desc(case, epsilon=0.0), dict(scale=0.0))
    corner = draw(13, 5, 4, 1, log=False, ss=0, scale=3.0)
    corner["x0"][:] = corner["hi"]                    # on the box's corner with a proposal of a third of its width: most leave it
    for e in corner["evals"][1:]:
        e["value"][:] = 0.0                           # ... and whatever is evaluated for them looks perfect
    out["corner"] = (corner, {})
    failed = draw(17, 5, 4, 3, log=True, ss=0)
    for e in failed["evals"][1:]:
        e["value"][:] = 0.0
        e["status"].reshape(5, 3)[:, 1] = 1           # every proposal fails, with a value that would be accepted
    out["failed_status"] = (failed, {})
    return out


# ---- analytic targets for the stand-in solver of the distribution tests ----

GAUSS_SD = np.array([0.05, 0.2, 1.0])
GAUSS_RHO = 0.45
GAUSS_CORR = np.array([[1.0, GAUSS_RHO, 0.0], [GAUSS_RHO, 1.0, GAUSS_RHO], [0.0, GAUSS_RHO, 1.0]])
GAUSS_COV = GAUSS_SD[:, None] * GAUSS_CORR * GAUSS_SD[None, :]
GAUSS_PREC = np.linalg.inv(GAUSS_COV)


def gauss_problem(log):
    """Target (a): three coordinates, fixed sigma = 1, S = d^T Sigma^-1 d, so the posterior of the SEARCH variables is N(centre, Sigma)
    (standard deviations 0.05 / 0.2 / 1.0, correlation 0.45 between neighbours); starts 3 sd away, the box +- 12 sd.  With log
    parameters the search variable is log x and d = log x - centre.  Returns dict(fn, x0 [64, 3], bounds, centre) in the parameters."""
    centre = np.array([1.0, 2.0, 3.0]) if not log else np.zeros(3)
    def fn(x):
        d = (np.log(x) if log else x) - centre
        return float(d @ GAUSS_PREC @ d)
    u0 = np.tile(centre + 3.0 * GAUSS_SD, (64, 1))
    ulo, uhi = centre - 12.0 * GAUSS_SD, centre + 12.0 * GAUSS_SD
    f = np.exp if log else (lambda a: a)
    return dict(fn=fn, x0=f(u0), bounds=(f(ulo), f(uhi)), centre=centre)


SIG_N, SIG_S0, SIG_KAPPA, SIG_XSTAR = 50, 12.5, 400.0, 2.0


def sigma_problem():
    """Target (b): one free parameter plus sampled sigma, S = S0 + kappa (x - x*)^2 with N = 50 residuals (5 protocols x 10 samples).
    With the log-uniform prior on sigma the marginals are exact: E[x] = x*, and sigma^2 given x is inverse-gamma, so E[sigma^2] =
    E[S / (N - 2)] = S0 / (N - 3) after integrating x (a Student-t with N - 1 degrees of freedom around x*)."""
    def fn(x):
        return SIG_S0 + SIG_KAPPA * float((x[0] - SIG_XSTAR) ** 2)
    x0 = np.tile(np.array([SIG_XSTAR + 0.1, 0.8]), (64, 1))
    return dict(fn=fn, x0=x0, bounds=(np.array([SIG_XSTAR - 1.0]), np.array([SIG_XSTAR + 1.0])), sigma_bounds=(0.05, 20.0),
                mean_x=SIG_XSTAR, mean_sigma2=SIG_S0 / (SIG_N - 3))


def analytic_solver(fn, free, P, calls=None, seen=None):
    """cmaes_cases.analytic_solver for the sampler: protocol p of a chain contributes fn(x) / P; calls receives the row count of every
    evaluation, seen the (model, keyword arguments) of every call."""
    def solver(model, params, prot_v, y0, t_eval, **kw):
        p = params.numpy()
        if calls is not None:
            calls.append(p.shape[0])
        if seen is not None:
            seen.append((model, {k: v for k, v in kw.items() if k in ("weights", "mlp_layers", "mlp_width", "weights_key", "objective", "max_step")}))
        assert kw["states"] is False and kw["sse_ref"] is not None and kw["objective"] == "sse"
        assert y0.shape[0] == p.shape[0] and kw["prot_of_traj"].shape[0] == p.shape[0]
        val, status = np.zeros(p.shape[0]), np.zeros(p.shape[0], dtype=np.int32)
        for b in range(p.shape[0]):
            if not np.isfinite(p[b]).all():
                val[b], status[b] = np.inf, 2
            else:
                val[b] = fn(p[b, list(free)]) / P
        return SimpleNamespace(sse=torch.from_numpy(val), sae=None, status=torch.from_numpy(status))
    return solver


# ---- the HH 2-state run of test_mcmc_driver_host.py (CPU oracle as the solver) and test_gpu_mcmc.py (the GPU solve) ----

HH_NOISE_SIGMA, HH_NOISE_SEED, HH_SEED = 0.1, 19, 3
HH_SIGMA_BOUNDS = (0.01, 1.0)


def fused_sum(term, t1, t_eval):
    """The fused objective's sum of one trajectory in the library's order (csrc/ionode_attempt_body.hpp, the lane-wise kernels): term
    [Nt] the residuals' terms, t1 the end times of the accepted steps.  Sample 0 starts the sum; an accepted step emits the samples it
    covers (t_k <= t1), sample s of the step going to lane s % 64 (a lane adds its samples in order); every group of 8 lanes is summed
    as ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7)) and added to the group's partial sum; the 8 partial sums are added at the end."""
    part, total, oi, Nt = [0.0] * 8, float(term[0]), 1, len(t_eval)
    for end in t1:
        n = 0
        while oi + n < Nt and t_eval[oi + n] <= end:
            n += 1
        lanes = [0.0] * 64
        for k in range(n):
            lanes[k % 64] = lanes[k % 64] + float(term[oi + k])
        for g in range((min(n, 64) + 7) // 8):
            r = lanes[8 * g:8 * g + 8]
            part[g] = part[g] + (((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7])))
        oi += n
    for m in range(8):
        total = total + part[m]
    return total


def oracle_solver(oracle, calls=None):
    """cmaes_cases.oracle_solver with the sum of squares formed in the library's order (fused_sum, from the oracle's own step log, one
    trajectory at a time): the stand-in then returns the GPU solve's values bit for bit, not only to rounding."""
    def solver(model, params, prot_v, y0, t_eval, **kw):
        p, te, pv = params.numpy(), t_eval.numpy(), prot_v.numpy()
        pot = kw["prot_of_traj"].numpy()
        assert kw.get("objective", "sse") == "sse"
        if calls is not None:
            calls.append(p.shape[0])
        ref = kw["sse_ref"].numpy()
        val, status = np.full(p.shape[0], np.inf), np.zeros(p.shape[0], dtype=np.int32)
        volt = [oracle.protocol_v(pv[k], te, prot_t0=kw["prot_t0"], prot_dt=kw["prot_dt"])[0] for k in range(pv.shape[0])]
        for b in range(p.shape[0]):
            r = oracle.solve(model, p[b:b + 1], pv, [0.0, 1.0], te, prot_t0=kw["prot_t0"], prot_dt=kw["prot_dt"], prot_of_traj=pot[b:b + 1], state_f32=False,
                             rtol=kw["rtol"], atol=kw["atol"], max_step=kw["max_step"], step_log_cap=1 << 16)
            status[b] = r["status"][0]
            if status[b] == 0:
                log = r["step_log"]
                assert len(log) < (1 << 16)
                acc = log[log[:, 3] != 0]
                res = oracle.current(r["y"][0], volt[pot[b]], state_f32=False) - ref[pot[b]]
                val[b] = fused_sum(res * res, acc[:, 0] + acc[:, 1], te)
        return SimpleNamespace(sse=torch.from_numpy(val), sae=None, status=torch.from_numpy(status))
    return solver


def hh_noisy(data):
    """The reference's noise (noise_sigma = 0.1) from a fixed seed on clean currents [2, 2001]."""
    return data + HH_NOISE_SIGMA * np.random.default_rng(HH_NOISE_SEED).normal(size=data.shape)


def hh_starts(pb, K):
    """K <= 64 starts: cmaes_cases.hh_problem()'s four, repeated with a 1 % spread, and sigma = 0.1.  Start k does not depend on K."""
    spread = np.exp(0.01 * np.random.default_rng(23).normal(size=(64, 4)))
    x = np.stack([pb["starts"][k % 4] * spread[k] for k in range(K)])
    return np.concatenate([x, np.full((K, 1), HH_NOISE_SIGMA)], axis=1)


def hh_sample(pb, data, solver, device, K, iters, **kw):
    """p1 .. p4 in log parameters plus sigma, scale 0.02, two protocols."""
    _, mc = mods()
    return mc.sample(0, hh_starts(pb, K), pb["pv"], data, pb["te"], base_params=pb["true"], free=L.HH_FREE, bounds=(pb["lo"], pb["hi"]),
                     sigma_bounds=HH_SIGMA_BOUNDS, scale=0.02, prot_dt=pb["prot_dt"], state_dtype=torch.float64, rtol=L.HH_RTOL, atol=L.HH_ATOL,
                     max_step=0.0, seed=HH_SEED, max_iter=iters, adapt_start=20, solver=solver, device=device, **kw)
