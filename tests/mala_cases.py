"""Shared inputs of the manifold-MALA tests (test_mala_host.py, test_mala_driver_host.py, test_gpu_mala.py) and a plain numpy statement
of the algorithm of include/ionode.h "Manifold MALA step": the generator of tests/cmaes_cases.py (Philox4x32-10, the step's logarithm,
AS241 PPND16 -- the library's bit for bit), the same formulas (Girolami and Calderhead 2011, the simplified manifold MALA), and
numpy.linalg.cholesky, numpy.linalg.solve, numpy.exp and numpy.log where the library runs its own.  It is the checker: no sampling
package is assumed."""
import importlib
import math

import numpy as np
import torch

import cmaes_cases as L

EPS = L.EPS
CALLS = 6            # consecutive calls of a drawn case: the start's evaluation and five tells
DIMS = [(1, 0), (2, 1), (4, 0), (5, 1), (8, 0), (12, 0), (13, 1)]   # (coordinates, sigma sampled): the issue's set
same_bits = L.same_bits
FLOOR_REL, FLOOR_ABS = 2.0 ** -20, 2.0 ** -256


def mods():
    ion = importlib.import_module("neural-ode-ion-channels_amd")
    return ion.capi, importlib.import_module("neural-ode-ion-channels_amd.mala")


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


def reduce(case, ev):
    """(S [K], g_x [K, nf], H_x [K, nf, nf]) from an evaluation's arrays, as the header states it: protocols in order, a status or a
    NaN makes S +inf, the free rows and columns of jtr and jtj."""
    K, P, npar, free = case["K"], case["P"], case["npar"], list(case["free"])
    v, s = ev["sse"].reshape(K, P), ev["status"].reshape(K, P)
    jtr, jtj = ev["jtr"].reshape(K, P, npar), ev["jtj"].reshape(K, P, npar, npar)
    S, g, H = np.zeros(K), np.zeros((K, len(free))), np.zeros((K, len(free), len(free)))
    for p in range(P):
        S = S + v[:, p]
        g = g + jtr[:, p][:, free]
        H = H + jtj[:, p][:, free][:, :, free]
    return np.where((s != 0).any(axis=1) | ~(S < np.inf), np.inf, S), g, H


def metric(case, d, S, gx, Hx, u, x):
    """(lp, grad [n], G [n, n] with its ridge) at the evaluated point (u, x) from the protocol sums."""
    n, nf, ss = case["n"], case["nf"], case["ss"]
    ls = u[nf] if ss else math.log(d.sigma)
    lp = log_posterior(S, ls, d.n_samples)
    inv_s2 = math.exp(-2.0 * ls)
    scale = x[:nf] if case["log"] else np.ones(nf)
    with np.errstate(all="ignore"):
        grad, G = np.zeros(n), np.zeros((n, n))
        grad[:nf] = -(gx * scale) * inv_s2
        Hl = np.tril(Hx)
        Hs = Hl + np.tril(Hx, -1).T                      # only the lower triangle is read
        G[:nf, :nf] = Hs * np.outer(scale, scale) * inv_s2
        if ss:
            grad[nf] = -d.n_samples + S * inv_s2
            G[nf, nf] = 2.0 * d.n_samples
        dg = np.diag(G).copy()
        dmax = max([0.0] + [v for v in dg if v > 0.0])
        floor = max(FLOOR_REL * dmax, FLOOR_ABS)
        G[np.diag_indices(n)] = dg + d.ridge * np.where(dg > floor, dg, floor)
    return lp, grad, G


def factor(grad, G):
    """(L, ld) or None when the metric does not factor."""
    if not (np.isfinite(G).all() and np.isfinite(grad).all()):
        return None
    try:
        Lf = np.linalg.cholesky(G)
    except np.linalg.LinAlgError:
        return None
    ld = float(np.log(np.diag(Lf)).sum())
    return (Lf, ld) if np.isfinite(ld) else None


def step(case, st, chain, t, S, gx, Hx, d=None):
    """One call for one running chain in numpy: st = dict(u, ut, x, xt, grad, L, lp, log_eps, ld, lqf, outside) before; S, gx, Hx the
    evaluation's protocol sums.  Returns (the dict after, info): info has alpha, accept, ratio, margin (|log w - ratio|, None at
    t = 0), flag, ok (the evaluated metric factored), and the quantities the rounding bounds are stated from."""
    capi, _ = mods()
    d = case["desc"] if d is None else d
    n = case["n"]
    ulo, uhi, _, _ = box(case)
    new = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in st.items()}
    info = dict(alpha=None, accept=False, margin=None, ratio=None, flag=capi.MALA_RUNNING)
    ue, xe = (st["u"], st["x"]) if t == 0 else (st["ut"], st["xt"])
    lp_t, grad_t, G_t = metric(case, d, S, gx, Hx, ue, xe)
    fac = factor(grad_t, G_t)
    info.update(ok=fac is not None, lp_t=lp_t, G_t=G_t, grad_t=grad_t)
    take = False
    if t == 0:
        new["lp"] = lp_t
        if not (((st["u"] >= ulo) & (st["u"] <= uhi)).all() and np.isfinite(lp_t)):
            info["flag"] = capi.MALA_NONFINITE
        elif fac is None:
            info["flag"] = capi.MALA_DEGENERATE
        else:
            take = True
    else:
        alpha, ratio, margin = 0.0, -math.inf, math.inf
        logw = math.log(acceptance_uniform(d.seed, d.chain_base + chain, t))
        if not st["outside"] and np.isfinite(lp_t) and fac is not None:
            Lt, ld_t = fac
            eps = math.exp(st["log_eps"])
            dvec = np.linalg.solve(G_t, grad_t)
            mu_t = st["ut"] + 0.5 * eps * eps * dvec
            v = Lt.T @ (st["u"] - mu_t)
            q = float(v @ v)
            lqr = ld_t - n * st["log_eps"] - q / (2.0 * eps * eps)
            ratio = lp_t + lqr - st["lp"] - st["lqf"]
            if not math.isnan(ratio):
                alpha = math.exp(min(ratio, 0.0))
            margin = abs(logw - ratio) if alpha > 0.0 else math.inf
            info.update(v=v, dvec=dvec, eps=eps, ld_t=ld_t, Lt=Lt, q=q)
        take = alpha > 0.0 and logw < ratio
        info.update(alpha=alpha, accept=take, ratio=ratio, margin=margin)
        if take:
            new["u"], new["x"], new["lp"] = st["ut"].copy(), st["xt"].copy(), lp_t
        new["log_eps"] = st["log_eps"] + math.exp(-d.eta * math.log(t + 1)) * (alpha - d.target_accept)
        if t >= d.max_iter:
            info["flag"] = capi.MALA_MAXITER
    if take:
        new["grad"], new["L"], new["ld"] = grad_t, fac[0], fac[1]
    if info["flag"] == capi.MALA_RUNNING:
        z = L.normals(d.seed, d.chain_base + chain, t + 1, 0, n, 0)
        eps = math.exp(new["log_eps"])
        Lc = new["L"]
        y = np.linalg.solve(Lc, new["grad"])
        ut = new["u"] + np.linalg.solve(Lc.T, 0.5 * eps * eps * y + eps * z)
        with np.errstate(all="ignore"):
            inside = bool(((ut >= ulo) & (ut <= uhi)).all())
        new["ut"], new["outside"], info["z"] = ut, not inside, z
        new["xt"] = to_x(case, ut) if inside else new["x"].copy()
        new["lqf"] = new["ld"] - n * new["log_eps"] - 0.5 * float(z @ z)
    return new, info


def state_dict(views, c):
    return dict(u=views["u"][c].copy(), ut=views["ut"][c].copy(), x=views["x"][c].copy(), xt=views["xt"][c].copy(),
                grad=views["grad"][c].copy(), L=views["L"][c].copy(), lp=float(views["lp"][c]), log_eps=float(views["log_eps"][c]),
                ld=float(views["ld"][c]), lqf=float(views["lqf"][c]), outside=bool(views["outside"][c] != 0.0))


def reference_chains(gn, x0, *, case, iters, eps0=1.0, chains=None):
    """The whole algorithm in numpy, chain after chain: gn(x [nf]) -> (S, g_x [nf], H_x [nf, nf]) at the parameters x.  Returns the
    recorded rows [K, iters + 1, n + 1] (NaN after a stop) and the accepted counts [K]."""
    n, nf = case["n"], case["nf"]
    x0 = np.asarray(x0, dtype=float)
    chains = range(x0.shape[0]) if chains is None else chains
    rows, accepted = np.full((len(chains), iters + 1, n + 1), np.nan), np.zeros(len(chains), dtype=int)
    for k, c in enumerate(chains):
        u0 = x0[c].copy()
        if case["log"]:
            u0[:nf] = np.log(u0[:nf])
        if case["ss"]:
            u0[nf] = math.log(u0[nf])
        st = dict(u=u0.copy(), ut=u0.copy(), x=x0[c].copy(), xt=x0[c].copy(), grad=np.zeros(n), L=np.zeros((n, n)), lp=0.0,
                  log_eps=math.log(eps0), ld=0.0, lqf=0.0, outside=False)
        for t in range(iters + 1):
            S, g, H = gn((st["x"] if t == 0 else st["xt"])[:nf])
            st, info = step(case, st, c, t, S, g, H)
            accepted[k] += int(info["accept"])
            rows[k, t] = np.append(st["x"], st["lp"])
            if info["flag"] != 0:
                break
    return rows, accepted


def plain_case(n, nf, ss, log, bounds, *, seed, sigma=None, sigma_bounds=None, n_samples, max_iter, **kw):
    """A case dict for reference_chains / step around a descriptor, without drawn evaluations."""
    _, ma = mods()
    desc = ma.mala_desc(1, 1, 8, list(range(nf)), np.zeros(8), log_parameters=log, lo=bounds[0], hi=bounds[1], sigma=sigma,
                        sigma_bounds=sigma_bounds, n_samples=n_samples, max_iter=max_iter, seed=seed, **kw)
    return dict(n=n, nf=nf, ss=ss, log=log, lo=bounds[0], hi=bounds[1], sigma_bounds=sigma_bounds, desc=desc)


# ---- seeded cases for the step itself ----

def draw(seed, K, n, P, *, log, ss, **desc_kw):
    """One drawn case: starts x0 [K, n], a descriptor, and the sse / jtr / jtj / status arrays of CALLS consecutive calls (the first
    is the start's evaluation).  Every trajectory's arrays come from a seeded Jacobian J [npar + 3, npar] and residual r: jtj = J^T J
    is positive definite and differs by a few per cent from call to call, as a metric does from point to point.  The arrays carry a
    failed status and a NaN."""
    capi, ma = mods()
    rng = np.random.default_rng(seed)
    nf = n - ss
    npar = 12 if nf > 8 else (8 if seed % 2 == 0 else 12)
    free = L.free_columns(nf, npar)
    base = rng.uniform(0.5, 2.0, npar)
    x0 = rng.uniform(0.8, 1.25, (K, n))
    lo, hi = np.full(nf, 0.1), np.full(nf, 10.0)
    sigma_bounds = (0.05, 20.0) if ss else None
    kw = dict(max_iter=50, thin=1, seed=1234 + seed, n_samples=10.0 * P)
    kw.update(desc_kw)
    desc = ma.mala_desc(K, P, npar, free, base, log_parameters=log, lo=lo, hi=hi, sigma=None if ss else 1.0, sigma_bounds=sigma_bounds, **kw)
    m = npar + 3
    J0 = rng.normal(size=(K * P, m, npar)) * 2.0
    evals = []
    for g in range(CALLS):
        J = J0 + 0.05 * rng.normal(size=J0.shape)
        r = rng.normal(size=(K * P, m)) * math.sqrt(0.7 / m)
        sse = np.einsum("bm,bm->b", r, r) * rng.uniform(0.5, 1.5, K * P)
        jtr = np.einsum("bmi,bm->bi", J, r)
        jtj = np.einsum("bmi,bmj->bij", J, J)
        jtj = 0.5 * (jtj + jtj.transpose(0, 2, 1))
        status = np.zeros(K * P, dtype=np.int32)
        if g == 2:
            status.reshape(K, P)[K // 2, P - 1] = 3      # a failure whose values are finite: the status alone decides
        if g == 4:
            sse.reshape(K, P)[0, 0] = np.nan             # ... and a NaN counts as one
        evals.append(dict(sse=sse, jtr=np.ascontiguousarray(jtr), jtj=np.ascontiguousarray(jtj), status=status))
    return dict(K=K, n=n, nf=nf, ss=ss, P=P, npar=npar, free=free, base=base, x0=x0, log=log, lo=lo, hi=hi, sigma_bounds=sigma_bounds,
                desc=desc, evals=evals, seed=kw["seed"])


def case_seed(n, ss, P, log, K):
    return 1000 * n + 100 * ss + 10 * P + K + int(log)


def start(case, eps0=1.0):
    _, ma = mods()
    return [torch.from_numpy(a) for a in ma.mala_init(case["x0"], case["desc"], eps0)]


def with_desc(case, **fields):
    d = mods()[0].IonodeMalaDesc.from_buffer_copy(case["desc"])
    for k, val in fields.items():
        setattr(d, k, val)
    return dict(case, desc=d)


def copy_evals(case):
    return [{k: v.copy() for k, v in e.items()} for e in case["evals"]]


def run_sequence(case, device=None, active=None, evals=None, eps0=1.0, samples=True):
    """The case's consecutive calls through mala.mala_step on `device` (None or "cpu": the host mirror; a HIP device: the kernel).
    Returns after every call numpy copies of (state, flag, iters, trial, samples)."""
    capi, ma = mods()
    device = "cpu" if device is None else device
    desc = capi.IonodeMalaDesc.from_buffer_copy(case["desc"])
    state, flag, iters, trial, smp = (t.to(device) for t in start(case, eps0))
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
        arrs = [torch.from_numpy(np.ascontiguousarray(pick(ev[k]))).to(device) for k in ("sse", "jtr", "jtj", "status")]
        assert arrs[0].shape[0] == trial.shape[0]
        ma.mala_step(desc, act, *arrs, state, flag, iters, trial, smp)
        out.append(tuple(None if x is None else x.cpu().numpy().copy() for x in (state, flag, iters, trial, smp)))
    return out


def path_cases():
    """The sequences of test_mala_host.py's path tests, by name: (case, keyword arguments of run_sequence).  test_gpu_mala.py runs the
    same on the device and compares with the mirror."""
    case = draw(11, 5, 5, 3, log=True, ss=1)
    out = {"plain": (case, {}), "max_iter_2": (with_desc(case, max_iter=2), {}), "no_samples": (case, dict(samples=False)),
           "thin_2_cap_2": (with_desc(case, thin=2, sample_cap=2), {})}
    ev = copy_evals(case)
    ev[0]["status"].reshape(5, 3)[2, 1] = 2           # chain 2: its start cannot be evaluated
    ev[0]["sse"].reshape(5, 3)[3, 0] = np.inf         # chain 3: an infinite sum
    out["bad_start"] = (case, dict(evals=ev))
    outside = dict(case, x0=case["x0"].copy())
    outside["x0"][4, 0] = 0.05                        # chain 4 starts outside the box
    out["start_outside"] = (outside, {})
    fixed = draw(12, 5, 4, 3, log=True, ss=0)
    ev = copy_evals(fixed)
    ev[0]["jtj"].reshape(5, 3, fixed["npar"], fixed["npar"])[1] = 0.0        # chain 1: J^T J = 0 at the start, with no ridge
    ev[0]["jtj"].reshape(5, 3, fixed["npar"], fixed["npar"])[3, 2, fixed["free"][2], fixed["free"][0]] = np.nan   # chain 3: a NaN entry
    out["degenerate_start"] = (with_desc(fixed, ridge=0.0), dict(evals=ev))
    ev = copy_evals(fixed)
    for e in ev[1:4]:
        e["jtj"].reshape(5, 3, fixed["npar"], fixed["npar"])[1] = 0.0        # chain 1: proposals whose metric is zero ...
        e["sse"].reshape(5, 3)[1] = 0.0                                      # ... at a sum of squares that looks perfect
        e["jtj"].reshape(5, 3, fixed["npar"], fixed["npar"])[3, 0, fixed["free"][1], fixed["free"][1]] = np.nan   # chain 3: a NaN entry
        e["sse"].reshape(5, 3)[3] = 0.0
    out["bad_trial_metric"] = (with_desc(fixed, ridge=0.0), dict(evals=ev))
    corner = draw(13, 5, 4, 1, log=False, ss=0)
    corner["x0"][:] = corner["hi"]                    # on the box's corner with a long first step: most proposals leave it
    for e in corner["evals"][1:]:
        e["sse"][:] = 0.0                             # ... and whatever is evaluated for them looks perfect
    out["corner"] = (corner, dict(eps0=3.0))
    failed = draw(17, 5, 4, 3, log=True, ss=0)
    for e in failed["evals"][1:]:
        e["sse"][:] = 0.0
        e["status"].reshape(5, 3)[:, 1] = 1           # every proposal fails, with a value that would be accepted
    out["failed_status"] = (failed, {})
    return out


# ---- analytic targets for the stand-in solver of the distribution tests ----

def gn_solver(resid, free, P, calls=None):
    """A stand-in with sensitivity.gauss_newton's signature: resid(x [nf]) -> (r [m], J [m, nf]), the residuals of a chain and their
    derivatives with respect to the PARAMETERS; protocol p of a chain contributes 1 / P of r . r, J^T r and J^T J.  calls receives the
    row count of every evaluation."""
    free = list(free)
    def solver(model, params, prot_v, y0, t_eval, sse_ref, **kw):
        p = params.numpy()
        B, npar = p.shape
        if calls is not None:
            calls.append(B)
        assert y0.shape[0] == B and kw["prot_of_traj"].shape[0] == B and sse_ref is not None
        sse, jtr, jtj, status = np.zeros(B), np.zeros((B, npar)), np.zeros((B, npar, npar)), np.zeros(B, dtype=np.int32)
        for b in range(B):
            if not np.isfinite(p[b]).all():
                sse[b], status[b] = np.inf, 2
                continue
            r, J = resid(p[b, free])
            sse[b] = float(r @ r) / P
            jtr[b, free] = (J.T @ r) / P
            jtj[b][np.ix_(free, free)] = (J.T @ J) / P
        return torch.from_numpy(sse), torch.from_numpy(jtr), torch.from_numpy(jtj), torch.from_numpy(status)
    return solver


def gn_sums(resid):
    """reference_chains' gn from a residual function: the sums over a chain's protocols."""
    def gn(x):
        r, J = resid(x)
        return float(r @ r), J.T @ r, J.T @ J
    return gn


def gauss_problem(log):
    """mcmc_cases.gauss_problem as residuals: r = A (u - c) with A^T A = Sigma^-1, so S = d^T Sigma^-1 d and J_u = A.  With log
    parameters u = log x and the solver's J_x = A diag(1 / x): the step's chain rule has to give A back."""
    import mcmc_cases as M
    pb = M.gauss_problem(log)
    A = np.linalg.cholesky(M.GAUSS_PREC).T
    centre = pb["centre"]
    def resid(x):
        u = np.log(x) if log else x
        return A @ (u - centre), (A / x[None, :] if log else A)
    return dict(pb, resid=resid)


DECAY_T = np.linspace(0.0, 4.0, 40)
DECAY_SIGMA, DECAY_TRUE = 0.05, np.array([1.0, 0.7])
DECAY_DATA = DECAY_TRUE[0] * np.exp(-DECAY_TRUE[1] * DECAY_T) + DECAY_SIGMA * np.random.default_rng(31).normal(size=40)
DECAY_BOUNDS = (np.array([0.5, 0.35]), np.array([2.0, 1.4]))


def decay_problem():
    """A metric that depends on the position: i_k = x1 exp(-x2 t_k), 40 samples on [0, 4], noise of sigma 0.05 from a fixed seed,
    log parameters, the box a factor two either side of the truth; 64 starts at the truth times exp(0.05)."""
    def resid(x):
        e = np.exp(-x[1] * DECAY_T)
        return x[0] * e - DECAY_DATA, np.stack([e, -x[0] * DECAY_T * e], axis=1)
    return dict(resid=resid, x0=np.tile(DECAY_TRUE * math.exp(0.05), (64, 1)), bounds=DECAY_BOUNDS)


def decay_quadrature(m=801):
    """Mean and variance of u = log x under the posterior exp(-S / (2 sigma^2)) with the prior uniform in u over the box: a grid of
    m x m points over +- 8 Laplace standard deviations around the mode (trapezoid; the integrand is below 1e-13 of its peak there)."""
    def S_of(u1, u2):
        i = np.exp(u1)[..., None] * np.exp(-np.exp(u2)[..., None] * DECAY_T)
        return ((i - DECAY_DATA) ** 2).sum(axis=-1)
    u = np.log(DECAY_TRUE)
    for _ in range(20):                               # Gauss-Newton to the mode
        x = np.exp(u)
        e = np.exp(-x[1] * DECAY_T)
        r, J = x[0] * e - DECAY_DATA, np.stack([e, -x[0] * DECAY_T * e], axis=1) * x[None, :]
        u = u - np.linalg.solve(J.T @ J, J.T @ r)
    sd = np.sqrt(np.diag(np.linalg.inv(J.T @ J / DECAY_SIGMA ** 2)))
    g1, g2 = np.linspace(u[0] - 8 * sd[0], u[0] + 8 * sd[0], m), np.linspace(u[1] - 8 * sd[1], u[1] + 8 * sd[1], m)
    assert g1[0] > math.log(DECAY_BOUNDS[0][0]) and g1[-1] < math.log(DECAY_BOUNDS[1][0])
    assert g2[0] > math.log(DECAY_BOUNDS[0][1]) and g2[-1] < math.log(DECAY_BOUNDS[1][1])
    U1, U2 = np.meshgrid(g1, g2, indexing="ij")
    S = S_of(U1, U2)
    w = np.exp(-(S - S.min()) / (2 * DECAY_SIGMA ** 2))
    w /= w.sum()
    mean = np.array([(w * U1).sum(), (w * U2).sum()])
    var = np.array([(w * (U1 - mean[0]) ** 2).sum(), (w * (U2 - mean[1]) ** 2).sum()])
    return mean, var


def sigma_problem():
    """mcmc_cases.sigma_problem as residuals: r = (sqrt(S0), sqrt(kappa) (x - x*)), so S = S0 + kappa (x - x*)^2 with N = 50."""
    import mcmc_cases as M
    pb = M.sigma_problem()
    def resid(x):
        return np.array([math.sqrt(M.SIG_S0), math.sqrt(M.SIG_KAPPA) * (x[0] - M.SIG_XSTAR)]), np.array([[0.0], [math.sqrt(M.SIG_KAPPA)]])
    return dict(pb, resid=resid)


def sigma_quadrature(m=4001):
    """E[x] and E[sigma^2] of sigma_problem's posterior by quadrature.  Integrating log sigma out of sigma^-N exp(-S / (2 sigma^2))
    over the whole line leaves S(x)^(-N / 2) (the bounds 0.05 .. 20 cut off less than 1e-30 of it), and E[sigma^2 | x] = S / (N - 2)."""
    import mcmc_cases as M
    x = np.linspace(M.SIG_XSTAR - 1.0, M.SIG_XSTAR + 1.0, m)
    S = M.SIG_S0 + M.SIG_KAPPA * (x - M.SIG_XSTAR) ** 2
    w = np.exp(-0.5 * M.SIG_N * (np.log(S) - np.log(S).min()))
    w[[0, -1]] *= 0.5
    w /= w.sum()
    return float((w * x).sum()), float((w * S).sum() / (M.SIG_N - 2))


# ---- the runs of test_gpu_mala.py on the real evaluation ----

def step_protocols(npts):
    """Two step protocols on a 0.1 ms grid of npts points: hold -80 mV, a depolarising step to +40 / +10 mV, then -50 / -110 mV."""
    pv = np.full((2, npts), -80.0)
    a, b, c = npts // 10, npts // 2, (4 * npts) // 5
    pv[0, a:b], pv[0, b:c] = 40.0, -50.0
    pv[1, a:b], pv[1, b:c] = 10.0, -110.0
    return pv
