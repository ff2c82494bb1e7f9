"""Shared inputs of the CMA-ES tests (test_cmaes_host.py, test_cmaes_driver_host.py, test_gpu_cmaes.py) and a plain numpy statement
of the algorithm of include/ionode.h "CMA-ES step": the same generator (Philox4x32-10, the step's logarithm, AS241 PPND16), the same
formulas (Hansen's tutorial, arXiv 1604.00772, positive weights) and numpy.linalg.eigh where the library runs cyclic Jacobi.  It is
the checker: no CMA-ES package is assumed.  Python floats are IEEE doubles and nothing here contracts a product into an fma, so the
generator below is bit for bit the library's; the update formulas sum in numpy's order and are compared to rounding bounds."""
import importlib
import math
import struct

import numpy as np
import torch

EPS = np.finfo(np.float64).eps
N_CASES, P_CASES, K_CASES = (1, 4, 12), (1, 3), (1, 67)
M32 = 0xFFFFFFFF


def mods():
    ion = importlib.import_module("neural-ode-ion-channels_amd")
    return ion.capi, importlib.import_module("neural-ode-ion-channels_amd.cmaes")


def lam_cases(n):
    """default, 2, 64"""
    return (mods()[0].cmaes_default_lambda(n), 2, 64)


# ---- the generator ----

def philox4x32(ctr, key, rounds=10):
    """Philox4x32 (Salmon et al., SC'11) on Python integers: counter [4], key [2] -> 4 words."""
    c0, c1, c2, c3 = (int(c) & M32 for c in ctr)
    k0, k1 = (int(k) & M32 for k in key)
    for _ in range(rounds):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = ((p1 >> 32) ^ c1 ^ k0) & M32, p1 & M32, ((p0 >> 32) ^ c3 ^ k1) & M32, p0 & M32
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return [c0, c1, c2, c3]


_LOG_COEF = [1.0 / k for k in (23.0, 21.0, 19.0, 17.0, 15.0, 13.0, 11.0, 9.0, 7.0, 5.0, 3.0)]
LN2_HI, LN2_LO, SQRT2 = float.fromhex("0x1.62e42fee00000p-1"), float.fromhex("0x1.a39ef35793c76p-33"), float.fromhex("0x1.6a09e667f3bcdp+0")


def det_log(x):
    """The step's logarithm (csrc/ionode_cmaes.hpp cm_log), operation for operation."""
    x = float(x)
    if x != x or x < 0.0:
        return math.nan
    if x == 0.0:
        return -math.inf
    if x == math.inf:
        return x
    e = 0
    b = struct.unpack("<Q", struct.pack("<d", x))[0]
    if (b >> 52) == 0:
        x = x * 2.0 ** 54
        b = struct.unpack("<Q", struct.pack("<d", x))[0]
        e = -54
    e += (b >> 52) - 1023
    m = struct.unpack("<d", struct.pack("<Q", (b & 0x000FFFFFFFFFFFFF) | 0x3FF0000000000000))[0]
    if m > SQRT2:
        m, e = m * 0.5, e + 1
    s = (m - 1.0) / (m + 1.0)
    z = s * s
    p = _LOG_COEF[0]
    for c in _LOG_COEF[1:]:
        p = p * z + c
    lm = 2.0 * s + (2.0 * s) * (z * p)
    ed = float(e)
    return (ed * LN2_HI + lm) + ed * LN2_LO


def _horner(c, r):
    v = c[0] * r + c[1]
    for x in c[2:]:
        v = v * r + x
    return v


_A = (2509.0809287301226727, 33430.575583588128105, 67265.770927008700853, 45921.953931549871457, 13731.693765509461125,
      1971.5909503065514427, 133.14166789178437745, 3.387132872796366608)
_B = (5226.495278852545925, 28729.085735721942674, 39307.89580009271061, 21213.794301586595867, 5394.1960214247511077,
      687.1870074920579083, 42.313330701600911252, 1.0)
_C = (7.7454501427834140764e-4, 0.0227238449892691845833, 0.24178072517745061177, 1.27045825245236838258, 3.64784832476320460504,
      5.7694972214606914055, 4.6303378461565452959, 1.42343711074968357734)
_D = (1.05075007164441684324e-9, 5.475938084995344946e-4, 0.0151986665636164571966, 0.14810397642748007459, 0.68976733498510000455,
      1.6763848301838038494, 2.05319162663775882187, 1.0)
_E = (2.01033439929228813265e-7, 2.71155556874348757815e-5, 0.0012426609473880784386, 0.026532189526576123093, 0.29656057182850489123,
      1.7848265399172913358, 5.4637849111641143699, 6.6579046435011037772)
_F = (2.04426310338993978564e-15, 1.4215117583164458887e-7, 1.8463183175100546818e-5, 7.868691311456132591e-4, 0.0148753612908506148525,
      0.13692988092273580531, 0.59983224863253602715, 1.0)


def ppnd16(p):
    """Wichura's AS241 PPND16 with det_log in the tails."""
    q = p - 0.5
    if abs(q) <= 0.425:
        r = 0.180625 - q * q
        return q * _horner(_A, r) / _horner(_B, r)
    r = p if q < 0.0 else 1.0 - p
    r = math.sqrt(-det_log(r))
    if r <= 5.0:
        r = r - 1.6
        v = _horner(_C, r) / _horner(_D, r)
    else:
        r = r - 5.0
        v = _horner(_E, r) / _horner(_F, r)
    return -v if q < 0.0 else v


def uniform(hi, lo):
    return (float((hi << 21) | (lo >> 11)) + 0.5) * 2.0 ** -53


def draw_words(seed, run, gen, cand, pair, attempt):
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    return philox4x32([run, gen, cand, pair + 65536 * attempt], [seed & M32, seed >> 32])


def normal_pair(seed, run, gen, cand, pair, attempt):
    w = draw_words(seed, run, gen, cand, pair, attempt)
    return ppnd16(uniform(w[0], w[1])), ppnd16(uniform(w[2], w[3]))


def normals(seed, run, gen, cand, n, attempt):
    z = []
    for jp in range((n + 1) // 2):
        z += list(normal_pair(seed, run, gen, cand, jp, attempt))
    return np.array(z[:n])


# ---- the algorithm ----

def constants(n, lam):
    """Strategy constants of the tutorial's table 1 (positive weights), the weights through det_log as the library forms them."""
    mu = lam // 2
    ln_mu_half = det_log(mu + 0.5)
    raw = np.array([ln_mu_half - det_log(float(i)) for i in range(1, mu + 1)])
    sw = 0.0
    for r in raw:
        sw = sw + r
    w = raw / sw
    mu_eff = 1.0 / float(np.sum(w * w))
    cs = (mu_eff + 2.0) / (n + mu_eff + 5.0)
    ds = 1.0 + 2.0 * max(0.0, math.sqrt((mu_eff - 1.0) / (n + 1.0)) - 1.0) + cs
    cc = (4.0 + mu_eff / n) / (n + 4.0 + 2.0 * mu_eff / n)
    c1 = 2.0 / ((n + 1.3) ** 2 + mu_eff)
    cmu = min(1.0 - c1, 2.0 * (mu_eff - 2.0 + 1.0 / mu_eff) / ((n + 2.0) ** 2 + mu_eff))
    chi_n = math.sqrt(n) * (1.0 - 1.0 / (4.0 * n) + 1.0 / (21.0 * n * n))
    return dict(mu=mu, w=w, mu_eff=mu_eff, cs=cs, ds=ds, cc=cc, c1=c1, cmu=cmu, chi_n=chi_n)


def ask_point(seed, run, gen, k, m, sigma, B, D, ulo, uhi, resamples=8):
    """Candidate k of a generation: (u after redraws and clipping, attempts used beyond the first, clipped?).  The sums run in the
    library's written order, so u is the library's bit for bit."""
    n = len(m)
    for attempt in range(resamples + 1):
        dz = D * normals(seed, run, gen, k, n, attempt)
        u = np.empty(n)
        for j in range(n):
            s = 0.0
            for l in range(n):
                s = s + B[j, l] * dz[l]
            u[j] = m[j] + sigma * s
        if ((u >= ulo) & (u <= uhi)).all():
            return u, attempt, False
    return np.minimum(np.maximum(u, ulo), uhi), resamples, True


def ranks(f):
    """Rank of every candidate by (f, index): ties and infs in index order."""
    order = sorted(range(len(f)), key=lambda k: (f[k], k))
    r = np.empty(len(f), dtype=int)
    r[order] = np.arange(len(f))
    return r


def tell(st, pop, f, c, tells):
    """One tell on a state dict (m, sigma, pc, ps, C), the points pop [lam, n] as evaluated and their values f [lam] (inf: failed), with
    numpy.linalg.eigh for C^-1/2.  tells counts this one.  Returns the new dict (with hsig), or None with fewer than mu finite values."""
    n = len(st["m"])
    if np.isfinite(f).sum() < c["mu"]:
        return None
    r = ranks(f)
    w = np.where(r < c["mu"], c["w"][np.minimum(r, c["mu"] - 1)], 0.0)
    y = (pop - st["m"][None]) / st["sigma"]
    yw = w @ y
    ev, E = np.linalg.eigh(st["C"])
    inv_sqrt = (E / np.sqrt(ev)) @ E.T
    ps = (1.0 - c["cs"]) * st["ps"] + math.sqrt(c["cs"] * (2.0 - c["cs"]) * c["mu_eff"]) * (inv_sqrt @ yw)
    norm = float(np.linalg.norm(ps))
    sigma = st["sigma"] * math.exp(min(1.0, (c["cs"] / c["ds"]) * (norm / c["chi_n"] - 1.0)))
    hsig = 1.0 if norm / math.sqrt(1.0 - (1.0 - c["cs"]) ** (2 * tells)) / c["chi_n"] < 1.4 + 2.0 / (n + 1.0) else 0.0
    pc = (1.0 - c["cc"]) * st["pc"] + hsig * math.sqrt(c["cc"] * (2.0 - c["cc"]) * c["mu_eff"]) * yw
    keep = 1.0 - c["c1"] - c["cmu"] + (1.0 - hsig) * c["c1"] * c["cc"] * (2.0 - c["cc"])
    C = keep * (0.5 * (st["C"] + st["C"].T)) + c["c1"] * np.outer(pc, pc) + c["cmu"] * np.einsum("k,ki,kl->il", w, y, y)
    return dict(m=st["m"] + st["sigma"] * yw, sigma=sigma, pc=pc, ps=ps, C=C, hsig=hsig, yw=yw, w=w)


def reference_run(fn, u0, *, lam=None, sigma0=0.1, seed=0, run=0, target, max_gen, ulo=None, uhi=None):
    """The whole algorithm on one run in numpy: minimise fn(u) from the mean u0 until the best value is <= target.  Returns
    (generations told, best value).  (tools/bench_cmaes.py runs it as the loop a user had before.)"""
    n = len(u0)
    capi, _ = mods()
    lam = capi.cmaes_default_lambda(n) if lam is None else lam
    c = constants(n, lam)
    ulo = np.full(n, -np.inf) if ulo is None else ulo
    uhi = np.full(n, np.inf) if uhi is None else uhi
    st = dict(m=np.array(u0, dtype=float), sigma=sigma0, pc=np.zeros(n), ps=np.zeros(n), C=np.eye(n))
    B, D, best = np.eye(n), np.ones(n), np.inf
    for g in range(max_gen):
        pop = np.stack([ask_point(seed, run, g, k, st["m"], st["sigma"], B, D, ulo, uhi)[0] for k in range(lam)])
        f = np.array([fn(u) for u in pop])
        f = np.where(np.isfinite(f), f, np.inf)
        best = min(best, float(f.min()))
        if best <= target:
            return g + 1, best
        st = tell(st, pop, f, c, g + 1)
        if st is None:
            return g + 1, best
        ev, B = np.linalg.eigh(st["C"])
        D = np.sqrt(np.maximum(ev, 0.0))
    return max_gen, best


# ---- analytic objectives for the stand-in solver: functions of the free parameters x (the step's search variable is log x or x) ----

def sphere(x):
    return float(np.sum((x - 1.0) ** 2))


ELLIPSOID_SCALES = 10.0 ** (6.0 * np.arange(12) / 11.0)   # condition 1e6


def ellipsoid(x):
    return float(np.sum(ELLIPSOID_SCALES[:len(x)] * (x - 1.0) ** 2))


def rosenbrock(x):
    return float(np.sum(100.0 * (x[1:] - x[:-1] ** 2) ** 2 + (1.0 - x[:-1]) ** 2))


def analytic_solver(fn, free, P, calls=None, kinds=None):
    """Stand-in with batched.solve's signature on CPU tensors: protocol p of a candidate contributes fn(x) / P (P a power of two keeps
    the sum of the P parts exact), a non-finite row fails with status 2.  calls / kinds receive the trajectory count and the
    objective kind of every evaluation."""
    from types import SimpleNamespace

    def solver(model, params, prot_v, y0, t_eval, **kw):
        p = params.numpy()
        if calls is not None:
            calls.append(p.shape[0])
        if kinds is not None:
            kinds.append((model, kw.get("objective", "sse")))
        assert kw["states"] is False and kw["sse_ref"] is not None and y0.shape[0] == p.shape[0] and kw["prot_of_traj"].shape[0] == p.shape[0]
        val, status = np.zeros(p.shape[0]), np.zeros(p.shape[0], dtype=np.int32)
        for b in range(p.shape[0]):
            if not np.isfinite(p[b]).all():
                val[b], status[b] = np.inf, 2
            else:
                val[b] = fn(p[b, list(free)]) / P
        out = torch.from_numpy(val)
        kind = kw.get("objective", "sse")
        return SimpleNamespace(sse=out if kind == "sse" else None, sae=out if kind == "sae" else None, status=torch.from_numpy(status))
    return solver


# ---- seeded cases for the step itself ----

def free_columns(n, npar):
    return [(5 * j + 3) % npar for j in range(n)]   # a permutation of the columns, not in order


def draw(seed, K, n, lam, P, *, log, bounds=False, **desc_kw):
    """One drawn case: starts x0 [K, n], a descriptor, and the value / status arrays of three consecutive tells (the first call only
    samples and reads nothing).  Values are seeded and carry ties and failures."""
    capi, cm = mods()
    rng = np.random.default_rng(seed)
    npar = 12 if n > 8 else (8 if seed % 2 == 0 else 12)
    free = free_columns(n, npar)
    base = rng.uniform(0.5, 2.0, npar)
    x0 = rng.uniform(0.5, 2.0, (K, n))
    lo, hi = (np.full(n, 0.45), np.full(n, 2.2)) if bounds else (None, None)
    kw = dict(max_iter=50, unchanged_iters=100, unchanged_threshold=1e-3, tolx=1e-300, seed=1234 + seed)
    kw.update(desc_kw)
    desc = cm.cmaes_desc(K, lam, P, npar, free, base, log_parameters=log, lo=lo, hi=hi, **kw)
    evals = []
    for g in range(3):
        value = rng.uniform(1.0, 2.0, K * lam * P) * 0.5 ** g
        status = np.zeros(K * lam * P, dtype=np.int32)
        if lam >= 8:
            v = value.reshape(K, lam, P)
            v[:, 3] = v[:, 1]                          # a tie: the index decides
            s = status.reshape(K, lam, P)
            s[:, 2, P - 1] = 3                         # a failure whose value is finite: the status alone decides
            v[:, 5, 0] = np.nan                        # ... and a NaN ranks as one
        evals.append(dict(value=value, status=status))
    return dict(K=K, n=n, lam=lam, P=P, npar=npar, free=free, base=base, x0=x0, log=log, lo=lo, hi=hi, desc=desc, evals=evals,
                seed=kw["seed"])


def start(case, sigma0=0.1, scale=None):
    _, cm = mods()
    return [torch.from_numpy(a) for a in cm.cmaes_init(case["x0"], case["desc"], sigma0, scale)]


def slot_rows(active, per):
    return np.concatenate([np.arange(c * per, (c + 1) * per) for c in active])


def run_sequence(case, device="cpu", active=None, sigma0=0.1, scale=None, evals=None, calls=None):
    """The case's consecutive calls through cmaes.cmaes_step on `device` (CPU tensors: the host mirror; HIP tensors: the kernel): the
    first samples, every later one tells an evaluation.  Returns after every call numpy copies of (state, flag, iters, trial)."""
    capi, cm = mods()
    desc = capi.IonodeCmaesDesc.from_buffer_copy(case["desc"])
    state, flag, iters, trial = (t.to(device) for t in start(case, sigma0, scale))
    per = case["lam"] * case["P"]
    act, rows = None, None
    if active is not None:
        act = torch.tensor(list(active), dtype=torch.int32, device=device)
        rows = slot_rows(active, per)
        trial = trial[torch.from_numpy(rows).to(device)].contiguous()
    evals = case["evals"] if evals is None else evals
    n_rows = trial.shape[0]
    feed = [dict(value=np.zeros(case["K"] * per), status=np.zeros(case["K"] * per, dtype=np.int32))] + list(evals)
    out = []
    for ev in feed[:(len(evals) + 1 if calls is None else calls)]:
        pick = (lambda a: a) if rows is None else (lambda a: a[rows])
        value = torch.from_numpy(np.ascontiguousarray(pick(ev["value"]))).to(device)
        status = torch.from_numpy(np.ascontiguousarray(pick(ev["status"]))).to(device)
        assert value.shape[0] == n_rows
        cm.cmaes_step(desc, act, value, status, state, flag, iters, trial)
        out.append(tuple(x.cpu().numpy().copy() for x in (state, flag, iters, trial)))
    return out


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---- the HH 2-state fit of test_cmaes_driver_host.py (CPU oracle as the solver) and test_gpu_cmaes.py (the GPU solve) ----

HH_RTOL, HH_ATOL = 1e-8, 1e-10
HH_FREE = (0, 1, 2, 3)
HH_SEED = 7


def hh_problem():
    """Two 200 ms step protocols (0.1 ms grid), 2001 samples: 20 ms at -80 mV, 80 ms at +40 / +10 mV, 60 ms at -50 / -110 mV, then
    -80 mV -- an activating and a deactivating step each, at four voltages besides the hold, so that p1 .. p4 are all visible in the
    data.  The known parameters are the HH ground truth with the activation gate twenty times faster (p1, p3 x 20): its time
    constants (16 ms at +40 mV, 35 ms at -80 mV) then fit the 200 ms.  The reference's box p / 10 .. 10 p, four starts p exp(0.1 N(0, 1))."""
    import kat_cases as K
    pv = np.full((2, 2001), -80.0)
    pv[0, 200:1000], pv[0, 1000:1600] = 40.0, -50.0
    pv[1, 200:1000], pv[1, 1000:1600] = 10.0, -110.0
    te = np.linspace(0.0, 200.0, 2001)
    true = K.P_HH.copy()
    true[[0, 2]] *= 20.0
    rng = np.random.default_rng(5)
    starts = true[None, :4] * np.exp(0.1 * rng.normal(size=(4, 4)))
    return dict(pv=pv, te=te, true=true, lo=true[:4] / 10.0, hi=true[:4] * 10.0, starts=starts, prot_dt=0.1)


HH_BUDGET = 300                  # the issue's cap on the CPU fit
HH_GENERATIONS = (57, 74, 62, 74)   # measured on the CPU (test_cmaes_driver_host.py::test_hh_fit_with_the_cpu_oracle_as_the_solver), runs 0 .. 3


def hh_data_oracle(oracle, pb):
    """The two current traces [2, 2001] of the CPU oracle at the known parameters (fp64 state)."""
    import kat_cases as K
    r = oracle.solve(K.MODEL_HH2, np.tile(pb["true"], (2, 1)), pb["pv"], [0.0, 1.0], pb["te"], prot_t0=0.0, prot_dt=pb["prot_dt"],
                     prot_of_traj=np.arange(2, dtype=np.int32), state_f32=False, rtol=HH_RTOL, atol=HH_ATOL, max_step=0.0)
    assert (r["status"] == 0).all()
    return np.stack([oracle.current(r["y"][k], oracle.protocol_v(pb["pv"][k], pb["te"], prot_t0=0.0, prot_dt=pb["prot_dt"])[0], state_f32=False)
                     for k in range(2)])


def hh_start_values(solver, pb, data, device="cpu"):
    """The sum of squares of the four starts themselves, through `solver` (batched.solve or a stand-in with its signature)."""
    import kat_cases as K
    p = np.repeat(np.tile(pb["true"], (4, 1)), 2, axis=0)
    p[:, :4] = np.repeat(pb["starts"], 2, axis=0)
    sol = solver(K.MODEL_HH2, torch.from_numpy(p), torch.from_numpy(pb["pv"]), torch.tensor([[0.0, 1.0]], dtype=torch.float64).expand(8, 2).contiguous(),
                 torch.from_numpy(pb["te"]), prot_t0=0.0, prot_dt=pb["prot_dt"], prot_of_traj=torch.from_numpy(np.tile(np.arange(2, dtype=np.int32), 4)),
                 rtol=HH_RTOL, atol=HH_ATOL, max_step=0.0, sse_ref=torch.from_numpy(data), states=False, objective="sse",
                 **({} if device == "cpu" else {"device": device}))
    assert (sol.status.cpu().numpy() == 0).all()
    return sol.sse.cpu().numpy().reshape(4, 2).sum(axis=1)


def hh_fit(pb, data, solver, device, start, *, max_iter, stop_early=True):
    """The fit: four runs, lambda = 8, two protocols -- 64 trajectories a generation.  Returns ({run: generations told when its best
    value first was <= 1e-6 of its start's}, best value after every step [steps, 4], minimise's result or None when stopped early --
    stop_early ends the loop once every run is there)."""
    capi, cm = mods()
    first, history = {}, []

    class Done(Exception):
        pass

    def watch(it, state, flag, iters):
        best = capi.cmaes_state_views(state, 4, 8)["best_f"].cpu().numpy().copy()
        history.append(best)
        for k in range(4):
            if best[k] <= 1e-6 * start[k]:
                first.setdefault(k, it)
        if stop_early and len(first) == 4:
            raise Done

    out = None
    try:
        out = cm.minimise(0, pb["starts"], pb["pv"], data, pb["te"], base_params=pb["true"], free=HH_FREE, bounds=(pb["lo"], pb["hi"]),
                          prot_dt=pb["prot_dt"], state_dtype=torch.float64, rtol=HH_RTOL, atol=HH_ATOL, max_step=0.0, seed=HH_SEED, max_iter=max_iter,
                          unchanged_iters=10 ** 6, unchanged_threshold=0.0, tolx=0.0, compact_every=None, solver=solver, device=device,
                          callback=watch if stop_early is not None else None)
    except Done:
        pass
    return first, np.array(history), out


def oracle_solver(oracle, calls=None):
    """The CPU oracle behind batched.solve's signature: fp64 state, the fused sum of squares (or absolute values) formed here from its
    current traces."""
    from types import SimpleNamespace

    def solver(model, params, prot_v, y0, t_eval, **kw):
        p, te, pv = params.numpy(), t_eval.numpy(), prot_v.numpy()
        pot = kw["prot_of_traj"].numpy()
        if calls is not None:
            calls.append(p.shape[0])
        r = oracle.solve(model, p, pv, [0.0, 1.0], te, prot_t0=kw["prot_t0"], prot_dt=kw["prot_dt"], prot_of_traj=pot, state_f32=False,
                         rtol=kw["rtol"], atol=kw["atol"], max_step=kw["max_step"])
        ref = kw["sse_ref"].numpy()
        val = np.full(p.shape[0], np.inf)
        volt = [oracle.protocol_v(pv[k], te, prot_t0=kw["prot_t0"], prot_dt=kw["prot_dt"])[0] for k in range(pv.shape[0])]
        for b in range(p.shape[0]):
            if r["status"][b] == 0:
                res = oracle.current(r["y"][b], volt[pot[b]], state_f32=False) - ref[pot[b]]
                val[b] = float(np.sum(res * res)) if kw.get("objective", "sse") == "sse" else float(np.sum(np.abs(res)))
        out = torch.from_numpy(val)
        kind = kw.get("objective", "sse")
        return SimpleNamespace(sse=out if kind == "sse" else None, sae=out if kind == "sae" else None,
                               status=torch.from_numpy(r["status"].astype(np.int32)))
    return solver


# ---- the NN-d fit of test_gpu_cmaes.py: a seeded net of width 10 around the HH rates, the absolute-residual objective ----

NND_LAYERS, NND_WIDTH, NND_SEED = 2, 10, 11
NND_GENERATIONS = 60   # twice what the numpy statement needs on the CPU oracle (test_gpu_cmaes.py::test_nnd_fit_with_the_absolute_objective)


def nnd_problem():
    """hh_problem()'s protocols and grid; a seeded (2, 10) net in the reference's flat state-dict order, weights N(0, 0.3^2 / fan-in);
    the HH ground truth as the known rate parameters, p1 .. p4 free; two starts p exp(0.3 N(0, 1))."""
    pb = hh_problem()
    L_, N = NND_LAYERS, NND_WIDTH
    rng = np.random.default_rng(17)
    parts = [rng.normal(0.0, 0.3 / np.sqrt(2.0), 2 * N), np.zeros(N)]
    for _ in range(L_):
        parts += [rng.normal(0.0, 0.3 / np.sqrt(N), N * N), np.zeros(N)]
    parts += [rng.normal(0.0, 0.3 / np.sqrt(N), N), np.zeros(1)]
    pb["weights"] = np.concatenate(parts).astype(np.float32)
    pb["starts"] = pb["true"][None, :4] * np.exp(0.3 * rng.normal(size=(2, 4)))
    return pb
