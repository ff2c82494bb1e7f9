"""Dev/bench tool (GPU box): one adaptive-Metropolis iteration of K chains (mcmc.py: the fused forward solve + ionode_mcmc_step) beside
the loop a caller had before -- objective.population_sum_of_squares on all chains' proposals, one device-to-host read, and a numpy
adaptive-Metropolis step per chain on the host (the same rule, numpy's own generator and numpy.linalg.cholesky, as a user would write
it).  Writes profiles/mcmc_sampling.md and prints one JSON line.

HH 2-state, p1 .. p4 free in log parameters plus sampled sigma, fp64 state, --nt samples, one sine-wave protocol with noise of sigma
0.1 on the data, the reference's box p / 10 .. 10 p, K chains = K trajectories an iteration.  Per case, best of the iterations after
the first (ms):
  solve_ms            the fused forward solve of the iteration (solve_mean_ms: its mean -- the iterations' points differ, and with
                      them the solves' step counts)
  step_ms             ionode_mcmc_step (tell + proposal)
  iteration_ms        mcmc.sample's own loop, per iteration (nothing timed inside it)
  host_iteration_ms   the host loop's iteration; host_sampler_ms = that minus the evaluation inside it
Every case runs in a child process of its own under `timeout`; a child that fails ends the run.
python tools/bench_mcmc.py [--chains 8,512,8192] [--nt 20001] [--iters 8] [--timeout 280] [--out profiles/mcmc_sampling.md]"""
import argparse
import importlib
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--chains", default="8,512,8192")
ap.add_argument("--nt", type=int, default=20001)
ap.add_argument("--iters", type=int, default=8)
ap.add_argument("--timeout", type=int, default=280)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mcmc_sampling.md"))
ap.add_argument("--child", default="")
a = ap.parse_args()


def report(cases):
    def row(c):
        if "error" in c:
            return f"| {c['chains']} | {c['error']} |"
        return (f"| {c['chains']:,} | {c['Nt']:,} | {c['solve_ms']:.2f} | {c['solve_mean_ms']:.2f} | {c['step_ms']:.3f} | {c['iteration_ms']:.2f} | "
                f"{100.0 * c['step_ms'] / c['iteration_ms']:.1f} % | {c['host_iteration_ms']:.2f} | {c['host_sampler_ms']:.2f} |").replace(",", " ")
    ok = [c for c in cases if "error" not in c]
    head = ok[0] if ok else {}
    over = [c["chains"] for c in ok if c["step_ms"] > 0.05 * c["iteration_ms"]]
    return "\n".join([
        "# Batched adaptive Metropolis (`mcmc.py`, `ionode_mcmc_step`): the per-iteration split",
        "",
        f"Library sha256 `{head.get('library_sha256', '?')}`, one {head.get('gpu', 'GPU')}; written by `tools/bench_mcmc.py`.",
        "",
        "HH 2-state, p1 .. p4 free in log parameters plus sampled sigma (five coordinates), fp64 state, one sine-wave protocol, noise of",
        "sigma 0.1 on the data, the box p / 10 .. 10 p, rtol 1e-7 / atol 1e-9, no step cap; one trajectory per chain and iteration.  Best of",
        "the iterations after the first (and the solve's mean over them: `mcmc.sample` per iteration is a mean too), ms; every case in a",
        "process of its own.  The host loop is `objective.population_sum_of_squares` on the proposals, one device-to-host read, and a numpy",
        "adaptive-Metropolis step per chain (the same rule with numpy's generator and `numpy.linalg.cholesky`).",
        "",
        "| chains | samples | fused solve, best | mean | `ionode_mcmc_step` | `mcmc.sample` per iteration | step / iteration | host loop per iteration | of which the numpy sampler and the read |",
        "|---:|---:|---:|---:|---:|---:|---:|---:|---:|",
        *[row(c) for c in cases],
        "",
        "Nobody had measured these numbers before this table; it sets no target.  The step is one lane per chain (`csrc/ionode_mcmc.hpp`):",
        "no scratch, no LDS, 103 registers at five coordinates, 296 at thirteen (`tests/test_mcmc_kernel_resources.py`).",
        ("The step is above 5 % of an iteration at " + ", ".join(str(k) for k in over) + " chains: an iteration there is one short solve launch, and the step's "
         "launch is a fixed cost beside it." if over else "The step stays below 5 % of an iteration at every size."),
        ""])


if not a.child:   # the parent never opens the GPU
    cases = []
    for n in [int(s) for s in a.chains.split(",")]:
        r = subprocess.run(["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--child", f"{n}:{a.nt}",
                            "--iters", str(a.iters)], stdout=subprocess.PIPE, text=True)
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        if r.returncode != 0 or not lines:
            cases.append({"chains": n, "error": f"child exit status {r.returncode}"})
            break   # (nothing more is started on a device that has just failed or hung)
        cases.append(json.loads(lines[-1]))
    with open(a.out, "w") as f:
        f.write(report(cases))
    print(json.dumps({"tool": "bench_mcmc", "cases": cases}))
    sys.exit(0 if all("error" not in c for c in cases) else 1)

import numpy as np   # noqa: E402
import torch   # noqa: E402

sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import kat_cases as K  # noqa: E402

ion = importlib.import_module("neural-ode-ion-channels_amd")
mc = importlib.import_module("neural-ode-ion-channels_amd.mcmc")
obj = importlib.import_module("neural-ode-ion-channels_amd.objective")
capi = ion.capi
dev = torch.device("cuda:0")
chains, Nt = (int(s) for s in a.child.split(":"))
FREE, N, SIGMA_BOUNDS, SCALE = (0, 1, 2, 3), 5, (0.01, 1.0), 0.02
pv = ion.protocols.sinewave(ion.protocols.sinewave_scales(0, 1), n_samples=Nt, dt=0.1, xp=torch, device=dev)
te = torch.arange(Nt, dtype=torch.float64, device=dev) * 0.1
rng = np.random.default_rng(0)
x0 = np.concatenate([K.P_HH[None, :4] * np.exp(0.02 * rng.normal(size=(chains, 4))), np.full((chains, 1), 0.1)], axis=1)
lo, hi = K.P_HH[:4] / 10.0, K.P_HH[:4] * 10.0
y1 = torch.tensor([[0.0, 1.0]], dtype=torch.float64, device=dev)
nom = ion.batched.solve(K.MODEL_HH2, torch.from_numpy(K.P_HH[None]).to(dev), pv, y1, te, prot_t0=0.0, prot_dt=0.1, current=True)
ref = (nom.i + torch.from_numpy(rng.normal(0.0, 0.1, (1, Nt))).to(dev)).contiguous()
pv_h, ref_h, te_h = pv.cpu().numpy(), ref.cpu().numpy(), te.cpu().numpy()


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) * 1e3


res = {"chains": chains, "Nt": Nt, "state": "fp64", "gpu": torch.cuda.get_device_name(dev), "library_sha256": capi.library_digest()}

# ---- the sampler's iteration, its two launches timed apart (adaptation on from the second iteration) ----
desc = mc.mcmc_desc(chains, 1, 8, FREE, K.P_HH, log_parameters=True, lo=lo, hi=hi, sigma_bounds=SIGMA_BOUNDS, n_samples=Nt, max_iter=10 ** 6,
                    adapt_start=2, sample_cap=a.iters + 1, seed=1)
state, flag, iters, trial, samples = (torch.from_numpy(x).to(dev) for x in mc.mcmc_init(x0, desc, SCALE))
y0 = y1.expand(chains, 2).contiguous()
pot = torch.zeros(chains, dtype=torch.int32, device=dev)
best, seen = {"solve_ms": float("inf"), "step_ms": float("inf")}, []
for g in range(a.iters):
    sol, ts = timed(lambda: ion.batched.solve(K.MODEL_HH2, trial, pv, y0, te, prot_t0=0.0, prot_dt=0.1, prot_of_traj=pot, sse_ref=ref, states=False))
    _, tk = timed(lambda: mc.mcmc_step(desc, None, sol.sse, sol.status, state, flag, iters, trial, samples))
    if g > 0:   # (the first iteration pays the allocations)
        best = {k: min(best[k], v) for k, v in zip(best, (ts, tk))}
        seen.append(ts)
res.update(best, solve_mean_ms=sum(seen) / len(seen), running_after=int((flag == 0).sum()), failed_after=int((sol.status != 0).sum()),
           accepted=int(iters[:, 1].sum()))
torch.cuda.empty_cache()

# ---- the driver's own loop, nothing timed inside it ----
common = dict(base_params=K.P_HH, free=FREE, prot_t0=0.0, prot_dt=0.1, state_dtype=torch.float64)
kw = dict(bounds=(lo, hi), sigma_bounds=SIGMA_BOUNDS, scale=SCALE, seed=1, max_iter=a.iters, adapt_start=2, compact_every=None, device=dev)
_, t = timed(lambda: mc.sample(K.MODEL_HH2, x0, pv_h, ref_h, te_h, **common, **kw))
_, t = timed(lambda: mc.sample(K.MODEL_HH2, x0, pv_h, ref_h, te_h, **common, **kw))
res["iteration_ms"] = t / (a.iters + 1)
torch.cuda.empty_cache()

# ---- the loop a caller had before: population_sum_of_squares + a numpy adaptive-Metropolis step per chain on the host ----
ulo, uhi = np.log(np.append(lo, SIGMA_BOUNDS[0])), np.log(np.append(hi, SIGMA_BOUNDS[1]))
hrng = np.random.default_rng(1)
u = np.log(x0)
mu, C, ll, lp = u.copy(), np.tile(np.eye(N) * SCALE ** 2, (chains, 1, 1)), np.zeros(chains), np.full(chains, -np.inf)
prop = u.copy()
t_it, t_eval = float("inf"), float("inf")
for g in range(min(a.iters, 4)):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    S = obj.population_sum_of_squares(np.exp(prop[:, :4]), pv_h, ref_h, te_h, model=K.MODEL_HH2, device=dev, **common).cpu().numpy()
    t1 = time.perf_counter()
    for k in range(chains):
        inside = bool(((prop[k] >= ulo) & (prop[k] <= uhi)).all())
        lp_t = -Nt * prop[k, 4] - 0.5 * S[k] * np.exp(-2.0 * prop[k, 4]) if inside and np.isfinite(S[k]) else -np.inf
        alpha = 1.0 if g == 0 else (np.exp(min(lp_t - lp[k], 0.0)) if np.isfinite(lp_t) else 0.0)
        if g == 0 or (alpha > 0.0 and np.log(hrng.random()) < lp_t - lp[k]):
            u[k], lp[k] = prop[k], lp_t
        if g >= 2:
            gamma = (g - 2 + 2.0) ** -0.6
            mu[k] = mu[k] + gamma * (u[k] - mu[k])
            d = u[k] - mu[k]
            C[k] = C[k] + gamma * (np.outer(d, d) - C[k])
            ll[k] = ll[k] + gamma * (alpha - 0.234)
        Lf = np.linalg.cholesky(np.exp(ll[k]) * (C[k] + 1e-12 * np.eye(N)))
        prop[k] = u[k] + Lf @ hrng.standard_normal(N)
    t2 = time.perf_counter()
    if g > 0:
        t_it, t_eval = min(t_it, (t2 - t0) * 1e3), min(t_eval, (t1 - t0) * 1e3)
res.update(host_iteration_ms=t_it, host_sampler_ms=t_it - t_eval)
print(json.dumps(res))
