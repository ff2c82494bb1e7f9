"""Dev/bench tool (GPU box): one manifold-MALA iteration of K chains (mala.py: sensitivity.gauss_newton's checkpointed forward and
tangent sweep + ionode_mala_step) beside, in the same run, one adaptive-Metropolis iteration (mcmc.py: the fused forward solve +
ionode_mcmc_step); and, on one synthetic noisy data set, the effective sample size per second of the worst coordinate for both
samplers.  Writes profiles/mala_sampling.md and prints one JSON line.  No target is set: the table says what was measured, including
where the new sampler loses.

HH 2-state, p1 .. p4 free in log parameters plus sampled sigma (five coordinates), fp64 state, --nt samples, one sine-wave protocol
with noise of sigma 0.1 on the data, the reference's box p / 10 .. 10 p, K chains = K trajectories an iteration.  Per case, best of the
iterations after the first (ms):
  forward_ms          the checkpointed forward with the fused sum of squares
  sweep_ms            the tangent sweep's J^T r and J^T J
  step_ms             ionode_mala_step (tell + proposal)
  iteration_ms        mala.sample's own loop, per iteration (nothing timed inside it)
  mcmc_solve_ms, mcmc_step_ms, mcmc_iteration_ms   the same for the adaptive-Metropolis sampler
The effective sample size (--ess-chains chains; --ess-iters-mala / --ess-iters-mcmc iterations, both samplers from the same starts):
per coordinate of the search space (log p1 .. log p4, log sigma), the second half of every chain centred on the pooled mean, the
autocovariance averaged over the chains, Geyer's initial positive sequence summed to tau = 1 + 2 sum rho_k, ESS = chains x rows /
tau, divided by the second half's share of the run's wall time.  Twice: every chain started at the Levenberg-Marquardt optimum of the
same data (the documented workflow), and the chains started 1 % around the truth, many posterior standard deviations from the mode.
Every case runs in a child process of its own under `timeout`; a child that fails ends the run.
python tools/bench_mala.py [--chains 8,512,8192] [--nt 20001] [--iters 8] [--ess-chains 64] [--timeout 280] [--out profiles/mala_sampling.md]"""
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
ap.add_argument("--ess-chains", type=int, default=64)
ap.add_argument("--ess-iters-mala", type=int, default=3000)
ap.add_argument("--ess-iters-mcmc", type=int, default=12000)
ap.add_argument("--timeout", type=int, default=280)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mala_sampling.md"))
ap.add_argument("--child", default="")
a = ap.parse_args()
COORDS = ("log p1", "log p2", "log p3", "log p4", "log sigma")


def np_exp(x):
    import math
    return math.exp(x)


def report(cases, ess):
    def row(c):
        if "error" in c:
            return f"| {c['chains']} | {c['error']} |"
        return (f"| {c['chains']:,} | {c['Nt']:,} | {c['forward_ms']:.2f} | {c['sweep_ms']:.2f} | {c['step_ms']:.3f} | {c['iteration_ms']:.2f} | "
                f"{c['mcmc_solve_ms']:.2f} | {c['mcmc_step_ms']:.3f} | {c['mcmc_iteration_ms']:.2f} | {c['iteration_ms'] / c['mcmc_iteration_ms']:.2f} |").replace(",", " ")
    ok = [c for c in cases if "error" not in c]
    head = ok[0] if ok else {}
    lines = [
        "# Batched manifold MALA (`mala.py`, `ionode_mala_step`) beside adaptive Metropolis (`mcmc.py`): iteration time and effective sample size",
        "",
        f"Library sha256 `{head.get('library_sha256', '?')}`, one {head.get('gpu', 'GPU')}; written by `tools/bench_mala.py`.",
        "",
        "HH 2-state, p1 .. p4 free in log parameters plus sampled sigma (five coordinates), fp64 state, one sine-wave protocol, noise of",
        "sigma 0.1 on the data, the box p / 10 .. 10 p, rtol 1e-7 / atol 1e-9, no step cap; one trajectory per chain and iteration.  Best of",
        "the iterations after the first, ms (the samplers' own loops: a mean per iteration); every case in a process of its own, both samplers",
        "in the same process.  A manifold-MALA iteration is the checkpointed forward, the tangent sweep and the step; an adaptive-Metropolis",
        "iteration is the plain fused forward and its step.",
        "",
        "| chains | samples | forward (checkpointed) | tangent sweep | `ionode_mala_step` | `mala.sample` per iteration | AM fused solve | `ionode_mcmc_step` | `mcmc.sample` per iteration | MALA / AM iteration |",
        "|---:|---:|---:|---:|---:|---:|---:|---:|---:|---:|",
        *[row(c) for c in cases],
        "",
    ]
    if ess:
        lines += [
            "## Effective sample size per second",
            "",
            "One data set and the same starts for both samplers; the second half of each run; per coordinate (the search space: log p1 .. log p4,",
            "log sigma) the chains centred on the pooled mean, the autocovariance averaged over the chains, Geyer's initial positive sequence;",
            "seconds are the second half's share of the run's wall time.  Chains that have not met (R-hat far from 1) show as a small pooled",
            "ESS: the pooled centring counts their distance as correlation.  Nobody had measured these numbers before; no target is set.",
            "",
        ]
    for e in ess:
        if "error" in e:
            lines += [f"Start `{e['start']}`: {e['error']}", ""]
            continue
        m, c = e["mala"], e["mcmc"]
        where = (f"every chain at the Levenberg-Marquardt optimum of the same data (`fit.levenberg_marquardt` from the truth, {e.get('fit_evaluations', '?')} "
                 f"evaluations), sigma at sqrt(S / N) = {e.get('fit_sigma', float('nan')):.4f}" if e["start"] == "optimum" else
                 "the parameters 1 % (log-normal) around the truth, sigma at 0.1: many posterior standard deviations from the mode")
        lines += [
            f"### {e['chains']} chains x {e['Nt']} samples; start: {where}",
            "",
            "| sampler | iterations | acceptance (second half) | ms per iteration | R-hat, worst | ESS per coordinate (log p1 .. log p4, log sigma) | worst coordinate | its ESS per second |",
            "|---|---:|---:|---:|---:|---|---|---:|",
            *[f"| {name} | {r['iters']} | {r['accept_second_half']:.3f} | {r['ms_per_iter']:.2f} | {r['rhat_worst']:.4f} | "
              f"{', '.join('%.0f' % e for e in r['ess'])} | {COORDS[r['worst']]} | {r['ess_per_s']:.2f} |"
              for name, r in (("manifold MALA", m), ("adaptive Metropolis", c))],
            "",
            f"Step size eps of the manifold MALA chains after the run: median {np_exp(m['log_scale_median']):.3f}, range {np_exp(m['log_scale_range'][0]):.3f} .. "
            f"{np_exp(m['log_scale_range'][1]):.3f} (1 is the Langevin step of a Gaussian target in its own metric).",
            f"Posterior standard deviations of the pooled second halves, manifold MALA: {', '.join('%.2e' % v for v in m['sd'])}; adaptive Metropolis: "
            f"{', '.join('%.2e' % v for v in c['sd'])}.",
            f"Ratio of the worst coordinates' ESS per second, manifold MALA over adaptive Metropolis: {m['ess_per_s'] / c['ess_per_s']:.2f}.",
            "",
        ]
    return "\n".join(lines)


def child(arg, extra):
    r = subprocess.run(["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--child", arg, "--iters", str(a.iters),
                        "--ess-iters-mala", str(a.ess_iters_mala), "--ess-iters-mcmc", str(a.ess_iters_mcmc)], stdout=subprocess.PIPE, text=True)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    if r.returncode != 0 or not lines:
        return dict(extra, error=f"child exit status {r.returncode}")
    return json.loads(lines[-1])


if not a.child:   # the parent never opens the GPU
    cases, ess = [], []
    for n in [int(s) for s in a.chains.split(",")]:
        cases.append(child(f"split:{n}:{a.nt}", {"chains": n}))
        if "error" in cases[-1]:
            break   # (nothing more is started on a device that has just failed or hung)
    if a.ess_chains > 0 and all("error" not in c for c in cases):
        for start in ("optimum", "spread"):
            ess.append(child(f"ess:{a.ess_chains}:{a.nt}:{start}", {"chains": a.ess_chains, "start": start}))
            if "error" in ess[-1]:
                break
    with open(a.out, "w") as f:
        f.write(report(cases, ess))
    print(json.dumps({"tool": "bench_mala", "cases": cases, "ess": ess}))
    sys.exit(0 if all("error" not in c for c in cases + ess) else 1)

import numpy as np   # noqa: E402
import torch   # noqa: E402

sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import kat_cases as K  # noqa: E402

ion = importlib.import_module("neural-ode-ion-channels_amd")
ma = importlib.import_module("neural-ode-ion-channels_amd.mala")
mc = importlib.import_module("neural-ode-ion-channels_amd.mcmc")
sens = importlib.import_module("neural-ode-ion-channels_amd.sensitivity")
capi = ion.capi
dev = torch.device("cuda:0")
mode, chains, Nt = a.child.split(":")[:3]
chains, Nt = int(chains), int(Nt)
start = (a.child.split(":") + ["optimum"])[3]
FREE, N, SIGMA_BOUNDS, SCALE = (0, 1, 2, 3), 5, (0.01, 1.0), 0.02
pv = ion.protocols.sinewave(ion.protocols.sinewave_scales(0, 1), n_samples=Nt, dt=0.1, xp=torch, device=dev)
te = torch.arange(Nt, dtype=torch.float64, device=dev) * 0.1
rng = np.random.default_rng(0)
spread = 0.02 if mode == "split" else 0.01
x0 = np.concatenate([K.P_HH[None, :4] * np.exp(spread * rng.normal(size=(chains, 4))), np.full((chains, 1), 0.1)], axis=1)
lo, hi = K.P_HH[:4] / 10.0, K.P_HH[:4] * 10.0
y1 = torch.tensor([[0.0, 1.0]], dtype=torch.float64, device=dev)
nom = ion.batched.solve(K.MODEL_HH2, torch.from_numpy(K.P_HH[None]).to(dev), pv, y1, te, prot_t0=0.0, prot_dt=0.1, current=True)
ref = (nom.i + torch.from_numpy(rng.normal(0.0, 0.1, (1, Nt))).to(dev)).contiguous()
pv_h, ref_h, te_h = pv.cpu().numpy(), ref.cpu().numpy(), te.cpu().numpy()
common = dict(base_params=K.P_HH, free=FREE, prot_t0=0.0, prot_dt=0.1, state_dtype=torch.float64, bounds=(lo, hi), sigma_bounds=SIGMA_BOUNDS, device=dev)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) * 1e3


res = {"chains": chains, "Nt": Nt, "state": "fp64", "gpu": torch.cuda.get_device_name(dev), "library_sha256": capi.library_digest()}

if mode == "split":
    y0 = y1.expand(chains, 2).contiguous()
    pot = torch.zeros(chains, dtype=torch.int32, device=dev)
    # ---- manifold MALA: its three launches timed apart ----
    desc = ma.mala_desc(chains, 1, 8, FREE, K.P_HH, log_parameters=True, lo=lo, hi=hi, sigma_bounds=SIGMA_BOUNDS, n_samples=Nt, max_iter=10 ** 6,
                        sample_cap=a.iters + 1, seed=1)
    state, flag, iters, trial, samples = (torch.from_numpy(x).to(dev) for x in ma.mala_init(x0, desc, 1.0))
    full = dict(prot_t=None, prot_t0=0.0, prot_dt=0.1, prot_of_traj=pot, rtol=1e-7, atol=1e-9, v_oob=-80.0, max_steps=0, max_total_steps=1_000_000,
                max_step=0.0, obs_g=1.0, obs_e=-86.0, obs_open_state_only=False, ckpt_cap=None, ckpt_budget_bytes=None)
    hint = ion.grad.uniform_grid_hint(te)
    jtr = torch.empty((chains, 8), dtype=torch.float64, device=dev)
    jtj = torch.empty((chains, 8, 8), dtype=torch.float64, device=dev)
    best = {"forward_ms": float("inf"), "sweep_ms": float("inf"), "step_ms": float("inf")}
    for g in range(a.iters):
        (r, cfg, p, ckpt, n_acc), tf = timed(lambda: sens._forward(K.MODEL_HH2, trial, pv, y0, te, full, sse_ref=ref, objective="sse", t_eval_hint=hint))
        _, ts = timed(lambda: sens._sweep(r, cfg, p, ckpt, n_acc, None, jtr, jtj))
        _, tk = timed(lambda: ma.mala_step(desc, None, r["sse"], jtr, jtj, r["status"].to(torch.int32), state, flag, iters, trial, samples))
        if g > 0:   # (the first iteration pays the allocations)
            best = {k: min(best[k], v) for k, v in zip(best, (tf, ts, tk))}
        del r, cfg, p, ckpt, n_acc
    res.update(best, running_after=int((flag == 0).sum()), accepted=int(iters[:, 1].sum()))
    del state, flag, iters, trial, samples, jtr, jtj
    torch.cuda.empty_cache()
    kw = dict(seed=1, max_iter=a.iters, compact_every=None)
    _, t = timed(lambda: ma.sample(K.MODEL_HH2, x0, pv_h, ref_h, te_h, **common, **kw))
    _, t = timed(lambda: ma.sample(K.MODEL_HH2, x0, pv_h, ref_h, te_h, **common, **kw))
    res["iteration_ms"] = t / (a.iters + 1)
    torch.cuda.empty_cache()
    # ---- adaptive Metropolis, in the same process ----
    desc = mc.mcmc_desc(chains, 1, 8, FREE, K.P_HH, log_parameters=True, lo=lo, hi=hi, sigma_bounds=SIGMA_BOUNDS, n_samples=Nt, max_iter=10 ** 6,
                        adapt_start=2, sample_cap=a.iters + 1, seed=1)
    state, flag, iters, trial, samples = (torch.from_numpy(x).to(dev) for x in mc.mcmc_init(x0, desc, SCALE))
    best = {"mcmc_solve_ms": float("inf"), "mcmc_step_ms": float("inf")}
    for g in range(a.iters):
        sol, ts = timed(lambda: ion.batched.solve(K.MODEL_HH2, trial, pv, y0, te, prot_t0=0.0, prot_dt=0.1, prot_of_traj=pot, sse_ref=ref, states=False))
        _, tk = timed(lambda: mc.mcmc_step(desc, None, sol.sse, sol.status, state, flag, iters, trial, samples))
        if g > 0:
            best = {k: min(best[k], v) for k, v in zip(best, (ts, tk))}
    res.update(best)
    torch.cuda.empty_cache()
    kw = dict(scale=SCALE, seed=1, max_iter=a.iters, adapt_start=2, compact_every=None)
    _, t = timed(lambda: mc.sample(K.MODEL_HH2, x0, pv_h, ref_h, te_h, **common, **kw))
    _, t = timed(lambda: mc.sample(K.MODEL_HH2, x0, pv_h, ref_h, te_h, **common, **kw))
    res["mcmc_iteration_ms"] = t / (a.iters + 1)
    print(json.dumps(res))
    sys.exit(0)


def ess_of(u):
    """[n]: u [K, R, n] -> K R / tau per coordinate, tau from the chain-averaged autocovariance by Geyer's initial positive sequence."""
    Kc, R, n = u.shape
    d = u - u.reshape(-1, n).mean(axis=0)
    out = np.zeros(n)
    for j in range(n):
        f = np.fft.rfft(d[:, :, j], n=2 * R, axis=1)
        acov = np.fft.irfft(f * np.conj(f), n=2 * R, axis=1)[:, :R].mean(axis=0) / np.arange(R, 0, -1)
        rho = acov / acov[0]
        tau, k = 1.0, 1
        while k + 1 < R:
            pair = rho[k] + rho[k + 1]
            if pair <= 0.0:
                break
            tau += 2.0 * pair
            k += 2
        out[j] = Kc * R / tau
    return out


def run(sampler, iters, **kw):
    last = {}   # (the live state tensor: read once, after the run)
    (smp, rate, flag, its), t = timed(lambda: sampler.sample(K.MODEL_HH2, x0, pv_h, ref_h, te_h, seed=1, max_iter=iters, compact_every=None,
                                                             callback=lambda it, st, fl, i: last.update(state=st), **common, **kw))
    s = smp.cpu().numpy()
    assert (flag.cpu().numpy() == 1).all() and np.isfinite(s).all()
    u = np.log(s[:, iters // 2 + 1:, :N])
    e = ess_of(u)
    moved = (s[:, iters // 2 + 1:, :N] != s[:, iters // 2:-1, :N]).any(axis=2).mean()
    worst = int(np.argmin(e))
    scale = last["state"][:, 1].cpu().numpy()   # log_eps (MALA_STATE_LOG_EPS) or log_lambda (MCMC_STATE_LOG_LAMBDA): word 1 of either state
    return dict(log_scale_median=float(np.median(scale)), log_scale_range=[float(scale.min()), float(scale.max())], iters=iters, ms_per_iter=t / (iters + 1), ess=e.tolist(), worst=worst, ess_per_s=float(e[worst] / (0.5 * t * 1e-3)),
                accept_second_half=float(moved), rhat_worst=float(np.max(mc.rhat(smp, flag))), mean=u.reshape(-1, N).mean(axis=0).tolist(),
                sd=u.reshape(-1, N).std(axis=0).tolist())


res["start"] = start
if start == "optimum":   # the documented workflow: the chains start where the Levenberg-Marquardt fit of the same data ends
    fit = importlib.import_module("neural-ode-ion-channels_amd.fit")
    xf, sf, ff, itf = fit.levenberg_marquardt(K.MODEL_HH2, K.P_HH[None, :4], pv_h, ref_h, te_h, base_params=K.P_HH, free=FREE, bounds=(lo, hi), prot_t0=0.0,
                                              prot_dt=0.1, state_dtype=torch.float64, device=dev, max_iter=50)
    x0 = np.tile(np.append(xf[0].cpu().numpy(), np.sqrt(float(sf[0]) / Nt)), (chains, 1))
    res.update(fit_flag=int(ff[0]), fit_evaluations=int(itf[0, 0]), fit_sigma=float(x0[0, 4]))
res["mala"] = run(ma, a.ess_iters_mala)
torch.cuda.empty_cache()
res["mcmc"] = run(mc, a.ess_iters_mcmc, scale=SCALE)
print(json.dumps(res))
