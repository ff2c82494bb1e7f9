"""Dev/bench tool (GPU box): one CMA-ES generation of K runs (cmaes.py: the fused forward solve + ionode_cmaes_step) beside the loop
a caller had before -- objective.population_sum_of_squares on the whole generation, one device-to-host read, and a numpy CMA-ES per
run on the host (tests/cmaes_cases.py's statement of the algorithm: its tell with numpy.linalg.eigh; the sampling vectorised with
numpy's own generator, as a user would write it).  Writes profiles/cmaes_fit.md and prints one JSON line.

HH 2-state, p1 .. p4 free in log parameters, fp64 state, --nt samples, one sine-wave protocol, the reference's box p / 10 .. 10 p,
lambda = 8 (the default at n = 4), K runs = 8 K trajectories a generation; and one NN-d leg (the shipped s2 net, 5 x 200) at --nn-nt
samples.  Per case, best of the generations after the first (ms):
  solve_ms            the fused forward solve of the generation (solve_mean_ms: its mean -- the generations' points differ, and with
                      them the solves' step counts)
  step_ms             ionode_cmaes_step (tell + ask)
  generation_ms       cmaes.minimise's own loop, per generation (nothing timed inside it)
  host_generation_ms  the host loop's generation; host_optimiser_ms = that minus the evaluation inside it
Every case runs in a child process of its own under `timeout`; a child that fails ends the run.
python tools/bench_cmaes.py [--runs 8,512,8192] [--nt 20001] [--nn-nt 2001] [--gens 6] [--timeout 280] [--out profiles/cmaes_fit.md]"""
import argparse
import importlib
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--runs", default="8,512,8192")
ap.add_argument("--nt", type=int, default=20001)
ap.add_argument("--nn-nt", type=int, default=2001)
ap.add_argument("--gens", type=int, default=6)
ap.add_argument("--timeout", type=int, default=280)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cmaes_fit.md"))
ap.add_argument("--child", default="")
a = ap.parse_args()


def report(cases):
    def row(c):
        if "error" in c:
            return f"| {c['model']} | {c['runs']} | {c['error']} |"
        return (f"| {c['model']} | {c['runs']:,} | {c['trajectories']:,} | {c['Nt']:,} | {c['solve_ms']:.2f} | {c['solve_mean_ms']:.2f} | {c['step_ms']:.3f} | {c['generation_ms']:.2f} | "
                f"{c['host_generation_ms']:.2f} | {c['host_optimiser_ms']:.2f} |").replace(",", " ")
    ok = [c for c in cases if "error" not in c]
    head = ok[0] if ok else {}
    return "\n".join([
        "# Batched CMA-ES (`cmaes.py`, `ionode_cmaes_step`): the per-generation split",
        "",
        f"Library sha256 `{head.get('library_sha256', '?')[:16]}…`, one {head.get('gpu', 'GPU')}; written by `tools/bench_cmaes.py`.",
        "",
        "HH 2-state, p1 .. p4 free in log parameters, fp64 state, one sine-wave protocol, the box p / 10 .. 10 p, lambda = 8, rtol 1e-7 /",
        "atol 1e-9, no step cap; the NN-d leg is the shipped s2 net (5 x 200) with the same free parameters.  Best of the generations after",
        "the first (and the solve's mean over them: `cmaes.minimise` per generation is a mean too), ms; every case in a process of its own.  The host loop is `objective.population_sum_of_squares` on the generation, one",
        "device-to-host read, and a numpy CMA-ES per run (`tests/cmaes_cases.py`: `tell` with `numpy.linalg.eigh`, vectorised sampling).",
        "",
        "| model | runs | trajectories | samples | fused solve, best | mean | `ionode_cmaes_step` | `cmaes.minimise` per generation | host loop per generation | of which the numpy optimiser and the read |",
        "|---|---:|---:|---:|---:|---:|---:|---:|---:|---:|",
        *[row(c) for c in cases],
        "",
        "Nobody had measured these numbers before this table; it sets no target.  The step is one 64-lane workgroup per run",
        "(`csrc/ionode_cmaes.hpp`): no scratch, static LDS 5 856 bytes at four variables, 17 632 at twelve (`tests/test_cmaes_kernel_resources.py`).",
        ""])


if not a.child:   # the parent never opens the GPU
    legs = [("hh", int(s), a.nt) for s in a.runs.split(",")] + [("nnd", 8, a.nn_nt)]
    cases = []
    for model, n, nt in legs:
        r = subprocess.run(["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--child", f"{model}:{n}:{nt}",
                            "--gens", str(a.gens)], stdout=subprocess.PIPE, text=True)
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        if r.returncode != 0 or not lines:
            cases.append({"model": model, "runs": n, "error": f"child exit status {r.returncode}"})
            break   # (nothing more is started on a device that has just failed or hung)
        cases.append(json.loads(lines[-1]))
    with open(a.out, "w") as f:
        f.write(report(cases))
    print(json.dumps({"tool": "bench_cmaes", "cases": cases}))
    sys.exit(0 if all("error" not in c for c in cases) else 1)

import numpy as np   # noqa: E402
import torch   # noqa: E402

sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import cmaes_cases as L  # noqa: E402
import kat_cases as K  # noqa: E402

ion = importlib.import_module("neural-ode-ion-channels_amd")
cm = importlib.import_module("neural-ode-ion-channels_amd.cmaes")
obj = importlib.import_module("neural-ode-ion-channels_amd.objective")
capi = ion.capi
dev = torch.device("cuda:0")
name, runs, Nt = a.child.split(":")
runs, Nt, FREE, LAM = int(runs), int(Nt), (0, 1, 2, 3), 8
MODEL = K.MODEL_HH2 if name == "hh" else K.MODEL_NND
mlp = {} if name == "hh" else dict(weights=K.load_weights("s2"), mlp_layers=K.MLP_L, mlp_width=K.MLP_N, weights_key="s2")
pv = ion.protocols.sinewave(ion.protocols.sinewave_scales(0, 1), n_samples=Nt, dt=0.1, xp=torch, device=dev)
te = torch.arange(Nt, dtype=torch.float64, device=dev) * 0.1
rng = np.random.default_rng(0)
x0 = K.P_HH[None, :4] * np.exp(0.1 * rng.normal(size=(runs, 4)))
lo, hi = K.P_HH[:4] / 10.0, K.P_HH[:4] * 10.0
y1 = torch.tensor([[0.0, 1.0]], dtype=torch.float64, device=dev)
nom = ion.batched.solve(MODEL, torch.from_numpy(K.P_HH[None]).to(dev), pv, y1, te, prot_t0=0.0, prot_dt=0.1, current=True, **mlp)
ref = (nom.i + torch.from_numpy(rng.normal(0.0, 0.1, (1, Nt))).to(dev)).contiguous()
pv_h, ref_h, te_h = pv.cpu().numpy(), ref.cpu().numpy(), te.cpu().numpy()


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) * 1e3


res = {"model": name, "runs": runs, "lambda": LAM, "trajectories": runs * LAM, "Nt": Nt, "state": "fp64", "gpu": torch.cuda.get_device_name(dev),
       "library_sha256": capi.library_digest()}
NEVER = dict(max_iter=10 ** 6, unchanged_iters=10 ** 6, unchanged_threshold=0.0, tolx=0.0)   # (nobody stops inside the timed generations)

# ---- the fit's generation, its two launches timed apart ----
desc = cm.cmaes_desc(runs, LAM, 1, 8, FREE, K.P_HH, log_parameters=True, lo=lo, hi=hi, seed=1, **NEVER)
state, flag, iters, trial = (torch.from_numpy(x).to(dev) for x in cm.cmaes_init(x0, desc))
rows = runs * LAM
y0 = y1.expand(rows, 2).contiguous()
pot = torch.zeros(rows, dtype=torch.int32, device=dev)
value, status = torch.zeros(rows, dtype=torch.float64, device=dev), torch.zeros(rows, dtype=torch.int32, device=dev)
cm.cmaes_step(desc, None, value, status, state, flag, iters, trial)
best, seen = {"solve_ms": float("inf"), "step_ms": float("inf")}, []
for g in range(a.gens):
    sol, ts = timed(lambda: ion.batched.solve(MODEL, trial, pv, y0, te, prot_t0=0.0, prot_dt=0.1, prot_of_traj=pot, sse_ref=ref, states=False, **mlp))
    _, tk = timed(lambda: cm.cmaes_step(desc, None, sol.sse, sol.status, state, flag, iters, trial))
    if g > 0:   # (the first generation pays the allocations)
        best = {k: min(best[k], v) for k, v in zip(best, (ts, tk))}
        seen.append(ts)
res.update(best, solve_mean_ms=sum(seen) / len(seen), running_after=int((flag == 0).sum()), failed_after=int((sol.status != 0).sum()))
torch.cuda.empty_cache()

# ---- the driver's own loop, nothing timed inside it ----
common = dict(base_params=K.P_HH, free=FREE, prot_t0=0.0, prot_dt=0.1, state_dtype=torch.float64)
kw = dict(NEVER, max_iter=a.gens)
_, t = timed(lambda: cm.minimise(MODEL, x0, pv_h, ref_h, te_h, bounds=(lo, hi), popsize=LAM, seed=1, compact_every=None, device=dev, **common, **mlp, **kw))
_, t = timed(lambda: cm.minimise(MODEL, x0, pv_h, ref_h, te_h, bounds=(lo, hi), popsize=LAM, seed=1, compact_every=None, device=dev, **common, **mlp, **kw))
res["generation_ms"] = t / a.gens
torch.cuda.empty_cache()

# ---- the loop a caller had before: population_sum_of_squares + a numpy CMA-ES per run on the host ----
c = L.constants(4, LAM)
ulo, uhi = np.log(lo), np.log(hi)
sts = [dict(m=np.log(x0[k]), sigma=0.1, pc=np.zeros(4), ps=np.zeros(4), C=np.eye(4)) for k in range(runs)]
BD = [(np.eye(4), np.ones(4)) for _ in range(runs)]
hrng = np.random.default_rng(1)
t_gen, t_eval = float("inf"), float("inf")
for g in range(min(a.gens, 3)):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    z = hrng.standard_normal((runs, LAM, 4))
    pop = np.stack([np.clip(sts[k]["m"][None] + sts[k]["sigma"] * (z[k] * BD[k][1][None]) @ BD[k][0].T, ulo, uhi) for k in range(runs)])
    t1 = time.perf_counter()
    f = obj.population_sum_of_squares(np.exp(pop.reshape(-1, 4)), pv_h, ref_h, te_h, model=MODEL, device=dev, **common, **mlp).cpu().numpy().reshape(runs, LAM)
    t2 = time.perf_counter()
    for k in range(runs):
        new = L.tell(sts[k], pop[k], f[k], c, g + 1)
        if new is not None:
            sts[k] = new
            ev, B = np.linalg.eigh(new["C"])
            BD[k] = (B, np.sqrt(np.maximum(ev, 0.0)))
    t3 = time.perf_counter()
    if g > 0:
        t_gen, t_eval = min(t_gen, (t3 - t0) * 1e3), min(t_eval, (t2 - t1) * 1e3)
res.update(host_generation_ms=t_gen, host_optimiser_ms=t_gen - t_eval)
print(json.dumps(res))
