"""Dev/bench tool (GPU box): one CMA-ES generation of K multi-exponential fits (expfit.py: ionode_multi_exp_objective +
ionode_cmaes_step) beside the routes a user had before on the host -- preprocess.fit_multi_exp (the restarted simplex) per segment, and
the numpy statement of the same CMA-ES (tests/cmaes_cases.py: reference_run) per run.  Writes profiles/expfit.md and prints one JSON line.

Tri-exponential segments of --nt samples at 0.5 ms (recovery case 0's curve, noise 0.01, one seed per segment), start TRI_EXP_X0_SLOW,
restarts 3: K runs = K / 4 segments, lambda = 9 (the default at n = 7), 9 K rows a generation.  Per case (ms unless stated):
  objective_ms        ionode_multi_exp_objective on the generation's rows (best of the generations after the first; mean beside it)
  step_ms             ionode_cmaes_step (tell + ask), the same way
  generation_ms       expfit.fit_runs's own loop, per generation (nothing timed inside it, no compaction): the difference of a
                      5 x --loop-gens and a --loop-gens fit, best of two each
  fit_s               expfit.fit_segments as a user calls it: max_iter = --fit-gens, the default stopping rule, compact_every = 4;
                      wall seconds of the second call, with the worst segment's RMSE over the noise and the mean generations told
  simplex_s_segment   preprocess.fit_multi_exp(restarts = 3) per segment, measured on --host-segments segments
  numpy_ms_generation cmaes_cases.reference_run per run and generation, measured on one run of --host-gens generations
Every case runs in a child process of its own under `timeout`; a child that fails ends the run.
python tools/bench_expfit.py [--runs 8,512,8192] [--nt 2000] [--gens 12] [--loop-gens 100] [--fit-gens 1000] [--timeout 280] [--out profiles/expfit.md]"""
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
ap.add_argument("--nt", type=int, default=2000)
ap.add_argument("--gens", type=int, default=12)
ap.add_argument("--loop-gens", type=int, default=100)
ap.add_argument("--fit-gens", type=int, default=1000)
ap.add_argument("--host-segments", type=int, default=2)
ap.add_argument("--host-gens", type=int, default=20)
ap.add_argument("--timeout", type=int, default=280)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "expfit.md"))
ap.add_argument("--child", default="")
a = ap.parse_args()
RESTARTS, LAM = 3, 9


def report(cases, regs):
    def row(c):
        if "error" in c:
            return f"| {c['runs']} | {c['error']} |"
        return (f"| {c['runs']:,} | {c['segments']:,} | {c['rows']:,} | {c['objective_ms']:.3f} | {c['objective_mean_ms']:.3f} | {c['step_ms']:.3f} | "
                f"{c['generation_ms']:.3f} | {c['fit_s']:.3f} | {c['fit_generations_mean']:.0f} | {c['fit_rmse_over_noise_worst']:.4f} | {c['simplex_s_segment']:.3f} | {c['simplex_s_segment'] * c['segments']:.1f} | "
                f"{c['simplex_rmse_over_noise_worst']:.4f} | {c['numpy_ms_generation']:.2f} | {c['numpy_ms_generation'] * c['runs']:.0f} |").replace(",", " ")
    ok = [c for c in cases if "error" not in c]
    head = ok[0] if ok else {}
    return "\n".join([
        "# Batched multi-exponential fits (`expfit.py`, `ionode_multi_exp_objective`): the per-generation split",
        "",
        f"Library sha256 `{head.get('library_sha256', '?')[:16]}…`, one {head.get('gpu', 'GPU')}; written by `tools/bench_expfit.py`.",
        "",
        f"Tri-exponential segments of {head.get('Nt', '?')} samples at 0.5 ms, start `TRI_EXP_X0_SLOW`, restarts 3 (four runs a segment), lambda = 9.",
        "Kernel times: best of the generations after the first (and the objective's mean), ms, a host clock around a device synchronise.",
        f"`fit_runs` per generation is its own loop, nothing timed inside it: a {5 * head.get('loop_gens', 0)}-generation fit minus a {head.get('loop_gens', '?')}-generation one, best of two each.  The whole",
        f"fit is `fit_segments` as a user calls it (`max_iter = {head.get('fit_gens', '?')}`, the default stopping rule, `compact_every = 4`), wall seconds of the second",
        "call, with the mean generations a run was told and the worst segment's RMSE over the noise (0.01).  The host routes are timed in the same process: the restarted",
        "simplex on a few segments (seconds per segment; the whole-protocol column is that times the segments, an extrapolation), the numpy",
        "CMA-ES on one run (ms per run and generation; the column beside it is that times the runs, an extrapolation).",
        "",
        "| runs | segments | rows | objective kernel, best | mean | `ionode_cmaes_step` | `fit_runs` per generation | whole fit, s | generations, mean | worst RMSE / noise | simplex, s per segment | x segments, s | worst RMSE / noise | numpy CMA-ES, ms per run and generation | x runs, ms |",
        "|---:|---:|---:|---:|---:|---:|---:|---:|---:|---:|---:|---:|---:|---:|---:|",
        *[row(c) for c in cases],
        "",
        "Registers of the new kernels (VGPR / SGPR / scratch bytes / static LDS bytes): "
        + "; ".join(f"`{r['kernel'].split('ionode::')[1].split('(')[0]}` {r['vgpr']} / {r['sgpr']} / {r['scratch_bytes']} / {r['lds_static']}" for r in regs) + ".",
        "",
        "Nobody had measured these numbers before this table; it sets no target.",
        ""])


if not a.child:   # the parent never opens the GPU
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernel_resources import kernel_resources
    regs = [r for r in kernel_resources(os.path.join(ROOT, "neural-ode-ion-channels_amd", "libionode.so")) if "multi_exp" in r["kernel"]]
    cases = []
    for n in (int(s) for s in a.runs.split(",")):
        r = subprocess.run(["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--child", str(n), "--nt", str(a.nt),
                            "--gens", str(a.gens), "--loop-gens", str(a.loop_gens), "--fit-gens", str(a.fit_gens), "--host-segments", str(a.host_segments), "--host-gens",
                            str(a.host_gens)], stdout=subprocess.PIPE, text=True)
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        if r.returncode != 0 or not lines:
            cases.append({"runs": n, "error": f"child exit status {r.returncode}"})
            break   # (nothing more is started on a device that has just failed or hung)
        cases.append(json.loads(lines[-1]))
    with open(a.out, "w") as f:
        f.write(report(cases, regs))
    print(json.dumps({"tool": "bench_expfit", "cases": cases, "registers": regs}))
    sys.exit(0 if all("error" not in c for c in cases) else 1)

import numpy as np   # noqa: E402
import torch   # noqa: E402

sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import cmaes_cases as L  # noqa: E402
import expfit_cases as E  # noqa: E402

ion, ef, pp = E.mods()
cm = importlib.import_module("neural-ode-ion-channels_amd.cmaes")
capi = ion.capi
dev = torch.device("cuda:0")
runs, Nt = int(a.child), a.nt
S, R, n = max(runs // (RESTARTS + 1), 1), RESTARTS + 1, 7
K = S * R
x0 = np.array(pp.TRI_EXP_X0_SLOW)
truth = np.array(E.RECOVERY[0][0])
t = np.arange(Nt) * 0.5
clean = pp.multi_exp(t, truth)
t_list = [t] * S
a_list = [clean + np.random.default_rng(g).normal(0.0, 0.01, Nt) for g in range(S)]
rng = np.random.default_rng(0)
per_segment = np.stack([x0] + [x0 * np.exp(rng.normal(0.0, 0.5, n)) for _ in range(RESTARTS)])
starts, seg = np.tile(per_segment, (S, 1)), np.repeat(np.arange(S, dtype=np.int32), R)
scale = np.abs(x0)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) * 1e3


res = {"runs": K, "segments": S, "lambda": LAM, "rows": K * LAM, "Nt": Nt, "gens": a.gens, "loop_gens": a.loop_gens, "fit_gens": a.fit_gens,
       "gpu": torch.cuda.get_device_name(dev), "library_sha256": capi.library_digest()}
NEVER = dict(max_iter=10 ** 6, unchanged_iters=10 ** 6, unchanged_threshold=0.0, tolx=0.0)   # (nobody stops inside the timed generations)

# ---- the fit's generation, its two launches timed apart ----
desc = cm.cmaes_desc(K, LAM, 1, n, list(range(n)), np.zeros(n), log_parameters=False, lo=None, hi=None, seed=0, **NEVER)
state, flag, iters, trial = (torch.from_numpy(x).to(dev) for x in cm.cmaes_init(starts, desc, 1.0 / 6.0, scale))
off = torch.from_numpy(np.arange(S + 1, dtype=np.int64) * Nt).to(dev)
seg_d = torch.from_numpy(seg).to(dev)
tt, aa = torch.from_numpy(np.concatenate(t_list)).to(dev), torch.from_numpy(np.concatenate(a_list)).to(dev)
value, status = torch.zeros(K * LAM, dtype=torch.float64, device=dev), torch.zeros(K * LAM, dtype=torch.int32, device=dev)
cm.cmaes_step(desc, None, value, status, state, flag, iters, trial)
best, seen = {"objective_ms": float("inf"), "step_ms": float("inf")}, []
for g in range(a.gens):
    _, to = timed(lambda: ef.objective(K, LAM, n, None, seg_d, off, tt, aa, trial, value, status))
    _, tk = timed(lambda: cm.cmaes_step(desc, None, value, status, state, flag, iters, trial))
    if g > 0:   # (the first generation pays the code objects' load)
        best = {k: min(best[k], v) for k, v in zip(best, (to, tk))}
        seen.append(to)
res.update(best, objective_mean_ms=sum(seen) / len(seen), running_after=int((flag == 0).sum()))

# ---- the driver's own loops, nothing timed inside them ----
kw = dict(NEVER, scale=scale, seed=0, compact_every=None, device=dev)


def loop_s(gens):   # best of two
    out = []
    for _ in range(2):
        t0 = time.perf_counter()
        ef.fit_runs(t_list, a_list, seg, starts, **dict(kw, max_iter=gens))
        out.append(time.perf_counter() - t0)
    return min(out)


ef.fit_runs(t_list, a_list, seg, starts, **dict(kw, max_iter=4))
short, long_ = a.loop_gens, 5 * a.loop_gens
res["generation_ms"] = (loop_s(long_) - loop_s(short)) * 1e3 / (long_ - short)   # (the difference of two lengths: uploads and the final read cancel)
for _ in range(2):   # (the second call: the first pays torch's own first launches)
    t0 = time.perf_counter()
    x, f, fl, it = ef.fit_segments(t_list, a_list, x0, restarts=RESTARTS, max_iter=a.fit_gens, device=dev)
    res["fit_s"] = time.perf_counter() - t0
res.update(fit_rmse_over_noise_worst=float(f.max() / 0.01), fit_flags=np.bincount(fl.reshape(-1), minlength=6).tolist(),
           fit_generations_mean=float(it[:, :, 0].mean()))

# ---- the routes a user had before, on the host ----
t0 = time.perf_counter()
worst = 0.0
for g in range(min(a.host_segments, S)):
    xs = pp.fit_multi_exp(t_list[g], a_list[g], x0, restarts=RESTARTS)
    worst = max(worst, E.rmse(t_list[g], a_list[g], xs) / 0.01)
res.update(simplex_s_segment=(time.perf_counter() - t0) / min(a.host_segments, S), simplex_rmse_over_noise_worst=worst)
fn = lambda u: np.sqrt(np.mean((pp.multi_exp(t_list[0], u * scale) - a_list[0]) ** 2))   # (the search variable carries the scale |x0|)
t0 = time.perf_counter()
gens, _ = L.reference_run(fn, x0 / scale, lam=LAM, sigma0=1.0 / 6.0, seed=0, run=0, target=-np.inf, max_gen=a.host_gens)
res["numpy_ms_generation"] = (time.perf_counter() - t0) * 1e3 / max(gens, 1)
print(json.dumps(res))
