"""Dev/bench tool (GPU box): posterior predictive bands of S parameter draws (predictive.bands: chunked fused solves,
ionode_predictive_accumulate, one ionode_predictive_quantiles) beside the route a user had before -- batched.solve(current=True) of all
draws at once, the whole trace [S, Nt] kept, torch.mean / std / amin / amax over the draws and torch.quantile on slices of time that
stay below its 16 M-element limit.  Writes profiles/predictive.md and prints one JSON line.

HH 2-state, fp64 state, --nt samples of one sine-wave protocol, S draws of p1 .. p4 (2 % log-normal around the ground truth), the
quantiles 0.025 / 0.5 / 0.975, no noise (the old route has none).  The two routes alternate, --rounds times; per case, best of the
rounds (ms) and the peak of torch's allocator over a round (MiB):
  bands_ms                       predictive.bands as a user calls it (nothing timed inside it)
  solve_ms, accumulate_ms,       the same call with a device synchronise around each stage (their sum exceeds bands_ms by what the
  quantiles_ms                   synchronises cost)
  old_solve_ms, old_moments_ms,  the old route's stages
  old_quantile_ms, old_ms
Every case runs in a child process of its own under `timeout`; a child that fails ends the run.
python tools/bench_predictive.py [--draws 256,4096,16384] [--chunk-mib 128,1024] [--nt 20001] [--rounds 3] [--timeout 280] [--out profiles/predictive.md]"""
import argparse
import importlib
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--draws", default="256,4096,16384")
ap.add_argument("--nt", type=int, default=20001)
ap.add_argument("--chunk-mib", default="128,1024")
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--timeout", type=int, default=280)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "predictive.md"))
ap.add_argument("--child", default="")
a = ap.parse_args()
Q = (0.025, 0.5, 0.975)


def report(cases):
    def row(c):
        if "error" in c:
            return f"| {c['draws']} | {c['error']} |"
        return (f"| {c['draws']:,} | {c['Nt']:,} | {c['chunk_mib']} | {c['chunks']} | {c['solve_ms']:.1f} | {c['accumulate_ms']:.2f} | {c['quantiles_ms']:.2f} | {c['bands_ms']:.1f} | "
                f"{c['bands_peak_mib']:,.0f} | {c['old_solve_ms']:.1f} | {c['old_moments_ms']:.2f} | {c['old_quantile_ms']:.1f} | {c['old_ms']:.1f} | "
                f"{c['old_peak_mib']:,.0f} | {c['max_abs_diff']:.1e} |").replace(",", " ")
    ok = [c for c in cases if "error" not in c]
    head = ok[0] if ok else {}
    at = lambda c: f"{c['draws']} draws in chunks of {c['chunk_mib']} MiB"   # noqa: E731
    slower = [at(c) for c in ok if c["bands_ms"] > c["old_ms"]]
    post = [at(c) for c in ok if c["accumulate_ms"] + c["quantiles_ms"] > c["old_moments_ms"] + c["old_quantile_ms"]]
    return "\n".join([
        "# Posterior predictive bands (`predictive.py`, `ionode_predictive_accumulate`, `ionode_predictive_quantiles`) beside the whole-trace route",
        "",
        f"Library sha256 `{head.get('library_sha256', '?')}`, one {head.get('gpu', 'GPU')}; written by `tools/bench_predictive.py`.",
        "",
        "HH 2-state, fp64 state, one sine-wave protocol, draws of p1 .. p4 (2 % log-normal around the ground truth), rtol 1e-7 / atol 1e-9,",
        "quantiles 0.025 / 0.5 / 0.975, no noise.  New route: `predictive.bands` with the `chunk_bytes` of the row (its default is 1 GiB) -- per chunk one",
        "fused solve that stores the current trace only and one accumulate launch, then one quantile launch.  Old route: one",
        "`batched.solve(current=True)` of all draws (states and current stored), `torch.mean` / `std` / `amin` / `amax` over the draws and",
        "`torch.quantile` on slices of time below its 16 M-element limit.  The routes alternate; best of the rounds, ms; peak of torch's",
        "allocator over a round, MiB; every case in a process of its own.  The three stage columns come from a run with a device",
        "synchronise around every stage, `bands` from a run without.  The last column is the largest absolute difference between the two",
        "routes' means, standard deviations and quantiles (currents of order 1 - 10).",
        "",
        "| draws | samples | `chunk_bytes`, MiB | chunks | solves | accumulate | quantiles | `bands` | peak MiB | old: solve | moments | `torch.quantile` | old route | peak MiB | max abs diff |",
        "|---:|---:|---:|---:|---:|---:|---:|---:|---:|---:|---:|---:|---:|---:|---:|",
        *[row(c) for c in cases],
        "",
        "Nobody had measured either route before this table; it sets no target.  A solve of these trajectories is bound by the",
        "length of one trajectory, not by their number (the old route's solve column hardly moves from 256 to 16 384 draws), so every",
        "chunk costs about one such solve: small chunks save memory and pay for it in time.",
        *([] if not ok else [
            ("The new route is SLOWER end to end at " + "; ".join(slower) + "." if slower
             else "The new route is faster end to end at every size measured."),
            ("Its two passes together take longer than the old route's torch reductions at " + "; ".join(post) + "."
             if post else "Its two passes together take less time than the old route's torch reductions at every size measured.")]),
        ""])


if not a.child:   # the parent never opens the GPU
    cases = []
    for n, mib in [(int(s), int(m)) for s in a.draws.split(",") for m in a.chunk_mib.split(",")]:
        r = subprocess.run(["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--child", f"{n}:{a.nt}:{mib}",
                            "--rounds", str(a.rounds)], stdout=subprocess.PIPE, text=True)
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        if r.returncode != 0 or not lines:
            cases.append({"draws": n, "error": f"child exit status {r.returncode}"})
            break   # (nothing more is started on a device that has just failed or hung)
        cases.append(json.loads(lines[-1]))
    with open(a.out, "w") as f:
        f.write(report(cases))
    print(json.dumps({"tool": "bench_predictive", "cases": cases}))
    sys.exit(0 if all("error" not in c for c in cases) else 1)

import numpy as np   # noqa: E402
import torch   # noqa: E402

sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import kat_cases as K  # noqa: E402

ion = importlib.import_module("neural-ode-ion-channels_amd")
pr = importlib.import_module("neural-ode-ion-channels_amd.predictive")
capi = ion.capi
dev = torch.device("cuda:0")
S, Nt, CHUNK_MIB = (int(s) for s in a.child.split(":"))
pv = ion.protocols.sinewave(ion.protocols.sinewave_scales(0, 1), n_samples=Nt, dt=0.1, xp=torch, device=dev)
te = torch.arange(Nt, dtype=torch.float64, device=dev) * 0.1
pv_h, te_h = pv.cpu().numpy(), te.cpu().numpy()
draws = K.P_HH[None, :4] * np.exp(0.02 * np.random.default_rng(0).normal(size=(S, 4)))
kw = dict(base_params=K.P_HH, free=(0, 1, 2, 3), prot_t0=0.0, prot_dt=0.1, state_dtype=torch.float64, quantiles=Q, device=dev,
          chunk_bytes=CHUNK_MIB << 20)
MIB = float(1 << 20)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) * 1e3


def peak_of(fn):
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats(dev)
    out = fn()
    torch.cuda.synchronize()
    return out, torch.cuda.max_memory_allocated(dev) / MIB


def new_route():
    return timed(lambda: pr.bands(K.MODEL_HH2, draws, pv_h, te_h, **kw))


def new_route_split():
    """bands with a synchronise around every stage: (Bands, {stage: ms}, chunks)."""
    ms = {"solve_ms": 0.0, "accumulate_ms": 0.0, "quantiles_ms": 0.0}
    chunks = [0]
    plain = (pr.accumulate, pr.quantile_pass)

    def solve(*args, **k):
        out, t = timed(lambda: ion.batched.solve(*args, **k))
        ms["solve_ms"] += t
        chunks[0] += 1
        return out

    def acc(*args, **k):
        ms["accumulate_ms"] += timed(lambda: plain[0](*args, **k))[1]

    def quant(*args, **k):
        out, t = timed(lambda: plain[1](*args, **k))
        ms["quantiles_ms"] += t
        return out

    pr.accumulate, pr.quantile_pass = acc, quant
    try:
        b = pr.bands(K.MODEL_HH2, draws, pv_h, te_h, solver=solve, **kw)
    finally:
        pr.accumulate, pr.quantile_pass = plain
    return b, ms, chunks[0]


def old_route():
    """(mean, sd, min, max, quantiles [Q, Nt]), {stage: ms}"""
    params = torch.from_numpy(np.concatenate([draws, np.tile(K.P_HH[4:], (S, 1))], axis=1)).to(dev)
    y0 = torch.tensor([[0.0, 1.0]], dtype=torch.float64, device=dev)
    sol, t_solve = timed(lambda: ion.batched.solve(K.MODEL_HH2, params, pv, y0, te, prot_t0=0.0, prot_dt=0.1, current=True))
    i = sol.i
    (mean, sd, mn, mx), t_mom = timed(lambda: (i.mean(dim=0), i.std(dim=0), i.amin(dim=0), i.amax(dim=0)))
    qt = torch.tensor(Q, dtype=torch.float64, device=dev)
    width = max(1, 16_000_000 // S)

    def quantiles():
        return torch.cat([torch.quantile(i[:, lo:lo + width], qt, dim=0) for lo in range(0, Nt, width)], dim=1)

    qv, t_q = timed(quantiles)
    return (mean, sd, mn, mx, qv), {"old_solve_ms": t_solve, "old_moments_ms": t_mom, "old_quantile_ms": t_q, "old_ms": t_solve + t_mom + t_q}


res = {"draws": S, "Nt": Nt, "chunk_mib": CHUNK_MIB, "state": "fp64", "gpu": torch.cuda.get_device_name(dev), "library_sha256": capi.library_digest()}
new_route()   # warm-up of both routes: code objects, the allocator
old_route()
best, peaks = {}, {"bands_peak_mib": 0.0, "old_peak_mib": 0.0}
for _ in range(a.rounds):
    (_, t), pk = peak_of(new_route)
    best["bands_ms"] = min(best.get("bands_ms", float("inf")), t)
    peaks["bands_peak_mib"] = max(peaks["bands_peak_mib"], pk)
    b, ms, chunks = new_route_split()
    (old, oms), pk = peak_of(old_route)
    peaks["old_peak_mib"] = max(peaks["old_peak_mib"], pk)
    for k, v in {**ms, **oms}.items():
        best[k] = min(best.get(k, float("inf")), v)
diff = max(float((b.mean[0] - old[0]).abs().max()), float((b.sd[0] - old[1]).abs().max()), float((b.min[0] - old[2]).abs().max()),
           float((b.max[0] - old[3]).abs().max()), float((b.quantiles[0] - old[4]).abs().max()))
res.update(best, **peaks, chunks=chunks, survivors=int(b.count[0]), max_abs_diff=diff)
print(json.dumps(res))
