"""Dev/bench tool (GPU box): ms per Adam iteration of the MLP regression loop (regress + reduce + Adam + image refresh) at the
reference's row count, for widths WITHOUT a tuned tile (the run-time-width kernels, csrc/ionode_grad_gen.hpp) and, at N = 100 and
N = 200, the tuned kernels against the run-time-width ones (IONODE_GRAD_GENERIC=1, read on every call).

python tools/bench_regress_widths.py [--rows 132410] [--reps 5] [--out FILE]   -> one JSON line per case (also appended to FILE)

Per case: warm-up iterations first (code objects, allocator), then `reps` timed windows of at least ~1 s each, every window ended
by a device synchronise; the median window and the spread are reported.  The A/B pairs alternate tuned / generic windows.
"""
import argparse, importlib, json, os, sys, time
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=132410)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--out", default=None)
a = ap.parse_args()
assert torch.cuda.is_available(), "needs an MI355X: there is no CPU path"
ion = importlib.import_module("neural-ode-ion-channels_amd")
reg = importlib.import_module("neural-ode-ion-channels_amd.regression")
rng = np.random.default_rng(0)
x = np.stack([rng.uniform(-1.3, 0.7, a.rows), rng.uniform(0.01, 0.99, a.rows)], 1).astype(np.float32)
y = rng.normal(0, 1e-3, a.rows).astype(np.float32)


def trainer(L, N, generic):
    if generic:
        os.environ["IONODE_GRAD_GENERIC"] = "1"
    else:
        os.environ.pop("IONODE_GRAD_GENERIC", None)
    w = np.random.default_rng(N).normal(0, 0.1, 2 * N + N + L * (N * N + N) + N + 1).astype(np.float32)
    r = reg.MlpRegression(w, L, N, x, y, device="cuda:0")
    plan = ion.capi.regress_plan(L, N)
    assert plan["generic"] == bool(generic or plan["generic"])
    return r, plan


def window(r, generic, iters):
    if generic:
        os.environ["IONODE_GRAD_GENERIC"] = "1"
    else:
        os.environ.pop("IONODE_GRAD_GENERIC", None)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        r.step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


def measure(L, N, variants):
    rs = {g: trainer(L, N, g) for g in variants}
    iters = {}
    for g, (r, _) in rs.items():
        window(r, g, 3)                                    # warm-up
        iters[g] = max(3, int(1000.0 / max(window(r, g, 3), 1e-3)) + 1)   # a window of >= ~1 s
    ms = {g: [] for g in variants}
    for _ in range(a.reps):
        for g in variants:                                 # alternate the variants
            ms[g].append(window(rs[g][0], g, iters[g]))
    for g in variants:
        r, plan = rs[g]
        flops = 3 * 2 * a.rows * (L * N * N + 3 * N)
        med = float(np.median(ms[g]))
        line = json.dumps({"workload": f"MLP regression step, {a.rows} rows, net 2->{N}x{L}->1, fp32",
                           "kernels": "run-time-width" if plan["generic"] else "tuned", "wg_per_cu": plan["wg_per_cu"],
                           "lds_bytes": plan["lds_bytes"], "n_slabs": r.n_slabs, "iters_per_window": iters[g],
                           "ms_per_iteration": round(med, 4), "min": round(min(ms[g]), 4), "max": round(max(ms[g]), 4),
                           "algorithmic_TFLOPs": round(flops / med / 1e9, 3)})
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")


for N in (50, 64, 150, 300):
    measure(5, N, (False,))
for N in (100, 200):
    measure(5, N, (False, True))
