"""Dev/bench tool (GPU box): the tangent sweep (sensitivity.gauss_newton / current_s1, ionode_tangent_sweep) beside what a user had
before it, in one run on one build.  fp64 state, the shape of README's fused-gradient rows.  Per model, best of --reps (ms):
  forward_ckpt_ms      the checkpointed fused forward (sensitivity's and grad.sum_of_squares')
  sweep_sums_ms        the tangent sweep, J^T r and J^T J only
  sweep_trace_ms       the tangent sweep with the [B, Nt, NPAR] trace, at --trace-batch trajectories
  backward_sse_ms      the fused sum-of-squares backward (grad.sum_of_squares(...).backward())
  forward_plain_ms     the fused forward without checkpoints; fd_route_ms = (NPAR + 1) x it, the finite-difference Jacobian a user has today
and the sweep kernel's registers (tools/kernel_resources.py) and achieved bytes/s of checkpoint reads (every lane group reads its
trajectory's records once: accepted steps x record bytes / sweep time).  One JSON line.
python tools/bench_tangent.py [--batch 65536] [--nt 20001] [--trace-batch 4096] [--models hh,m6] [--reps 3]"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kat_cases as K  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=65536)
ap.add_argument("--nt", type=int, default=20001)
ap.add_argument("--trace-batch", type=int, default=4096)
ap.add_argument("--models", default="hh,m6")
ap.add_argument("--reps", type=int, default=3)
a = ap.parse_args()
ion = importlib.import_module("neural-ode-ion-channels_amd")
sens = importlib.import_module("neural-ode-ion-channels_amd.sensitivity")
dev = torch.device("cuda:0")
B, Nt, NPROT = a.batch, a.nt, 64
pv = ion.protocols.sinewave(ion.protocols.sinewave_scales(0, NPROT), n_samples=Nt, dt=0.1, xp=torch, device=dev)
te = torch.arange(Nt, dtype=torch.float64, device=dev) * 0.1


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) * 1e3


def best_of(fn):
    out, best = None, float("inf")
    for _ in range(a.reps):
        out, t = timed(fn)
        best = min(best, t)
    return out, best


def registers(model):
    try:
        from kernel_resources import kernel_resources
        rows = [r for r in kernel_resources(ion.capi.LIB_PATH) if f"ionode_tangent_sweep_kernel<{model}, double>" in r["kernel"]]
        return {"vgpr_unified": rows[0]["vgpr"], "agpr": rows[0]["agpr"], "scratch_bytes": rows[0]["scratch_bytes"]}
    except Exception as e:   # (the llvm tools are not on every box)
        return {"error": str(e)}


def run_case(name):
    m6 = name == "m6"
    model = K.MODEL_MARKOV6 if m6 else K.MODEL_HH2
    p0 = K.P_M6 if m6 else K.P_HH
    npar = p0.size
    obs = dict(obs_g=1.0, obs_e=-86.0, obs_open_state_only=m6)   # 6-state: the open state (train-d1.py:299)
    rng = np.random.default_rng(0)

    def batch(n):
        y0 = torch.tensor([[0.0, 1.0] + ([0.0, 0.0, 0.0, 0.0] if m6 else [])], dtype=torch.float64, device=dev).repeat(n, 1)
        params = torch.from_numpy(np.tile(p0, (n, 1)) * np.random.default_rng(0).uniform(0.9, 1.1, (n, npar))).to(dev)
        return params, y0, (torch.arange(n, device=dev) % NPROT).to(torch.int32)
    params, y0, pot = batch(B)
    cap = ion.grad.stable_step_cap(model, params, pv)
    nom = ion.batched.solve(model, torch.from_numpy(np.tile(p0, (NPROT, 1))).to(dev), pv, y0[:NPROT], te, prot_t0=0.0, prot_dt=0.1,
                            prot_of_traj=torch.arange(NPROT, dtype=torch.int32, device=dev), current=True, max_step=cap, **obs)
    ref = (nom.i + torch.from_numpy(rng.normal(0.0, 0.05, (NPROT, Nt))).to(dev)).contiguous()
    del nom
    kw = dict(prot_t0=0.0, prot_dt=0.1, max_step=cap, **obs)
    res = {"model": name, "state": "fp64", "B": B, "Nt": Nt, "NPAR": npar, "protocols": NPROT, "max_step_ms": cap, "kernel": registers(model)}

    # the fused forward alone: what (NPAR + 1) finite-difference solves cost
    sol, res["forward_plain_ms"] = best_of(lambda: ion.batched.solve(model, params, pv, y0, te, prot_of_traj=pot, sse_ref=ref, states=False, **kw))
    res["fd_route_ms"] = (npar + 1) * res["forward_plain_ms"]
    del sol

    # checkpointed forward, then the sweep with sums only (sensitivity.gauss_newton's two launches, timed apart)
    full = dict(prot_t=None, prot_of_traj=pot, rtol=1e-7, atol=1e-9, v_oob=-80.0, max_steps=0, max_total_steps=0, ckpt_cap=None,
                ckpt_budget_bytes=None, **kw)
    hint = ion.grad.uniform_grid_hint(te)
    fwd, res["forward_ckpt_ms"] = best_of(lambda: sens._forward(model, params, pv, y0, te, full, sse_ref=ref, objective="sse", t_eval_hint=hint))
    r, cfg, p, ckpt, n_acc = fwd
    jtr = torch.empty((B, npar), dtype=torch.float64, device=dev)
    jtj = torch.empty((B, npar, npar), dtype=torch.float64, device=dev)
    _, res["sweep_sums_ms"] = best_of(lambda: sens._sweep(r, cfg, p, ckpt, n_acc, None, jtr, jtj))
    steps = int(n_acc.sum())
    res["accepted_steps_mean"] = steps / B
    res["ckpt_read_GBps"] = steps * ckpt.shape[2] * 8 / (res["sweep_sums_ms"] * 1e-3) / 1e9
    res["gauss_newton_ms"] = res["forward_ckpt_ms"] + res["sweep_sums_ms"]
    res["ok"] = int((r["status"] == 0).sum())
    del fwd, r, cfg, p, ckpt, n_acc, jtr, jtj
    torch.cuda.empty_cache()

    # the fused reverse sweep on the same inputs
    def reverse():
        pr = params.clone().requires_grad_(True)
        (sse, st), tf = timed(lambda: ion.grad.sum_of_squares(model, pr, pv, y0, te, ref, prot_of_traj=pot, **kw))
        _, tb = timed(lambda: sse.sum().backward())
        return tf, tb
    res["backward_sse_ms"] = min(reverse()[1] for _ in range(a.reps))
    torch.cuda.empty_cache()

    # the trace, at a batch whose [B, Nt, NPAR] fits
    Bt = min(a.trace_batch, B)
    pt, y0t, pott = batch(Bt)
    fwd = sens._forward(model, pt, pv, y0t, te, dict(full, prot_of_traj=pott), forward_kw=dict(current=True, **obs))
    r, cfg, p, ckpt, n_acc = fwd
    di_dp = torch.empty((Bt, Nt, npar), dtype=torch.float64, device=dev)
    _, res["sweep_trace_ms"] = best_of(lambda: sens._sweep(r, cfg, p, ckpt, n_acc, di_dp, None, None))
    res["trace_batch"] = Bt
    res["trace_write_GBps"] = di_dp.numel() * 8 / (res["sweep_trace_ms"] * 1e-3) / 1e9
    return res


cases = [run_case(m) for m in a.models.split(",")]
print(json.dumps({"tool": "bench_tangent", "gpu": torch.cuda.get_device_name(dev), "library_sha256": ion.capi.library_digest(),
                  "cases": cases}))
