"""Dev/bench tool (GPU box): the gradient of the sum-of-squares objective, fused (grad.sum_of_squares: checkpoints + per-trajectory
sums forward, ionode_dopri5_backward_sse backward) against the materialised route (grad.solve -> current and squared residuals in
torch -> autograd -> ionode_dopri5_backward), at the same size.  Per path: forward ms, backward ms, peak allocated bytes over
forward + backward.  One JSON line.
python tools/bench_sse_grad.py [--batch 65536] [--nt 20001] [--models hh,m6] [--reps 2]"""
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
import kat_cases as K  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=65536)
ap.add_argument("--nt", type=int, default=20001)
ap.add_argument("--models", default="hh,m6")
ap.add_argument("--reps", type=int, default=2)
a = ap.parse_args()
ion = importlib.import_module("neural-ode-ion-channels_amd")
dev = torch.device("cuda:0")
B, Nt, NPROT = a.batch, a.nt, 64
pv = ion.protocols.sinewave(ion.protocols.sinewave_scales(0, NPROT), n_samples=Nt, dt=0.1, xp=torch, device=dev)
pot = (torch.arange(B, device=dev) % NPROT).to(torch.int32)
te = torch.arange(Nt, dtype=torch.float64, device=dev) * 0.1
vtab = ion.capi.protocol_at_outputs(ion.capi.make_desc(n_out=Nt, n_prot=NPROT, prot_n=Nt, prot_t0=0.0, prot_dt=0.1, v_oob=-80.0),
                                    pv, None, te)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) * 1e3


def run_case(name):
    m6 = name == "m6"
    model = K.MODEL_MARKOV6 if m6 else K.MODEL_HH2
    p0 = K.P_M6 if m6 else K.P_HH
    obs = dict(obs_g=1.0, obs_e=-86.0, obs_open_state_only=m6)   # 6-state: the open state (train-d1.py:299)
    y0 = torch.tensor([[0.0, 1.0] + ([0.0, 0.0, 0.0, 0.0] if m6 else [])], dtype=torch.float64, device=dev).repeat(B, 1)
    rng = np.random.default_rng(0)
    params = torch.from_numpy(np.tile(p0, (B, 1)) * rng.uniform(0.9, 1.1, (B, p0.size))).to(dev)
    cap = ion.grad.stable_step_cap(model, params, pv)   # = max_step="auto" of both paths
    # data: the nominal model's current on every protocol plus noise
    nom = ion.batched.solve(model, torch.from_numpy(np.tile(p0, (NPROT, 1))).to(dev), pv, y0[:NPROT], te, prot_t0=0.0, prot_dt=0.1,
                            prot_of_traj=torch.arange(NPROT, dtype=torch.int32, device=dev), current=True, max_step=cap, **obs)
    ref = (nom.i + torch.from_numpy(rng.normal(0.0, 0.05, (NPROT, Nt))).to(dev)).contiguous()
    del nom
    res = {"model": name, "state": "fp64", "B": B, "Nt": Nt, "protocols": NPROT, "max_step_ms": cap}

    def fused():
        p = params.clone().requires_grad_(True)
        (sse, st), tf = timed(lambda: ion.grad.sum_of_squares(model, p, pv, y0, te, ref, prot_t0=0.0, prot_dt=0.1, prot_of_traj=pot,
                                                              max_step=cap, **obs))
        _, tb = timed(lambda: sse.sum().backward())
        return {"fwd_ms": tf, "bwd_ms": tb}, p.grad, sse.detach(), st

    def materialised():
        p = params.clone().requires_grad_(True)

        def fwd():
            y, st = ion.grad.solve(model, None, p, pv, y0, te, prot_t0=0.0, prot_dt=0.1, prot_of_traj=pot, max_step=cap)
            gate = y[..., -1] if m6 else y[..., 0] * y[..., 1]
            i = obs["obs_g"] * gate * (vtab[pot.long()] - obs["obs_e"])
            return ((i - ref[pot.long()]) ** 2).sum(1), st
        (sse, st), tf = timed(fwd)
        _, tb = timed(lambda: sse.sum().backward())
        return {"fwd_ms": tf, "bwd_ms": tb}, p.grad, sse.detach(), st

    grads = {}
    for label, fn in (("fused", fused), ("materialised", materialised)):
        best = None
        try:
            for _ in range(a.reps):
                torch.cuda.empty_cache()
                torch.cuda.reset_peak_memory_stats(dev)
                base = torch.cuda.memory_allocated(dev)
                t, g, sse, st = fn()
                t["peak_alloc_bytes"] = int(torch.cuda.max_memory_allocated(dev) - base)
                best = t if best is None or t["bwd_ms"] + t["fwd_ms"] < best["bwd_ms"] + best["fwd_ms"] else best
                grads[label] = (g.detach(), sse, st)
                del g
            best["ok"] = int((grads[label][2] == 0).sum())
        except torch.cuda.OutOfMemoryError as e:
            best = {"error": "out of memory", "detail": str(e).splitlines()[0]}
        res[label] = best
        torch.cuda.empty_cache()
    if "fused" in grads and "materialised" in grads:
        gf, sf, _ = grads["fused"]
        gm, sm, _ = grads["materialised"]
        res["rel_l2_dsse_dp"] = float((gf - gm).norm() / gm.norm())
        res["rel_sse"] = float(((sf - sm).abs() / sm.abs()).max())
    return res


cases = [run_case(m) for m in a.models.split(",")]
print(json.dumps({"tool": "bench_sse_grad", "gpu": torch.cuda.get_device_name(dev), "library_sha256": ion.capi.library_digest(),
                  "cases": cases}))
