"""Dev/bench tool (GPU box): the gradient of the sum-of-squares objective for the NN models, fused (grad.sum_of_squares with
weights_flat: checkpoints + per-trajectory sums forward; ionode_dopri5_backward_sse_gc + the two-phase sweep without grad_y backward)
against the materialised route (grad.solve -> current and squared residuals in torch -> autograd -> the two-phase sweep with grad_y),
at the same size.  Per path: forward ms, backward ms, peak allocated bytes over forward + backward.  One JSON line.
Shapes: s00 = NN-f 5 x 200, 1024 x 100 001, fp32 state (BASELINE configs[4]'s per-GPU share); s03 = NN-f 5 x 10, 65 536 x 20 001, fp64.
python tools/bench_sse_grad_nn.py [--shapes s00,s03] [--reps 2] [--batch B] [--nt Nt]"""
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

SHAPES = {"s00": dict(L=5, N=200, B=1024, Nt=100001, f32=True), "s03": dict(L=5, N=10, B=65536, Nt=20001, f32=False)}
ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default="s00,s03")
ap.add_argument("--reps", type=int, default=2)
ap.add_argument("--batch", type=int, default=0)
ap.add_argument("--nt", type=int, default=0)
a = ap.parse_args()
ion = importlib.import_module("neural-ode-ion-channels_amd")
dev = torch.device("cuda:0")
NPROT = 64


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) * 1e3


def run_case(name):
    sh = SHAPES[name]
    L, N, f32 = sh["L"], sh["N"], sh["f32"]
    B, Nt = a.batch or sh["B"], a.nt or sh["Nt"]
    model = K.MODEL_NNF
    sdt = torch.float32 if f32 else torch.float64
    rng = np.random.default_rng(0)
    if name == "s00":
        w = K.load_weights("s1")
    else:   # no trained 5 x 10 net ships with the tests: gain ~1 per layer
        w = rng.normal(0, 0.3, 2 * N + N + L * (N * N + N) + N + 1).astype(np.float32)
    pv = ion.protocols.sinewave(ion.protocols.sinewave_scales(0, NPROT), n_samples=Nt, dt=0.1, xp=torch, device=dev)
    pot = (torch.arange(B, device=dev) % NPROT).to(torch.int32)
    te = torch.arange(Nt, dtype=torch.float64, device=dev) * 0.1
    vtab = ion.capi.protocol_at_outputs(ion.capi.make_desc(n_out=Nt, n_prot=NPROT, prot_n=Nt, prot_t0=0.0, prot_dt=0.1, v_oob=-80.0),
                                        pv, None, te)
    y0 = torch.tensor([[0.0, 1.0]], dtype=sdt, device=dev).repeat(B, 1)
    params = torch.from_numpy(np.tile(K.P_HH, (B, 1)) * rng.uniform(0.9, 1.1, (B, 8))).to(dev)
    cap = ion.grad.stable_step_cap(model, params, pv)   # = max_step="auto" of both paths
    kw = dict(mlp_layers=L, mlp_width=N, prot_t0=0.0, prot_dt=0.1, prot_of_traj=pot, max_step=cap)
    # data: the nominal parameters' current on every protocol plus noise
    nom = ion.batched.solve(model, torch.from_numpy(np.tile(K.P_HH, (NPROT, 1))).to(dev), pv, y0[:NPROT], te, weights=w, mlp_layers=L,
                            mlp_width=N, prot_t0=0.0, prot_dt=0.1, prot_of_traj=torch.arange(NPROT, dtype=torch.int32, device=dev),
                            current=True, max_step=cap)
    ref = (nom.i + torch.from_numpy(rng.normal(0.0, 0.05, (NPROT, Nt))).to(dev)).contiguous()
    del nom
    res = {"shape": name, "model": "NN-f", "L": L, "N": N, "state": "fp32" if f32 else "fp64", "B": B, "Nt": Nt, "protocols": NPROT,
           "max_step_ms": cap}

    def leaves():
        return torch.from_numpy(w.copy()).to(dev).requires_grad_(True), params.clone().requires_grad_(True)

    def fused():
        wt, p = leaves()
        (sse, st), tf = timed(lambda: ion.grad.sum_of_squares(model, p, pv, y0, te, ref, weights_flat=wt, weights_key=("bench", name), **kw))
        _, tb = timed(lambda: sse.sum().backward())
        return {"fwd_ms": tf, "bwd_ms": tb}, (wt.grad.double(), p.grad), sse.detach(), st

    def materialised():
        wt, p = leaves()

        def fwd():
            y, st = ion.grad.solve(model, wt, p, pv, y0, te, weights_key=("bench", name), t_eval_hint=(0.0, 0.1), **kw)
            i = (y[..., 0] * y[..., 1]).double() * (vtab[pot.long()] + 86.0)
            per = ((i - ref[pot.long()]) ** 2).sum(1)
            return torch.where(st == 0, per, torch.zeros_like(per)), st
        (sse, st), tf = timed(fwd)
        _, tb = timed(lambda: sse.sum().backward())
        return {"fwd_ms": tf, "bwd_ms": tb}, (wt.grad.double(), p.grad), sse.detach(), st

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
                grads[label] = (g, sse, st)
                del g
            best["ok"] = int((grads[label][2] == 0).sum())
        except torch.cuda.OutOfMemoryError as e:
            best = {"error": "out of memory", "detail": str(e).splitlines()[0]}
        res[label] = best
        torch.cuda.empty_cache()
    if "fused" in grads and "materialised" in grads:
        (gwf, gpf), sf, stf = grads["fused"]
        (gwm, gpm), sm, _ = grads["materialised"]
        ok = stf == 0
        res["rel_l2_dsse_dw"] = float((gwf - gwm).norm() / gwm.norm())
        res["rel_l2_dsse_dp"] = float((gpf - gpm)[:, 4:].norm() / gpm[:, 4:].norm())
        res["rel_sse"] = float(((sf - sm).abs() / sm.abs())[ok].max())
    return res


cases = [run_case(s) for s in a.shapes.split(",")]
print(json.dumps({"tool": "bench_sse_grad_nn", "gpu": torch.cuda.get_device_name(dev), "library_sha256": ion.capi.library_digest(),
                  "cases": cases}))
