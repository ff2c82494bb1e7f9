"""Dev/bench tool (GPU box): the NN models' tangent sweep (sensitivity.gauss_newton with weights: ionode_tangent_sweep_nn) beside what
a user had before it, in one run on one build.  Per case -- s00 (NN-f, 5 x 200) and NN-d (5, 200), fp32 and fp64 state -- best of
--reps (ms):
  forward_ckpt_ms      the checkpointed fused forward (sensitivity's and grad.sum_of_squares')
  sweep_ms             the chunk loop of ionode_tangent_sweep_nn, J^T r and J^T J only: recompute kernel + tangent walk per chunk
  recompute_ms         the recompute kernel alone on the same chunks (ionode_dopri5_backward_recompute_sse without records: the very
                       launch the entry point makes)
  walk_ms              sweep_ms - recompute_ms: the tangent walk (the two run back to back on one stream)
  forward_plain_ms     the fused forward without checkpoints; fd_route_ms = (n_free + 1) x it, the finite-difference Jacobian a user
                       has today (n_free = 4 for NN-f, p5..p8; 8 for NN-d)
  backward_sse_ms      the fused reverse sweep, dL/dp only (grad.sum_of_squares(...).backward(), no weight gradient)
and the walk kernel's registers (tools/kernel_resources.py).  One JSON line; --md prints the table of profiles/tangent_nn.md.
python tools/bench_tangent_nn.py [--batch 1024] [--nt 20001] [--reps 3] [--md]"""
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
ap.add_argument("--batch", type=int, default=1024)
ap.add_argument("--nt", type=int, default=20001)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--md", action="store_true")
a = ap.parse_args()
ion = importlib.import_module("neural-ode-ion-channels_amd")
sens = importlib.import_module("neural-ode-ion-channels_amd.sensitivity")
capi, grad = ion.capi, ion.grad
dev = torch.device("cuda:0")
B, Nt, NPROT, L, N = a.batch, a.nt, 64, 5, 200
pv = ion.protocols.sinewave(ion.protocols.sinewave_scales(0, NPROT), n_samples=Nt, dt=0.1, xp=torch, device=dev)
te = torch.arange(Nt, dtype=torch.float64, device=dev) * 0.1
W = K.load_weights("s1")   # the trained 5 x 200 net of s00


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


def registers(model, f32):
    try:
        from kernel_resources import kernel_resources
        name = f"ionode_tangent_walk_kernel<{model}, {'float' if f32 else 'double'}>"
        rows = [r for r in kernel_resources(capi.LIB_PATH) if name in r["kernel"]]
        return {"vgpr_unified": rows[0]["vgpr"], "agpr": rows[0]["agpr"], "scratch_bytes": rows[0]["scratch_bytes"]}
    except Exception as e:   # (the llvm tools are not on every box)
        return {"error": str(e)}


def run_case(model, f32):
    nnd = model == K.MODEL_NND
    n_free = 8 if nnd else 4
    sdt = torch.float32 if f32 else torch.float64
    y0 = torch.tensor([[0.0, 1.0]], dtype=sdt, device=dev).repeat(B, 1)
    params = torch.from_numpy(np.tile(K.P_HH, (B, 1)) * np.random.default_rng(0).uniform(0.9, 1.1, (B, 8))).to(dev)
    pot = (torch.arange(B, device=dev) % NPROT).to(torch.int32)
    mlp = dict(weights=W, mlp_layers=L, mlp_width=N)
    cap = grad.stable_step_cap(model, params, pv)
    nom = ion.batched.solve(model, torch.from_numpy(np.tile(K.P_HH, (NPROT, 1))).to(dev), pv, y0[:NPROT], te, prot_t0=0.0, prot_dt=0.1,
                            prot_of_traj=torch.arange(NPROT, dtype=torch.int32, device=dev), current=True, max_step=cap, **mlp)
    ref = (nom.i + torch.from_numpy(np.random.default_rng(1).normal(0.0, 0.05, (NPROT, Nt))).to(dev)).contiguous()
    del nom
    kw = dict(prot_t0=0.0, prot_dt=0.1, max_step=cap)
    res = {"model": "NN-d" if nnd else "NN-f (s00)", "state": "fp32" if f32 else "fp64", "B": B, "Nt": Nt, "L": L, "N": N, "n_free": n_free,
           "max_step_ms": cap, "kernel": registers(model, f32)}

    sol, res["forward_plain_ms"] = best_of(lambda: ion.batched.solve(model, params, pv, y0, te, prot_of_traj=pot, sse_ref=ref, states=False, **kw, **mlp))
    res["fd_route_ms"] = (n_free + 1) * res["forward_plain_ms"]
    del sol

    full = dict(prot_t=None, prot_of_traj=pot, rtol=1e-7, atol=1e-9, v_oob=-80.0, max_steps=0, max_total_steps=0, ckpt_cap=None,
                ckpt_budget_bytes=None, obs_g=1.0, obs_e=-86.0, obs_open_state_only=False, **kw)
    hint = grad.uniform_grid_hint(te)
    nn = (W, L, N, "bench", None, None)
    fwd, res["forward_ckpt_ms"] = best_of(lambda: sens._forward(model, params, pv, y0, te, full, sse_ref=ref, objective="sse", t_eval_hint=hint, nn=nn))
    r, cfg, p, ckpt, n_acc = fwd
    jtr = torch.empty((B, 8), dtype=torch.float64, device=dev)
    jtj = torch.empty((B, 8, 8), dtype=torch.float64, device=dev)
    _, res["sweep_ms"] = best_of(lambda: sens._sweep(r, cfg, p, ckpt, n_acc, None, jtr, jtj))

    # the recompute launches alone, on the same chunks and the same packet buffer size
    desc = r["desc"]
    n_iter = int(n_acc.max().item()) + 1
    tiles, pkd = (B + 15) // 16, int(capi.lib().ionode_grad_packet_doubles())
    chunk, bounds = sens.nn_chunks(n_iter, tiles, pkd, grad._bounded_budget(None, grad.DEFAULT_RECORD_BUDGET, dev, 0.5))
    packets = torch.empty(tiles * chunk * pkd, dtype=torch.float64, device=dev)
    image = grad.grad_image(cfg["w_np"], L, N, dev, key="bench")
    stream = torch.cuda.current_stream(dev)

    def recompute():
        for it0, it1 in bounds:
            capi.sweep_launch("ionode_dopri5_backward_recompute_sse", desc, it0, it1, n_iter, stream, grad_image=image, params=p, prot_v=pv,
                              prot_t=None, prot_of_traj=pot, t_eval=te, n_accepted=n_acc, records=None, packets=packets)
    _, res["recompute_ms"] = best_of(recompute)
    res["walk_ms"] = res["sweep_ms"] - res["recompute_ms"]
    res["chunks"], res["n_iter"] = len(bounds), n_iter
    res["accepted_steps_mean"] = int(n_acc.sum()) / B
    res["gauss_newton_ms"] = res["forward_ckpt_ms"] + res["sweep_ms"]
    res["ok"] = int((r["status"] == 0).sum())
    del fwd, r, cfg, ckpt, n_acc, jtr, jtj, packets
    torch.cuda.empty_cache()

    def reverse():
        pr = params.clone().requires_grad_(True)
        (sse, st), tf = timed(lambda: grad.sum_of_squares(model, pr, pv, y0, te, ref, prot_of_traj=pot, weights_flat=torch.from_numpy(W).to(dev),
                                                          mlp_layers=L, mlp_width=N, weights_key="bench", **kw))
        _, tb = timed(lambda: sse.sum().backward())
        return tf, tb
    res["backward_sse_ms"] = min(reverse()[1] for _ in range(a.reps))
    res["gn_over_fd"] = res["gauss_newton_ms"] / res["fd_route_ms"]
    res["gn_over_reverse"] = res["gauss_newton_ms"] / (res["forward_ckpt_ms"] + res["backward_sse_ms"])
    torch.cuda.empty_cache()
    return res


cases = [run_case(m, f32) for m in (K.MODEL_NNF, K.MODEL_NND) for f32 in (True, False)]
out = {"tool": "bench_tangent_nn", "gpu": torch.cuda.get_device_name(dev), "library_sha256": capi.library_digest(), "cases": cases}
print(json.dumps(out))
if a.md:
    rows = [("accepted steps per trajectory (mean)", "accepted_steps_mean", "{:.0f}"), ("sweep iterations / chunks", None, None),
            ("fused forward, no checkpoints", "forward_plain_ms", "{:.1f} ms"), ("finite-difference Jacobian: (n_free + 1) x that", "fd_route_ms", "{:.1f} ms"),
            ("checkpointed fused forward", "forward_ckpt_ms", "{:.1f} ms"), ("recompute kernel (all chunks)", "recompute_ms", "{:.1f} ms"),
            ("tangent walk (sweep - recompute)", "walk_ms", "{:.1f} ms"), ("**`gauss_newton` = forward + recompute + walk**", "gauss_newton_ms", "**{:.1f} ms**"),
            ("fused reverse sweep, dL/dp only (backward alone)", "backward_sse_ms", "{:.1f} ms"), ("`gauss_newton` / finite differences", "gn_over_fd", "{:.2f} x"),
            ("`gauss_newton` / (checkpointed forward + reverse sweep)", "gn_over_reverse", "{:.2f} x")]
    print("| leg | " + " | ".join(f"{c['model']}, {c['state']}" for c in cases) + " |")
    print("|---|" + "---|" * len(cases))
    for label, key, fmt in rows:
        cells = [f"{c['n_iter']} / {c['chunks']}" if key is None else fmt.format(c[key]) for c in cases]
        print(f"| {label} | " + " | ".join(cells) + " |")
    print("| walk kernel registers | " + " | ".join(f"{c['kernel'].get('vgpr_unified')} VGPR, scratch {c['kernel'].get('scratch_bytes')} B" for c in cases) + " |")
