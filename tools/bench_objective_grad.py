"""Dev tool: what the objective's kind costs the fused BACKWARD (profiles/objective_kinds.md).  Run from the repository root:

    python tools/bench_objective_grad.py --parent-lib path/to/the/parent/commit's/libionode.so [--rounds 3] [--reps 2] [--out file.json]

Arms, alternating, `--rounds` rounds, every arm of every round in a child process of its own (IONODE_LIB selects the library):
    parent sse   the parent commit's library: ionode_dopri5_backward_sse, which knows the squares alone
    this sse     this tree's library, grad.sum_of_squares  -- ionode_objective_backward reads the kind and takes the squares' side
    this sae     this tree's library, grad.sum_of_abs
and once, at the end, `--materialised`: grad.solve plus abs() in torch, the route the absolute values had before (time and peak memory).
Shape: README's fused-gradient row, 65 536 trajectories x 20 001 samples (0.1 ms grid), 64 sine-wave protocols, fp64 state, the stable
step cap; HH 2-state and 6-state.  A child runs one launch to warm up, then `--reps` times: forward (not timed), backward between two
synchronisations; it reports every backward time, the peak allocation over forward + backward and a digest of dL/dp.  The judgement:
`this sse` minus `parent sse` (medians over all launches) against the spread of the parent's own launches in this session."""
import argparse
import ctypes as C
import hashlib
import importlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
ARMS = (("parent sse", "parent", "sse"), ("this sse", "this", "sse"), ("this sae", "this", "sae"))
MODELS = ("hh", "m6")
OLD = {"ionode_objective_backward": "ionode_dopri5_backward_sse", "ionode_objective_backward_gc": "ionode_dopri5_backward_sse_gc"}


def child(kind, reps, batch, nt, materialised):
    import numpy as np
    import torch
    import kat_cases as K
    ion = importlib.import_module("neural-ode-ion-channels_amd")
    capi = ion.capi
    if not hasattr(C.CDLL(capi.LIB_PATH), "ionode_objective_backward"):
        # the parent commit's library: the squares' kind of the two new entry points IS the entry points it has
        assert kind == "sse" and not materialised

        class ParentLib(C.CDLL):
            def __getattr__(self, name):
                if name not in OLD:
                    return super().__getattr__(name)
                old = super().__getattr__(OLD[name])

                def call(d, objective, *a):
                    assert objective == capi.OBJECTIVE_SSE
                    return old(d, *a)
                self.__dict__[name] = call
                return call
        capi.C.CDLL = ParentLib
        lib = capi.lib()
        for new, old in OLD.items():
            getattr(lib, old).restype = C.c_int
            getattr(lib, old).argtypes = [C.POINTER(capi.IonodeDesc), C.c_int32, C.c_int32, C.c_int32] + [C.c_void_p] * (len(capi.SWEEP_BUFFERS[old]) + 1)
    dev = torch.device("cuda:0")
    B, Nt, NPROT = batch, nt, 64
    pv = ion.protocols.sinewave(ion.protocols.sinewave_scales(0, NPROT), n_samples=Nt, dt=0.1, xp=torch, device=dev)
    pot = (torch.arange(B, device=dev) % NPROT).to(torch.int32)
    te = torch.arange(Nt, dtype=torch.float64, device=dev) * 0.1
    vtab = capi.protocol_at_outputs(capi.make_desc(n_out=Nt, n_prot=NPROT, prot_n=Nt, prot_t0=0.0, prot_dt=0.1, v_oob=-80.0), pv, None, te)
    out = {"library": capi.LIB_PATH, "digest": capi.library_digest()[:16], "kind": kind, "materialised": bool(materialised)}
    for name in MODELS:
        m6 = name == "m6"
        model = K.MODEL_MARKOV6 if m6 else K.MODEL_HH2
        p0 = K.P_M6 if m6 else K.P_HH
        obs = dict(obs_g=1.0, obs_e=-86.0, obs_open_state_only=m6)
        y0 = torch.tensor([[0.0, 1.0] + ([0.0, 0.0, 0.0, 0.0] if m6 else [])], dtype=torch.float64, device=dev).repeat(B, 1)
        rng = np.random.default_rng(0)
        params = torch.from_numpy(np.tile(p0, (B, 1)) * rng.uniform(0.9, 1.1, (B, p0.size))).to(dev)
        cap = ion.grad.stable_step_cap(model, params, pv)
        nom = ion.batched.solve(model, torch.from_numpy(np.tile(p0, (NPROT, 1))).to(dev), pv, y0[:NPROT], te, prot_t0=0.0, prot_dt=0.1,
                                prot_of_traj=torch.arange(NPROT, dtype=torch.int32, device=dev), current=True, max_step=cap, **obs)
        ref = (nom.i + torch.from_numpy(rng.normal(0.0, 0.05, (NPROT, Nt))).to(dev)).contiguous()
        del nom
        fn = ion.grad.sum_of_squares if kind == "sse" else ion.grad.sum_of_abs

        def forward(p):
            if not materialised:
                return fn(model, p, pv, y0, te, ref, prot_t0=0.0, prot_dt=0.1, prot_of_traj=pot, max_step=cap, **obs)
            y, st = ion.grad.solve(model, None, p, pv, y0, te, prot_t0=0.0, prot_dt=0.1, prot_of_traj=pot, max_step=cap)
            gate = y[..., -1] if m6 else y[..., 0] * y[..., 1]
            r = obs["obs_g"] * gate * (vtab[pot.long()] - obs["obs_e"]) - ref[pot.long()]
            return ((r ** 2) if kind == "sse" else r.abs()).sum(1), st

        fwd, bwd, peak, digest, ok = [], [], 0, None, 0
        for rep in range(reps + 1):   # the first launch warms up
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats(dev)
            base = torch.cuda.memory_allocated(dev)
            p = params.clone().requires_grad_(True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            val, st = forward(p)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            val.sum().backward()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            if rep:
                fwd.append((t1 - t0) * 1e3)
                bwd.append((t2 - t1) * 1e3)
            peak = max(peak, int(torch.cuda.max_memory_allocated(dev) - base))
            digest = hashlib.sha256(p.grad.cpu().numpy().tobytes()).hexdigest()[:16]
            ok = int((st == 0).sum())
            del p, val, st
        out[name] = {"B": B, "Nt": Nt, "max_step_ms": cap, "fwd_ms": fwd, "bwd_ms": bwd, "peak_alloc_bytes": peak, "grad_digest": digest, "ok": ok}
        del params, y0, ref
        torch.cuda.empty_cache()
    print("RESULT " + json.dumps(out), flush=True)


def run_child(args, lib, kind, materialised=False):
    env = dict(os.environ, IONODE_LIB=lib)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--kind", kind, "--reps", str(args.reps), "--batch", str(args.batch), "--nt", str(args.nt)]
    p = subprocess.run(cmd + (["--materialised"] if materialised else []), cwd=ROOT, env=env, capture_output=True, text=True, timeout=args.child_timeout)
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
    if p.returncode != 0 or not line:
        # a child that failed ends the measurement: nothing further is started on the device
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
        raise SystemExit(f"child ({lib}, {kind}) exited with {p.returncode}")
    return json.loads(line[0][len("RESULT "):])


def parent(args):
    libs = {"parent": os.path.abspath(args.parent_lib), "this": os.path.join(ROOT, "neural-ode-ion-channels_amd", "libionode.so")}
    runs = {a[0]: [] for a in ARMS}
    for rnd in range(args.rounds):
        for arm, lib, kind in ARMS:
            res = run_child(args, libs[lib], kind)
            runs[arm].append(res)
            print(f"round {rnd} {arm:10s} " + "  ".join(f"{m} bwd {statistics.median(res[m]['bwd_ms']):.1f} ms" for m in MODELS), flush=True)
    summary = {}
    for m in MODELS:
        s = summary[m] = {}
        for arm, _, _ in ARMS:
            every = [t for r in runs[arm] for t in r[m]["bwd_ms"]]
            s[arm] = {"bwd_median_ms": statistics.median(every), "bwd_min_ms": min(every), "bwd_max_ms": max(every), "bwd_spread_ms": max(every) - min(every),
                      "launches": len(every), "fwd_median_ms": statistics.median([t for r in runs[arm] for t in r[m]["fwd_ms"]]),
                      "peak_alloc_bytes": max(r[m]["peak_alloc_bytes"] for r in runs[arm]), "ok": runs[arm][0][m]["ok"],
                      "grad_digests": sorted({r[m]["grad_digest"] for r in runs[arm]})}
        s["this_sse_minus_parent_ms"] = s["this sse"]["bwd_median_ms"] - s["parent sse"]["bwd_median_ms"]
        s["parent_spread_ms"] = s["parent sse"]["bwd_spread_ms"]
        s["this_sse_within_parent_spread"] = abs(s["this_sse_minus_parent_ms"]) <= s["parent_spread_ms"]
        s["squares_gradients_equal"] = s["this sse"]["grad_digests"] == s["parent sse"]["grad_digests"]
    doc = {"rounds": args.rounds, "reps_per_child": args.reps, "digests": {a[0]: runs[a[0]][0]["digest"] for a in ARMS}, "summary": summary}
    if args.materialised:
        mat = run_child(args, libs["this"], "sae", materialised=True)
        doc["materialised_sae"] = {m: {"fwd_median_ms": statistics.median(mat[m]["fwd_ms"]), "bwd_median_ms": statistics.median(mat[m]["bwd_ms"]),
                                       "peak_alloc_bytes": mat[m]["peak_alloc_bytes"], "ok": mat[m]["ok"]} for m in MODELS}
    print(json.dumps(doc, indent=1), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(dict(doc, runs=runs), f, indent=1)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--nt", type=int, default=20001)
    ap.add_argument("--out")
    ap.add_argument("--child-timeout", type=float, default=300.0)
    ap.add_argument("--materialised", action="store_true")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--kind", default="sse")
    a = ap.parse_args()
    if a.child:
        child(a.kind, a.reps, a.batch, a.nt, a.materialised)
    else:
        if not a.parent_lib:
            ap.error("--parent-lib is required")
        parent(a)
