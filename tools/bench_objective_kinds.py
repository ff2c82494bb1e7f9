"""Dev tool: what the fused objective's run-time kind costs (profiles/objective_kinds.md).  Run from the repository root:

    python tools/bench_objective_kinds.py --parent-lib path/to/the/parent/commit's/libionode.so [--rounds 5] [--out file.json]

Three arms, alternating, `--rounds` rounds, every arm of every round in a child process of its own (IONODE_LIB selects the library,
as tests/golden/make_grad_entry_checks.py describes):
    parent sse   the parent commit's library, sum of squares
    this sse     this tree's library, sum of squares  -- the flag is read, the multiply is taken
    this sae     this tree's library, sum of absolute values
Two shapes, both with states=False (nothing but one double per trajectory leaves the kernel), 64 sine-wave protocols, 0.1 ms grid:
    hh2_f32      HH 2-state, fp32 state, 196 608 x 20 001  (BASELINE configs[3]'s inner operation; the table variant)
    markov6_f64  6-state, fp64 state, 65 536 x 20 001
A child warms up, then times `--reps` launches between two events on the launch stream (the protocol-at-outputs table is made once,
ahead of the timed region) and reports their median.  The judgement: `this sse` within three times the parent's measured spread of
the parent's median (the rule of profiles/compose_order.md); `this sae` has no target.
"""
import argparse
import ctypes as C
import importlib
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ARMS = (("parent sse", "parent", "sse"), ("this sse", "this", "sse"), ("this sae", "this", "sae"))
SHAPES = ("hh2_f32", "markov6_f64")


def child(kind, reps):
    import numpy as np
    import torch
    import bench
    ion = importlib.import_module("neural-ode-ion-channels_amd")
    capi, P = ion.capi, ion.protocols
    probe = C.CDLL(capi.LIB_PATH)
    if not hasattr(probe, "ionode_dopri5_objective"):
        # the parent commit's library: capi.dopri5 launches through ionode_dopri5_objective, whose kind 0 IS ionode_dopri5_composed
        assert kind == "sse"

        class ParentLib(C.CDLL):
            def __getattr__(self, name):
                if name != "ionode_dopri5_objective":
                    return super().__getattr__(name)
                composed = self.ionode_dopri5_composed

                def forward(*a):
                    assert a[-1] == capi.OBJECTIVE_SSE
                    return composed(*a[:-1])
                self.__dict__[name] = forward
                return forward
        capi.C.CDLL = ParentLib
    dev = torch.device("cuda:0")
    Nt, n_prot = 20001, 64
    pv = P.sinewave(P.sinewave_scales(0, n_prot), n_samples=Nt, xp=torch, device=dev)
    te = torch.arange(Nt, dtype=torch.float64, device=dev) * 0.1
    rng = np.random.default_rng(0)
    p_m6 = np.array([5.94625498751561316e-02, 1.21417701632850410e+02, 4.76436985414236425e+00, 3.49383233960778904e-03,
                     9.62243079990877703e+01, 2.26404683824047979e+01, 8.00924780462999131e+00, 2.43749808069009823e+01,
                     2.06822607368134157e+02, 3.30791433507312362e+01, 1.26069071928587784e+00, 2.24844970727316245e+01]) * 1e-3
    ref = torch.from_numpy(rng.normal(0.0, 0.1, (n_prot, Nt))).to(dev)
    out = {"library": capi.LIB_PATH, "digest": capi.library_digest()[:16], "kind": kind}
    for name, model, p0, y0, B, sdt, extra in (("hh2_f32", capi.MODEL_HH2, bench.P_HH, [0.0, 1.0], 196608, torch.float32, {}),
                                               ("markov6_f64", capi.MODEL_MARKOV6, p_m6, [0.0, 1.0, 0, 0, 0, 0], 65536, torch.float64,
                                                dict(obs_open_state_only=True))):
        params = torch.from_numpy(p0[None, :] * rng.uniform(0.8, 1.25, (B, p0.size))).to(dev)
        y0t = torch.tensor([y0], dtype=sdt, device=dev).repeat(B, 1).contiguous()
        pot = (torch.arange(B, dtype=torch.int32, device=dev) % n_prot).contiguous()
        kw = dict(prot_t0=0.0, prot_dt=0.1, prot_of_traj=pot, t_eval_hint=(0.0, 0.1), t_eval_exact=True, sse_ref=ref, states=False,
                  stats=False, **extra)
        if kind != "sse":
            kw["objective"] = kind
        o = {}
        r = capi.dopri5(model, params, pv, y0t, te, out=o, **kw)       # warm-up; makes the table and the launch order once
        kw.update(v_at_outputs=r["v_at_outputs"], launch_order=r["launch_order"])
        o.update({kind: r[kind], "status": r["status"]})
        capi.dopri5(model, params, pv, y0t, te, out=o, **kw)
        torch.cuda.synchronize()
        ms = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            r = capi.dopri5(model, params, pv, y0t, te, out=o, **kw)
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        val = r[kind]
        out[name] = {"kernel": r["kernel"], "trajectories": B, "n_out": Nt, "ms": ms, "median_ms": statistics.median(ms),
                     "ok": int((r["status"] == 0).sum().item()), "finite": int(torch.isfinite(val).sum().item()),
                     "sum": float(val[torch.isfinite(val)].sum().item())}
        del params, y0t, pot, o, r
        torch.cuda.empty_cache()
    print("RESULT " + json.dumps(out), flush=True)


def parent(args):
    this_lib = os.path.join(ROOT, "neural-ode-ion-channels_amd", "libionode.so")
    libs = {"parent": os.path.abspath(args.parent_lib), "this": this_lib}
    runs = {a[0]: [] for a in ARMS}
    for rnd in range(args.rounds):
        for arm, lib, kind in ARMS:
            env = dict(os.environ, IONODE_LIB=libs[lib])
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--kind", kind, "--reps", str(args.reps)], cwd=ROOT, env=env,
                               capture_output=True, text=True, timeout=args.child_timeout)
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
            if p.returncode != 0 or not line:
                # a child that failed ends the measurement: nothing further is started on the device
                sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
                raise SystemExit(f"round {rnd}, arm '{arm}': child exited with {p.returncode}")
            res = json.loads(line[0][len("RESULT "):])
            runs[arm].append(res)
            print(f"round {rnd} {arm:10s} " + "  ".join(f"{s} {res[s]['median_ms']:.3f} ms" for s in SHAPES), flush=True)
    summary = {}
    for s in SHAPES:
        summary[s] = {}
        for arm, _, _ in ARMS:
            med = [r[s]["median_ms"] for r in runs[arm]]
            summary[s][arm] = {"kernel": runs[arm][0][s]["kernel"], "median_ms": statistics.median(med), "min_ms": min(med), "max_ms": max(med),
                               "spread_ms": max(med) - min(med), "per_round_ms": med, "ok": runs[arm][0][s]["ok"], "sum": runs[arm][0][s]["sum"]}
        pa, ts, ta = (summary[s][a[0]] for a in ARMS)
        summary[s]["this_sse_minus_parent_ms"] = ts["median_ms"] - pa["median_ms"]
        summary[s]["three_parent_spreads_ms"] = 3.0 * pa["spread_ms"]
        summary[s]["this_sse_within_three_parent_spreads"] = abs(ts["median_ms"] - pa["median_ms"]) <= 3.0 * pa["spread_ms"]
        summary[s]["squares_sums_equal"] = ts["sum"] == pa["sum"]
        summary[s]["this_sae_over_this_sse"] = ta["median_ms"] / ts["median_ms"]
    doc = {"rounds": args.rounds, "reps_per_child": args.reps, "digests": {a[0]: runs[a[0]][0]["digest"] for a in ARMS}, "summary": summary}
    print(json.dumps(doc, indent=1))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(dict(doc, runs=runs), f, indent=1)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out")
    ap.add_argument("--child-timeout", type=float, default=120.0)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--kind", default="sse")
    a = ap.parse_args()
    if a.child:
        child(a.kind, a.reps)
    else:
        if not a.parent_lib:
            ap.error("--parent-lib is required")
        parent(a)
