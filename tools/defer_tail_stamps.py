"""Dev tool: when every tile of the lean N = 200 16-tile ends, and what its in-kernel expansion of the deferred dense output costs --
read from the step log of the diagnostic build (100 MHz wall clock, three stamps per tile behind the per-tile block):

  tools/build_variant.sh stamps -DIONODE_STAMPS
  IONODE_DEFER_TAIL=all IONODE_LIB=neural-ode-ion-channels_amd/variants/stamps/libionode.so python tools/defer_tail_stamps.py

The headline workload of bench.py (NN-f s00, sine-wave protocols, fp64 state, current trace), forced onto the 16-tile.  Prints one JSON
line: the tiles' finish times relative to the first tile's start (quantiles), the per-tile expansion times, and the gate rule of
profiles/defer_tail.md -- the largest fraction of the tiles (in eighths) whose last member still ends at least twice the slowest
expansion before the last tile does.  Under IONODE_DEFER_TAIL=0 no stamp is written (the tail is not entered)."""
import argparse
import importlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--nt", type=int, default=100001)
    ap.add_argument("--uniform-scale", action="store_true", help="one protocol scale set for every trajectory: all tiles end together")
    ap.add_argument("--compose", choices=("none", "exact", "pilot"), default="none",
                    help="tile composition of the stamped launch (capi.dopri5 cost_hint): index order, the RHS evaluations of a first "
                         "solve of the same batch as cost, or the pilot")
    args = ap.parse_args()
    import bench
    ion = importlib.import_module("neural-ode-ion-channels_amd")
    protocols = importlib.import_module("neural-ode-ion-channels_amd.protocols")
    capi = ion.capi
    dev = torch.device("cuda:0")
    B, Nt = args.batch, args.nt
    w, _ = bench.load_weights()
    packed = torch.from_numpy(capi.mlp_pack(w, bench.MLP_L, bench.MLP_N)).to(dev)
    scales = protocols.sinewave_scales(0, B)
    if args.uniform_scale:
        scales = np.repeat(scales[:1], B, axis=0)
    pv = protocols.sinewave(scales, n_samples=Nt, dt=0.1, xp=torch, device=dev)
    params = torch.from_numpy(np.tile(bench.P_HH, (B, 1))).to(dev)
    y0 = torch.tensor([[0.0, 1.0]], dtype=torch.float64, device=dev).repeat(B, 1).contiguous()
    te = torch.arange(Nt, dtype=torch.float64, device=dev) * 0.1
    tiles = (B + 15) // 16
    rows = (64 + 4 * tiles + 3) // 4
    slog = torch.zeros((rows, 4), dtype=torch.float64, device=dev)
    kw = dict(mlp_packed=packed, mlp_layers=bench.MLP_L, mlp_width=bench.MLP_N, prot_t0=0.0, prot_dt=0.1, current=True, tile_waves=4,
              t_eval_hint=(0.0, 0.1))
    hint = {"none": None, "exact": "hint", "pilot": "pilot"}[args.compose]
    prev = {}
    if args.compose == "exact":
        first = capi.dopri5(capi.MODEL_NNF, params, pv, y0, te, step_log=torch.zeros_like(slog), cost_hint=None, **kw)
        prev = {k: first[k] for k in ("y", "i", "status", "stats")}
    r = capi.dopri5(capi.MODEL_NNF, params, pv, y0, te, step_log=slog, cost_hint=hint, out=prev, **kw)
    torch.cuda.synchronize()
    s = slog.cpu().numpy().reshape(-1)[64 + tiles:64 + 4 * tiles].reshape(tiles, 3)
    tail = capi.compose_tail_plan(r["desc"], True, r["composed"])
    out = {"kernel": capi.lib().ionode_last_kernel_name().decode(), "tiles": tiles, "tail": tail,
           "switch": os.environ.get("IONODE_DEFER_TAIL", "default"), "compose": args.compose, "composed": r["composed"]}
    if s[:, 0].max() > 0:
        ms = lambda ticks: ticks / 1e5   # 100 MHz
        t0 = s[:, 0].min()
        fin = np.sort(ms(s[:, 1] - t0))
        end = ms(s[:, 2] - t0)
        exp = ms(s[:, 2] - s[:, 1])
        q = lambda a: {k: round(float(np.quantile(a, p)), 3) for k, p in (("min", 0), ("q25", .25), ("q50", .5), ("q75", .75), ("q875", .875), ("max", 1))}
        last, slow = float(fin[-1]), float(exp.max())
        with_margin = int((fin <= last - 2 * slow).sum())
        out.update({"start_spread_ms": round(float(ms(s[:, 0].max() - t0)), 3), "finish_ms": q(fin), "launch_end_ms": round(float(end.max()), 3),
                    "expand_ms": q(exp), "expand_sum_ms": round(float(exp.sum()), 1), "tiles_with_2x_margin": with_margin,
                    "gate_eighths": int(8 * with_margin // tiles), "finish_by_eighth_ms": [round(float(fin[min(tiles - 1, tiles * k // 8)]), 2) for k in range(1, 9)]})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
