"""Dev tool: where the lean N = 200 16-tile's attempts ran -- on its own net or, once <= 4 of a tile's trajectories were live, on the
4-trajectory net (MlpShrink4, ionode_mlp_tile4.hpp) -- read from the step log of the diagnostic build:

  tools/build_variant.sh stamps -DIONODE_STAMPS
  IONODE_LIB=neural-ode-ion-channels_amd/variants/stamps/libionode.so python tools/tile_shrink_stamps.py [--batch 4096] [--nt 100001]

The headline workload of bench.py (NN-f s00, sine-wave protocols, fp64 state, current trace), forced onto the 16-tile.  Prints one JSON
line: the attempts of every tile on MlpShrink4 (summary), and for tile 0 (wavefront 0) the cycles per evaluation (attempt / 6) on each
net.  IONODE_TILE_SHRINK=0 in the environment turns the switch off (every tile then reports 0 shrunk attempts).
"""
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
    ap.add_argument("--clock-ghz", type=float, default=2.4, help="shader clock for the cycles -> us conversion (s_memtime counts it)")
    args = ap.parse_args()
    import bench
    ion = importlib.import_module("neural-ode-ion-channels_amd")
    protocols = importlib.import_module("neural-ode-ion-channels_amd.protocols")
    capi = ion.capi
    dev = torch.device("cuda:0")
    B, Nt = args.batch, args.nt
    w, _ = bench.load_weights()
    packed = torch.from_numpy(capi.mlp_pack(w, bench.MLP_L, bench.MLP_N)).to(dev)
    pv = protocols.sinewave(protocols.sinewave_scales(0, B), n_samples=Nt, dt=0.1, xp=torch, device=dev)
    params = torch.from_numpy(np.tile(bench.P_HH, (B, 1))).to(dev)
    y0 = torch.tensor([[0.0, 1.0]], dtype=torch.float64, device=dev).repeat(B, 1).contiguous()
    te = torch.arange(Nt, dtype=torch.float64, device=dev) * 0.1
    tiles = (B + 15) // 16
    rows = (64 + tiles + 3) // 4
    slog = torch.zeros((rows, 4), dtype=torch.float64, device=dev)
    r = capi.dopri5(capi.MODEL_NNF, params, pv, y0, te, mlp_packed=packed, mlp_layers=bench.MLP_L, mlp_width=bench.MLP_N,
                    prot_t0=0.0, prot_dt=0.1, current=True, tile_waves=4, t_eval_hint=(0.0, 0.1), step_log=slog)
    torch.cuda.synchronize()
    kernel = ion.capi.lib().ionode_last_kernel_name().decode()
    s = slog.cpu().numpy().reshape(-1)
    shr = s[64:64 + tiles]
    att = r["stats"][:, 0].cpu().numpy() + r["stats"][:, 1].cpu().numpy()
    tile_max = np.array([att[16 * t:16 * t + 16].max() for t in range(tiles)])
    c16, n16, c4, n4 = s[32:36]
    per_eval = lambda c, n: float(c / (6 * n)) if n > 0 else None
    us = lambda c: None if c is None else round(c / (args.clock_ghz * 1e3), 3)
    out = {
        "kernel": kernel, "tile_shrink": os.environ.get("IONODE_TILE_SHRINK", "default"), "tiles": tiles,
        "tiles_shrunk": int((shr > 0).sum()),
        "shrunk_attempts": {"sum": int(shr.sum()), "mean": round(float(shr.mean()), 1), "max": int(shr.max())},
        "shrunk_share_of_tile_attempts": round(float((shr / tile_max).mean()), 4),
        "tile0": {"attempts_sorted": sorted(att[:16].astype(int).tolist(), reverse=True), "attempts_16": int(n16), "attempts_4": int(n4),
                  "cycles_per_eval_16": per_eval(c16, n16), "cycles_per_eval_4": per_eval(c4, n4),
                  "us_per_eval_16": us(per_eval(c16, n16)), "us_per_eval_4": us(per_eval(c4, n4))},
    }
    print(json.dumps(out))


if __name__ == "__main__":
    main()
