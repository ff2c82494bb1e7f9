"""Dev tool, CPU only: replay the shrink-aware tile composition on a file of attempt counts and print the table of DESIGN.md 5.2.

  python tools/compose_replay.py [counts.npy] [--cost name=file.npy ...] [--e16-us 14.7] [--e4-us 10.1]

counts.npy: int [B, 2] accepted / rejected step attempts per trajectory (default tests/golden/headline_attempts.npy, the headline's own
4096 trajectories from the oracle: tests/golden/make_headline_attempts.py).  A tile steps its 16 slots in lock step, six evaluations of
the net per attempt, and finishes on the 4-trajectory net once <= 4 of them are live:

    T_tile = A5 * 6 e16 + (A1 - A5) * 6 e4        A1, A5: largest, fifth-largest attempt count of the tile's trajectories

The launch lasts as long as its slowest tile.  Rows: index order, the composition (libionode.so's host mirror of the rule) with the exact
counts as cost, with every --cost file (fp64 or int [B]: a pilot's RHS evaluations read back from the GPU, say), with the protocol's
total variation (--protocol-tv) or with the CPU oracle's HH 2-state pilot (--pilot; both generate the headline's protocols, a minute
of numpy), and H = 1 .. 6 heavies per tile for
comparison.  `margin` counts the tiles that end at least --margin-ms before the last (profiles/defer_tail.md: twice the slowest
in-kernel expansion), the gate of the solve kernel's tail.
"""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def tile_ms(attempts, order, e16_us, e4_us):
    out = []
    for s in range(0, len(order), 16):
        a = np.sort(attempts[order[s:s + 16]])[::-1].astype(np.float64)
        a5 = a[4] if len(a) > 4 else 0.0
        out.append((a5 * 6 * e16_us + (a[0] - a5) * 6 * e4_us) * 1e-3)
    return np.array(out)


def compose_h(cost, H):
    """The rule with H heavies per tile instead of 4 (comparison only; full tiles)."""
    B = len(cost)
    NT = B // 16
    s = np.lexsort((np.arange(B), -np.asarray(cost, dtype=np.float64)))
    heavy, light = s[:H * NT], s[H * NT:][::-1]
    return np.concatenate([np.concatenate([heavy[H * k:H * k + H], light[(16 - H) * k:(16 - H) * (k + 1)]]) for k in range(NT)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("counts", nargs="?", default=os.path.join(ROOT, "tests", "golden", "headline_attempts.npy"))
    ap.add_argument("--cost", action="append", default=[], metavar="NAME=FILE")
    ap.add_argument("--protocol-tv", action="store_true")
    ap.add_argument("--pilot", action="store_true", help="pilot costs from the CPU oracle (HH 2-state, the headline's protocols), rtol 1e-7 and 1e-4")
    ap.add_argument("--e16-us", type=float, default=14.7)
    ap.add_argument("--e4-us", type=float, default=10.1)
    ap.add_argument("--margin-ms", type=float, default=17.7)
    args = ap.parse_args()
    capi = importlib.import_module("neural-ode-ion-channels_amd").capi
    ar = np.load(args.counts)
    att = ar.sum(axis=1).astype(np.int64)
    B = len(att)
    print(f"{B} trajectories: mean {att.mean():.1f} attempts, max {att.max()}, cv {att.std() / att.mean() * 100:.1f} %, "
          f"rejected {ar[:, 1].sum() / att.sum() * 100:.0f} %")
    rows = [("index order", np.arange(B)), ("4 heaviest + 12 lightest, exact attempt counts", capi.compose_order_host(att))]
    for spec in args.cost:
        name, path = spec.split("=", 1)
        rows.append((f"same, cost = {name}", capi.compose_order_host(np.load(path).astype(np.float64).reshape(-1))))
    if args.pilot:
        from oracle import oracle
        import bench
        protocols = importlib.import_module("neural-ode-ion-channels_amd.protocols")
        for rtol, atol in ((1e-7, 1e-9), (1e-4, 1e-6)):
            st = np.concatenate([oracle.solve(oracle.MODEL_HH2, np.tile(bench.P_HH, (256, 1)), protocols.sinewave(protocols.sinewave_scales(b, 256)),
                                              [0.0, 1.0], [0.0, 10000.0], prot_t0=0.0, prot_dt=0.1, rtol=rtol, atol=atol)["stats"] for b in range(0, B, 256)])
            rows.append((f"same, cost = HH 2-state pilot at rtol {rtol:g} / atol {atol:g} ({st[:, :2].sum(axis=1).mean():.0f} attempts)",
                         capi.compose_order_host(st[:, 2])))
    if args.protocol_tv:
        protocols = importlib.import_module("neural-ode-ion-channels_amd.protocols")
        tv = np.concatenate([np.abs(np.diff(protocols.sinewave(protocols.sinewave_scales(b, 256)), axis=1)).sum(axis=1) for b in range(0, B, 256)])
        rows.append(("same, cost = total variation of the protocol", capi.compose_order_host(tv)))
    if B % 16 == 0:
        rows += [(f"H = {H} heavies per tile, exact counts", compose_h(att, H)) for H in (1, 2, 3, 5, 6)]
    print("| composition | tile time min / median / max (ms) | tiles ending >= %.1f ms before the last |" % args.margin_ms)
    print("|---|---|---|")
    res = {}
    for name, order in rows:
        t = tile_ms(att, np.asarray(order), args.e16_us, args.e4_us)
        res[name] = float(t.max())
        print(f"| {name} | {t.min():.1f} / {np.median(t):.1f} / **{t.max():.1f}** | {int((t <= t.max() - args.margin_ms).sum())} |")
    print(json.dumps({"max_ms": res, "composed_over_index": res[rows[1][0]] / res[rows[0][0]]}))


if __name__ == "__main__":
    main()
