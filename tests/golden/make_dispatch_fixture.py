#!/usr/bin/env python3
"""Fixture that pins the dispatcher and the weight packer of libionode.so (no GPU: nothing is launched).

    python tests/golden/make_dispatch_fixture.py   ->  tests/golden/dispatch_table.json

(a) a descriptor sweep: for every descriptor of sweep() the return code and the numbers of ionode_launch_geometry, the name
    ionode_kernel_name reports, and (on an error) the first 60 characters of ionode_last_error;
(b) the SHA-256 and the length of ionode_mlp_pack's image for seeded weights of the shapes in PACK_SHAPES.

tests/test_host_logic.py::test_dispatch_table_and_images_are_pinned replays both with replay_row() / pack_digest() below.  Regenerate
only for a change that is MEANT to move a dispatch decision, a launch geometry, an error message or a packed image.
"""
import hashlib
import importlib
import json
import os
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "dispatch_table.json")

HH2, MARKOV6, NNF, NND = 0, 1, 2, 3
N_TRAJ = (1, 4, 16, 64, 256, 257, 1024, 1025, 4096, 8191, 8192, 24576, 32768, 32769, 49152, 65536)
N_TRAJ_FEW = (64, 1024, 4096, 65536)       # the batch sizes that tile_waves / traj_per_image are paired with
WIDTHS = (1, 10, 16, 17, 64, 100, 200, 201, 500, 512, 513)
LAYERS = (0, 1, 5, 6, 7, 10, 11, 15, 16)
TILE_WAVES = (0, 1, 2, 4, 8, 16, 64)
TRAJ_PER_IMAGE = (0, 4, 16, 32, 64)
# the contract axis: what the caller asks for beyond the states (the lean variants serve only the first)
CONTRACTS = ("lean", "nohint", "step_log", "ckpt", "v_at_outputs", "sse_out")
COLUMNS = ("model", "state_f32", "n_traj", "mlp_width", "mlp_layers", "tile_waves", "traj_per_image", "contract")
PACK_SHAPES = ((0, 10), (5, 10), (3, 16), (2, 17), (1, 64), (5, 100), (5, 200), (10, 200), (1, 300), (2, 500))
PTR = 0x1000   # any non-null address: nothing is launched


def sweep():
    """The descriptors, as tuples in COLUMNS order.  The full product of the axes has ~10^6 members; this is a union of slices
    through it, each of which varies the axes that one dispatch decision reads (every row is a member of the full product)."""
    rows = []
    for model in (HH2, MARKOV6):          # closed-form models: no MLP axes
        for f32 in (0, 1):
            rows += [(model, f32, n, 0, 0, 0, 0, "lean") for n in N_TRAJ]
            rows += [(model, f32, n, 0, 0, 0, 0, c) for n in (4096, 65536) for c in CONTRACTS]
            rows += [(model, f32, n, 0, 0, tw, 0, c) for n in (64, 65536) for tw in (4, 16, 64) for c in ("lean", "sse_out")]
    # NN-f, fp64 state: batch size x width (the tile-size thresholds of every width) ...
    rows += [(NNF, 0, n, N, 5, 0, 0, "lean") for n in N_TRAJ for N in WIDTHS]
    # ... the contract of every net kind, with and without hidden layers ...
    rows += [(NNF, 0, n, N, L, 0, 0, c) for n in (64, 65536) for N in (10, 16, 64, 100, 200, 500) for L in (0, 5) for c in CONTRACTS]
    # ... depth: the resident-weights limit of N <= 16, the one-trajectory tile's two forms, the run-time-width tile ...
    rows += [(NNF, 0, n, N, L, 0, 0, "lean") for n in (1, 4096) for N in (10, 16, 200, 201, 512) for L in LAYERS]
    # ... forced tile forms x weight-image granularity
    rows += [(NNF, 0, n, N, 5, tw, tpi, "lean") for n in (64, 65536) for N in (10, 200) for tw in TILE_WAVES for tpi in TRAJ_PER_IMAGE]
    rows += [(NNF, 0, 4096, N, 5, tw, tpi, "lean") for N in (16, 64, 100, 500) for tw in TILE_WAVES for tpi in (0, 16)]
    rows += [(NNF, 0, 64, 200, 10, tw, tpi, "nohint") for tw in TILE_WAVES for tpi in TRAJ_PER_IMAGE]
    # the other three (model, state type) tables: every variant once more
    for model, f32 in ((NNF, 1), (NND, 0), (NND, 1)):
        rows += [(model, f32, n, N, 5, 0, 0, c) for n in N_TRAJ_FEW for N in (10, 16, 64, 100, 200, 500) for c in ("lean", "nohint", "sse_out")]
    for model in (NNF, NND):
        for f32 in (0, 1):   # the one-trajectory tile for deep stacks
            rows += [(model, f32, 64, 200, L, 0, 0, c) for L in (7, 15) for c in ("lean", "nohint")]
    seen, out = set(), []
    for r in rows:
        if r not in seen:
            seen.add(r)
            out.append(r)
    return out


def make_desc(capi, row):
    model, f32, n_traj, N, L, tw, tpi, contract = row
    D = 6 if model == MARKOV6 else 2
    d = capi.make_desc(model=model, state_f32=f32, n_state=D, n_out=10, n_traj=n_traj, n_prot=1, prot_n=100, mlp_layers=L, mlp_width=N,
                       n_params=12 if D == 6 else 8, prot_dt=0.1, rtol=1e-7, atol=1e-9, tile_waves=tw)
    if tpi:
        d.traj_per_image, d.mlp_image_stride = tpi, 1 << 40
    if contract != "nohint":
        d.t_eval_t0_hint, d.t_eval_dt_hint, d.t_eval_exact = 0.0, 0.5, 1
    if contract == "step_log":
        d.step_log, d.step_log_cap = PTR, 64
    elif contract == "ckpt":
        d.ckpt, d.ckpt_cap = PTR, 8
    elif contract == "v_at_outputs":
        d.v_at_outputs = PTR
    elif contract == "sse_out":
        d.sse_ref, d.sse_out = PTR, PTR
    return d


def replay_row(capi, row):
    """(rc, [grid, block, lds_bytes, tile_waves] or None, kernel name, error text or "")"""
    import ctypes as C
    d = make_desc(capi, row)
    geo = (C.c_int32 * 4)()
    rc = capi.lib().ionode_launch_geometry(C.byref(d), C.byref(geo))
    err = capi.last_error()[:60] if rc != 0 else ""
    return rc, (list(geo) if rc == 0 else None), capi.kernel_name(d), err


def pack_digest(capi, L, N):
    """(floats, sha256) of the packed image of the seeded weights of shape (L, N)"""
    n = 2 * N + N + L * (N * N + N) + N + 1
    w = np.random.default_rng(L * 1000 + N).standard_normal(n).astype(np.float32)
    img = capi.mlp_pack(w, L, N)
    assert img.size == capi.lib().ionode_mlp_packed_floats(L, N)
    return int(img.size), hashlib.sha256(img.tobytes()).hexdigest()


def main():
    sys.path.insert(0, ROOT)
    capi = importlib.import_module("neural-ode-ion-channels_amd").capi
    names, errors, table = [""], [""], []
    for row in sweep():
        rc, geo, name, err = replay_row(capi, row)
        for lst, x in ((names, name), (errors, err)):
            if x not in lst:
                lst.append(x)
        table.append(list(row[:7]) + [CONTRACTS.index(row[7]), rc, names.index(name), errors.index(err)] + (geo or []))
    # every compiled variant is reached at least once: the tables' name strings are literals of the library
    compiled = set(re.findall(rb"ionode_dopri5_kernel<[0-9a-z, ]+>", open(capi.LIB_PATH, "rb").read()))
    compiled = {c.decode() for c in compiled}
    assert len(compiled) == 24 + 4 * 21, len(compiled)   # the closed table + IONODE_MLP_VARIANTS for two models x two state types
    missing = compiled - set(names)
    assert not missing, sorted(missing)
    assert len(table) <= 4000, len(table)
    packs = [[L, N, *pack_digest(capi, L, N)] for L, N in PACK_SHAPES]
    # four descriptor rows per line (a compact file whose diff still points at the rows that moved), keys sorted
    doc = {
        "columns": list(COLUMNS) + ["rc", "kernel", "error", "grid", "block", "lds_bytes", "waves"],
        "contracts": list(CONTRACTS),
        "errors": errors,
        "kernels": names,
        "packs": packs,
        "packs_columns": ["mlp_layers", "mlp_width", "floats", "sha256"],
        "rows": table,
    }
    with open(OUT, "w") as f:
        f.write("{\n")
        for i, k in enumerate(sorted(doc)):
            v = doc[k]
            if k in ("rows", "packs", "kernels", "errors"):
                items = [json.dumps(r, separators=(",", ":")) for r in v]
                per = 4 if k == "rows" else 1
                body = "[\n" + ",\n".join("  " + ", ".join(items[j:j + per]) for j in range(0, len(items), per)) + "\n ]"
            else:
                body = json.dumps(v)
            f.write(' "%s": %s%s\n' % (k, body, "," if i + 1 < len(doc) else ""))
        f.write("}\n")
    json.load(open(OUT))
    print(len(table), "rows,", len(names) - 1, "kernels,", len(errors) - 1, "error texts,", os.path.getsize(OUT), "bytes ->", OUT)
    assert os.path.getsize(OUT) < 300 * 1024


if __name__ == "__main__":
    main()
