#!/usr/bin/env python3
"""Fixture that pins how grad._Solve.backward cuts a sweep into chunk launches (no GPU, no library: integer arithmetic).

    python tests/golden/make_grad_chunk_plans.py   ->  tests/golden/grad_chunk_plans.json

reference_plan() below is the chunk arithmetic of _Solve.backward as it stood BEFORE it became grad.plan_backward_chunks -- the
statements lifted unchanged, in their order, with a tag appended per branch taken -- so the table records the old decisions, not the
new function's output.  tests/test_host_logic.py::test_backward_chunk_plans_are_pinned replays every row through
grad.plan_backward_chunks with digest() and asserts that every tag of BRANCHES occurs.  Regenerate only for a change that is MEANT to
move a chunking decision, and then from the arithmetic that is being replaced.
"""
import hashlib
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "grad_chunk_plans.json")

MAX_RECOMPUTE_ITERS = 65535 * 4
PACKET_DOUBLES = 16 * 64                              # ionode_grad_packet_doubles()
RECORD_FLOATS = (2 * 2 * 1 * 256 + 64, 2 * 6 * 13 * 256 + 64)   # ionode_grad_record_floats: (L, N) = (1, 10) and (5, 200)
N_ITER = (1, 2, 255, 256, 257, 65535 * 4 - 1, 65535 * 4, 65535 * 4 + 1)
TILES = (1, 4096)
BUDGETS = ("fits", "two_chunks", "one_iteration", "too_small")
COLUMNS = ("need_w", "two_phase", "n_iter", "tiles", "record_floats", "budget")
# every branch of the old code: the first cut (with / without records), the grid.y clamp where it binds, the second buffer and the
# halved budget, the clamp binding again there, the packet-bound chunks (one buffer / two), and no buffering at all
BRANCHES = ("first:records", "first:whole", "clamp", "double:records", "double:clamp", "packets:1", "packets:2", "single")


def reference_plan(n_iter, tiles, recf, pkd, budget, need_w, two_phase):
    """(chunk, n_buf, bounds, tags): the parent's statements; `lib.ionode_grad_packet_doubles()` is `pkd`."""
    tags = []
    chunk = n_iter if not need_w else max(1, min(n_iter, budget // (tiles * 6 * recf * 4)))
    tags.append("first:records" if need_w else "first:whole")
    if two_phase:
        if chunk > MAX_RECOMPUTE_ITERS:
            tags.append("clamp")
        chunk = min(chunk, MAX_RECOMPUTE_ITERS)
    n_chunks = (n_iter + chunk - 1) // chunk
    n_buf = 2 if (n_chunks > 1 and (need_w or two_phase)) else 1
    if need_w and n_buf == 2:
        tags.append("double:records")
        chunk = max(1, min(n_iter, (budget // 2) // (tiles * 6 * recf * 4)))
        if two_phase:
            if chunk > MAX_RECOMPUTE_ITERS:
                tags.append("double:clamp")
            chunk = min(chunk, MAX_RECOMPUTE_ITERS)
        n_chunks = (n_iter + chunk - 1) // chunk
    elif two_phase and not need_w:
        per_it = tiles * int(pkd) * 8
        chunk = max(1, min(n_iter, 256, (budget // 2) // per_it))
        n_chunks = (n_iter + chunk - 1) // chunk
        n_buf = 2 if n_chunks > 1 else 1
        tags.append("packets:%d" % n_buf)
    else:
        tags.append("single")
    bounds = [(it0, min(n_iter, it0 + chunk)) for it0 in range(0, n_iter, chunk)]
    assert len(bounds) == n_chunks
    return chunk, n_buf, bounds, tags


def budget_bytes(kind, n_iter, tiles, recf, need_w):
    """The four budget cases, in units of what one iteration holds (records with weight gradients, packets without)."""
    per_it = tiles * 6 * recf * 4 if need_w else tiles * PACKET_DOUBLES * 8
    return {"fits": 4 * per_it * n_iter,                 # the whole sweep, also at half the budget
            "two_chunks": per_it * ((n_iter + 1) // 2),  # the first cut makes exactly two chunks (n_iter > 1)
            "one_iteration": 2 * per_it,                 # half the budget holds one iteration
            "too_small": per_it // 3}[kind]              # not even one: chunk clamps to 1


def rows():
    out = []
    for need_w in (False, True):
        for two_phase in (False, True):
            for n_iter in N_ITER:
                for tiles in TILES:
                    for recf in (RECORD_FLOATS if need_w else (0,)):   # (without weight gradients the caller passes 0)
                        for kind in BUDGETS:
                            out.append((need_w, two_phase, n_iter, tiles, recf, budget_bytes(kind, n_iter, tiles, recf or RECORD_FLOATS[0], need_w)))
    # the clamp of the halved budget: more than two grid.y limits of iterations, a budget that would hold half of them at once
    n = 3 * MAX_RECOMPUTE_ITERS
    out.append((True, True, n, 1, RECORD_FLOATS[0], 1 * 6 * RECORD_FLOATS[0] * 4 * (n - 1)))
    return out


def digest(chunk, n_buf, bounds):
    """What the table keeps of a plan: the bounds as count, ends and a hash (one iteration per chunk makes 262 141 of them)."""
    b = np.asarray(bounds, dtype="<i8").reshape(-1, 2)
    return {"chunk": chunk, "n_buf": n_buf, "n_chunks": len(b), "head": b[:2].tolist(), "tail": b[-2:].tolist(),
            "sha1": hashlib.sha1(b.tobytes()).hexdigest()}   # of the [n_chunks][2] little-endian int64 array


def main():
    table = []
    for r in rows():
        need_w, two_phase, n_iter, tiles, recf, budget = r
        chunk, n_buf, bounds, tags = reference_plan(n_iter, tiles, recf, PACKET_DOUBLES, budget, need_w, two_phase)
        table.append({"in": list(r), "tags": tags, "plan": digest(chunk, n_buf, bounds)})
    seen = {t for row in table for t in row["tags"]}
    assert seen == set(BRANCHES), sorted(set(BRANCHES) ^ seen)
    with open(OUT, "w") as f:
        json.dump({"columns": COLUMNS, "packet_doubles": PACKET_DOUBLES, "branches": BRANCHES, "rows": table}, f, separators=(",", ":"))
        f.write("\n")
    print(f"{OUT}: {len(table)} rows")


if __name__ == "__main__":
    main()
