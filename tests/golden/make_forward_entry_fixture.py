#!/usr/bin/env python3
"""Fixture that pins the host side of the forward solve's entry points of libionode.so (no GPU: nothing is launched).

    python tests/golden/make_forward_entry_fixture.py   ->  tests/golden/forward_entry_checks.json

Recorded from the library of commit 83355a2 ("Fused mean-absolute-error objective with its gradient, all four models"), the last one
whose ionode_capi.hip planned a launch in seven places and reached dopri5_impl by three routes.

(a) plans: for every descriptor of sweep() under every environment of ENVIRONMENTS (the development switches are read per plan) what
    ionode_dense_defer_plan, ionode_dense_tail_plan, ionode_compose_tail_plan (cost_source 0, 1, 2 and 3, which is refused) and
    ionode_compose_plan report: their numbers, or the return code and the ionode_last_error() text.
(b) refusals: for the four solve entry points (ionode_dopri5_objective with either kind) and ionode_protocol_at_outputs, on an HH 2-state
    and an NN-f call, the return code and the ionode_last_error() text of each single defect of defects() and of every unordered pair
    of them that does not set the same field twice.  The pairs pin the PRECEDENCE of the checks.  Every recorded call is one the
    library refuses with IONODE_ERR_ARG or IONODE_ERR_UNSUPPORTED: the pointers are host stand-ins.

The four rows under "null_descriptor" are the ONLY ones not recorded from that commit: there a NULL descriptor on ionode_dopri5,
_deferred, _composed and _objective (kind 0) was dereferenced.  They were recorded from the library that refuses it.  A pair of defects
with a NULL descriptor is recorded where the other defect was already refused ahead of the descriptor's first use.  With --parent the
generator leaves the four calls out and writes the rest (IONODE_LIB selects the library, --out the file): everything but that key
is then byte for byte the committed file.

tests/test_forward_entry_checks.py replays the file with sweep(), plans(), cases() and call() below.  Regenerate only for a change
that is MEANT to move a plan or a check, and then from the library that is being replaced.
"""
import ctypes as C
import importlib
import itertools
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "forward_entry_checks.json")

HH2, MARKOV6, NNF, NND = 0, 1, 2, 3
ARG, UNSUPPORTED = -1, -2
PTR = 0x1000   # any non-null address: nothing is launched

SWITCHES = ("IONODE_TILE_SHRINK", "IONODE_DEFER_DENSE", "IONODE_DEFER_DENSE_CAP", "IONODE_DEFER_TAIL", "IONODE_DEFER_TAIL_RANK",
            "IONODE_COMPOSE")
ENVIRONMENTS = (
    [{}, {"IONODE_TILE_SHRINK": "0"}, {"IONODE_DEFER_DENSE": "0"}]
    + [{"IONODE_DEFER_DENSE_CAP": c} for c in ("1", "2", "8", "100000")]
    + [{"IONODE_DEFER_TAIL": t} for t in ("0", "all")]
    + [{"IONODE_DEFER_TAIL_RANK": r} for r in ("0", "1", "7")]
    + [{"IONODE_DEFER_TAIL": "0", "IONODE_DEFER_TAIL_RANK": "2"}]
    + [{"IONODE_COMPOSE": c} for c in ("0", "pilot", "hint", "1", "")]
)

# ---- (a) plans ----
N_TRAJ = (16, 64, 256, 257, 1024, 1025, 4096, 4097, 8192)
N_OUT = (2, 65, 1000, 20001)
OPTIONS = ("", "sse_out", "launch_order", "traj_per_image", "tile_waves", "launch_order+tile_waves", "nohint")
COLUMNS = ("model", "state_f32", "mlp_width", "n_traj", "n_out", "want_current", "option")


def sweep():
    """The descriptors, as tuples in COLUMNS order: the ones that reach the lean N = 200 16-tile, and enough that do not."""
    nets = [(m, f) for m in (NNF, NND) for f in (0, 1)]
    rows = [(m, f, 200, n, t, w, "") for m, f in nets for n in N_TRAJ for t in N_OUT for w in (0, 1)]
    rows += [(m, f, 200, n, t, w, o) for m, f in nets for n in (1024, 4096, 4097) for t in (65, 20001) for w in (0, 1) for o in OPTIONS[1:]]
    rows += [(NNF, f, 100, n, 1000, w, "") for f in (0, 1) for n in (64, 4096) for w in (0, 1)]
    rows += [(m, f, 0, n, 1000, w, o) for m in (HH2, MARKOV6) for f in (0, 1) for n in (64, 65536) for w in (0, 1) for o in ("", "sse_out")]
    return rows


def plan_desc(capi, row):
    model, f32, N, n_traj, n_out, _want, option = row
    D = 6 if model == MARKOV6 else 2
    d = capi.make_desc(model=model, state_f32=f32, n_state=D, n_out=n_out, n_traj=n_traj, n_prot=1, prot_n=100, mlp_layers=5 if N else 0,
                       mlp_width=N, n_params=12 if D == 6 else 8, prot_dt=0.1, rtol=1e-7, atol=1e-9)
    if option != "nohint":
        d.t_eval_t0_hint, d.t_eval_dt_hint, d.t_eval_exact = 0.0, 0.5, 1
    if option == "sse_out":
        d.sse_ref, d.sse_out = PTR, PTR
    if "launch_order" in option:
        d.launch_order = PTR
    if option == "traj_per_image":
        d.traj_per_image, d.mlp_image_stride = 16, 1 << 40
    if "tile_waves" in option:
        d.tile_waves = 4
    return d


def plans(capi, row):
    """What the four plan queries say of `row` under the current environment: per query its numbers, or [rc, error text]."""
    lib, d, want = capi.lib(), plan_desc(capi, row), row[5]

    def ask(fn, n, ctype, *args):
        out = (ctype * n)()
        rc = fn(C.byref(d), want, *args, C.byref(out))
        return list(out) if rc == 0 else [rc, capi.last_error()]
    return [ask(lib.ionode_dense_defer_plan, 2, C.c_int64), ask(lib.ionode_dense_tail_plan, 2, C.c_int64)] + \
           [ask(lib.ionode_compose_tail_plan, 2, C.c_int64, cs) for cs in (0, 1, 2, 3)] + [ask(lib.ionode_compose_plan, 2, C.c_int32)]


# ---- (b) refusals ----
SOLVES = ("ionode_dopri5", "ionode_dopri5_deferred", "ionode_dopri5_composed", "ionode_dopri5_objective")
PROTOCOL = "ionode_protocol_at_outputs"
# table -> (entry point, objective kind of the complete call)
TABLES = {**{e: (e, 0) for e in SOLVES}, "ionode_dopri5_objective/sae": ("ionode_dopri5_objective", 1), PROTOCOL: (PROTOCOL, 0)}
MODELS = {PROTOCOL: (HH2,)}   # every other table: HH2 and NNF
REQUIRED = ("params", "prot_v", "y0", "t_eval", "y_out", "status")
NULL_DESC = "desc=NULL"


def defects(table, model):
    """[(name, the fields it sets, what)]: the single defects the entry point of `table` can see on a call of `model`.  what: None
    (no descriptor), a dict of descriptor fields, or a dict of arguments under the key "args"."""
    entry, kind = TABLES[table]
    if entry == PROTOCOL:
        return [(NULL_DESC, {"desc"}, None)] + [(f"{p}=NULL", {p}, {"args": {p: None}}) for p in ("prot_v", "t_eval", "v_out")] + \
               [(f"{k}={v}", {k}, {k: v}) for k, v in (("n_out", 0), ("n_prot", 0), ("prot_n", 1), ("prot_dt", 0.0))]
    nn, ws = model == NNF, entry != "ionode_dopri5"
    out = [(NULL_DESC, {"desc"}, None)]
    out += [(f"{p}=NULL", {p}, {"args": {p: None}}) for p in REQUIRED if not (p == "y_out" and kind == 1)]   # sse_out stands in for y_out
    if nn:
        out.append(("mlp_packed=NULL", {"mlp_packed"}, {"args": {"mlp_packed": None}}))
    if kind == 0:
        out += [("sse_out without sse_ref", {"sse_out", "sse_ref"}, {"sse_out": PTR}),
                ("sse_out without hint", {"sse_out", "sse_ref", "t_eval_dt_hint"}, {"sse_out": PTR, "sse_ref": PTR, "t_eval_dt_hint": 0.0}),
                ("sse_out with n_out=1", {"sse_out", "sse_ref", "n_out"}, {"sse_out": PTR, "sse_ref": PTR, "n_out": 1})]
    else:
        out += [("sse_ref=NULL", {"sse_ref"}, {"sse_ref": None}), ("no hint", {"t_eval_dt_hint"}, {"t_eval_dt_hint": 0.0}),
                ("n_out=1", {"n_out"}, {"n_out": 1})]
    out.append(("ckpt with ckpt_cap=0", {"ckpt", "ckpt_cap"}, {"ckpt": PTR, "ckpt_cap": 0}))
    if nn:
        out.append(("launch_order with traj_per_image", {"launch_order", "traj_per_image"},
                    {"launch_order": PTR, "traj_per_image": 16, "mlp_image_stride": 1 << 40}))
    if nn and ws and kind == 0:   # the complete NN-f call defers its dense output (kind 1: a fused objective defers nothing)
        out += [("workspace too small", {"workspace_bytes"}, {"args": {"workspace_bytes": -1}}),
                ("workspace misaligned", {"workspace"}, {"args": {"workspace": 8}})]
    if entry in SOLVES[2:]:
        out.append(("cost_source=9", {"cost_source"}, {"args": {"cost_source": 9}}))
    if entry == SOLVES[3]:
        out += [("objective=2", {"objective"}, {"args": {"objective": 2}}), ("objective=-1", {"objective"}, {"args": {"objective": -1}})]
        out.append(("SAE without sse_out", {"objective", "sse_out", "sse_ref"}, {"args": {"objective": 1}}) if kind == 0 else
                   ("sse_out=NULL", {"sse_out"}, {"sse_out": None}))
    out += [("model=7", {"model"}, {"model": 7}), ("n_state=3", {"n_state"}, {"n_state": 3}), ("n_traj=0", {"n_traj"}, {"n_traj": 0}),
            ("n_params=4", {"n_params"}, {"n_params": 4}), ("rtol=0", {"rtol"}, {"rtol": 0.0}), ("prot_dt=0", {"prot_dt"}, {"prot_dt": 0.0})]
    if nn:
        out += [("mlp_width=0", {"mlp_width"}, {"mlp_width": 0}), ("mlp_width=513", {"mlp_width"}, {"mlp_width": 513}),
                ("mlp_layers=-1", {"mlp_layers"}, {"mlp_layers": -1}), ("tile_waves=3", {"tile_waves"}, {"tile_waves": 3}),
                ("11 layers of width 10", {"mlp_width", "mlp_layers"}, {"mlp_width": 10, "mlp_layers": 11}),
                ("traj_per_image=8", {"traj_per_image"}, {"traj_per_image": 8, "mlp_image_stride": 1 << 40})]
    return out


def refused_before_the_descriptor(table, defect):
    """At the recorded commit: is `defect` refused ahead of the descriptor's first use, whatever else is wrong with the call?"""
    entry, kind = TABLES[table]
    return entry == PROTOCOL or kind == 1 or bool(defect[1] & {"cost_source", "objective"})


def cases(table, model):
    """The rows of (table, model): every single defect, then every unordered pair that sets no field twice.  Without the calls that
    the recorded commit answered by dereferencing NULL; the single ones among them are null_descriptor_cases()."""
    ds = defects(table, model)
    rows = [(d,) for d in ds] + [p for p in itertools.combinations(ds, 2) if not (p[0][1] & p[1][1])]
    return [c for c in rows if c[0][0] != NULL_DESC or (refused_before_the_descriptor(table, c[1]) if len(c) == 2 else
                                                        refused_before_the_descriptor(table, c[0]))]


def null_descriptor_cases():
    """[(table, model, case)]: the NULL descriptor alone on the four solve entry points, kind 0 -- the rows of the soundness fix."""
    return [(t, HH2, (defects(t, HH2)[0],)) for t in SOLVES]


_buf = np.zeros(4096, dtype=np.float64)
_addr = (_buf.ctypes.data + 63) & ~63   # stand-in address, 64-byte aligned: every call returns before anything is dereferenced


def complete_desc(capi, model, kind):
    """The descriptor of the complete call: HH 2-state on 4 trajectories, or NN-f on the lean N = 200 16-tile (which defers)."""
    if model == NNF:
        kw = dict(model=NNF, n_state=2, n_out=2000, n_traj=2048, n_prot=1, prot_n=10, mlp_layers=5, mlp_width=200, n_params=8, prot_dt=1.0)
    else:
        kw = dict(model=HH2, n_state=2, n_out=8, n_traj=4, n_prot=2, prot_n=16, n_params=8, prot_dt=1.0)
    kw.update(rtol=1e-7, atol=1e-9, v_oob=-80.0, obs_g=1.0, obs_e=-86.0, t_eval_t0_hint=0.0, t_eval_dt_hint=0.5, t_eval_exact=1)
    if kind == 1:
        kw.update(sse_ref=PTR, sse_out=PTR)
    return kw


def call(capi, table, model, case):
    """(rc, ionode_last_error()) of the table's entry point with the defects of `case` applied to an otherwise complete call."""
    entry, kind = TABLES[table]
    lib, fields = capi.lib(), complete_desc(capi, model, kind)
    ws_bytes = capi.dense_defer_plan(capi.make_desc(**fields), False)["workspace_bytes"] if entry in SOLVES[1:] else 0
    assert (ws_bytes > 0) == (model == NNF and kind == 0 and entry in SOLVES[1:]), (table, model, ws_bytes)
    args = {p: _addr for p in REQUIRED + ("prot_v", "t_eval", "v_out")}
    args.update(mlp_packed=_addr if model == NNF else None, workspace=_addr if ws_bytes else None, workspace_bytes=ws_bytes, cost_source=0,
                objective=kind)
    no_desc = False
    for _name, _fields, what in case:
        if what is None:
            no_desc = True
            continue
        for k, v in what.get("args", {}).items():
            args[k] = v if (v is None or k in ("cost_source", "objective")) else args[k] + v   # workspace: an offset
        fields.update({k: v for k, v in what.items() if k != "args"})
    d = None if no_desc else C.byref(capi.make_desc(**fields))
    p = lambda n: None if args[n] is None else C.c_void_p(args[n])
    if entry == PROTOCOL:
        rc = lib.ionode_protocol_at_outputs(d, p("prot_v"), None, p("t_eval"), p("v_out"), None)
    else:
        tail = ((), (p("workspace"), args["workspace_bytes"]), (p("workspace"), args["workspace_bytes"], args["cost_source"]),
                (p("workspace"), args["workspace_bytes"], args["cost_source"], args["objective"]))[SOLVES.index(entry)]
        rc = getattr(lib, entry)(d, p("mlp_packed"), p("params"), p("prot_v"), None, None, p("y0"), p("t_eval"), p("y_out"), None, p("status"),
                                 None, None, *tail)
    return rc, capi.last_error()


def clear_switches():
    for k in SWITCHES:
        os.environ.pop(k, None)


def _lines(items, per):
    return ",\n".join("    " + ", ".join(items[j:j + per]) for j in range(0, len(items), per))


def main():
    sys.path.insert(0, ROOT)
    import torch
    assert not torch.cuda.is_available(), "record on a machine without a HIP device: the pointers are host addresses"
    parent = "--parent" in sys.argv
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else OUT
    capi = importlib.import_module("neural-ode-ion-channels_amd").capi
    clear_switches()
    messages = []

    def msg_index(m):
        if m not in messages:
            messages.append(m)
        return messages.index(m)

    # (a): unique answers, and per environment the answer of every descriptor
    answers, per_env, rows = [], [], sweep()
    for env in ENVIRONMENTS:
        clear_switches()
        os.environ.update(env)
        idx = []
        for row in rows:
            a = [q if len(q) == 2 and not isinstance(q[1], str) else [q[0], "e", msg_index(q[1])] for q in plans(capi, row)]
            assert all(len(q) == 2 or q[0] in (ARG, UNSUPPORTED) for q in a), (env, row, a)
            a = json.dumps(a, separators=(",", ":"))
            if a not in answers:
                answers.append(a)
            idx.append(answers.index(a))
        per_env.append(idx)
    clear_switches()
    # (b)
    tables, n = {}, 0
    for table in TABLES:
        for model in MODELS.get(table, (HH2, NNF)):
            names = [d[0] for d in defects(table, model)]
            trows = []
            for case in cases(table, model):
                rc, msg = call(capi, table, model, case)
                assert rc in (ARG, UNSUPPORTED), (table, model, [d[0] for d in case], rc, msg)   # refused, never launched
                ij = [names.index(d[0]) for d in case]
                trows.append(ij + [-1] * (2 - len(ij)) + [rc, msg_index(msg)])
            tables[f"{table}:{model}"] = {"defects": names, "rows": trows}
            n += len(trows)
    null_rows = []
    if not parent:
        for table, model, case in null_descriptor_cases():
            rc, msg = call(capi, table, model, case)
            assert rc == ARG, (table, rc, msg)
            null_rows.append([table, rc, msg])
    with open(out_path, "w") as f:   # plans: one line per environment; refusals: [defect, second defect or -1, rc, message], eight per line
        f.write('{\n "commit": "83355a2",\n "null_descriptor": %s,\n "messages": [\n' % json.dumps(null_rows))
        f.write(",\n".join("  " + json.dumps(m) for m in messages) + "\n ],\n")
        f.write(' "plan_columns": %s,\n "plan_queries": ["dense_defer", "dense_tail", "compose_tail/0", "compose_tail/1", "compose_tail/2", '
                '"compose_tail/3", "compose"],\n "plan_answers": [\n' % json.dumps(list(COLUMNS)))
        f.write(",\n".join("  " + a for a in answers) + "\n ],\n \"plans\": [\n")
        f.write(",\n".join('  {"env": %s, "answers": [\n%s\n  ]}' % (json.dumps(e), _lines([str(i) for i in idx], 40))
                           for e, idx in zip(ENVIRONMENTS, per_env)) + "\n ],\n \"tables\": {\n")
        blocks = []
        for k, v in tables.items():
            items = [json.dumps(r, separators=(",", ":")) for r in v["rows"]]
            blocks.append('  "%s": {\n   "defects": %s,\n   "rows": [\n%s\n   ]\n  }' % (k, json.dumps(v["defects"]), _lines(items, 8)))
        f.write(",\n".join(blocks) + "\n }\n}\n")
    json.load(open(out_path))
    print(len(rows), "descriptors x", len(ENVIRONMENTS), "environments,", len(answers), "answers,", n, "refusals,", len(messages), "messages,",
          os.path.getsize(out_path), "bytes ->", out_path)
    assert os.path.getsize(out_path) < 300 * 1024


if __name__ == "__main__":
    main()
