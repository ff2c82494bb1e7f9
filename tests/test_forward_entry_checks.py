"""CPU tests of the forward solve's entry points' host side, pinned by tests/golden/forward_entry_checks.json
(tests/golden/make_forward_entry_fixture.py): what the four plan queries report under every development switch, and what the four
solve entry points and ionode_protocol_at_outputs refuse, in which order.  Nothing is launched."""
import importlib.util
import json
import os

import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture(scope="module")
def gen():
    spec = importlib.util.spec_from_file_location("make_forward_entry_fixture", os.path.join(GOLDEN, "make_forward_entry_fixture.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def doc():
    return json.load(open(os.path.join(GOLDEN, "forward_entry_checks.json")))


def _set_switches(monkeypatch, gen, env):
    for k in gen.SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def test_plans_under_every_development_switch_are_pinned(ion, gen, doc, monkeypatch):
    """Defer, tail, composed-tail (cost_source 0 .. 3) and compose plan of every descriptor of the sweep, per environment."""
    rows = gen.sweep()
    assert [p["env"] for p in doc["plans"]] == gen.ENVIRONMENTS and doc["plan_columns"] == list(gen.COLUMNS)
    answers = [[q if len(q) == 2 else [q[0], doc["messages"][q[2]]] for q in a] for a in doc["plan_answers"]]
    for plan in doc["plans"]:
        _set_switches(monkeypatch, gen, plan["env"])
        assert len(plan["answers"]) == len(rows)
        for row, a in zip(rows, plan["answers"]):
            assert gen.plans(ion.capi, row) == answers[a], (plan["env"], row)
    assert len(rows) * len(doc["plans"]) > 10000


def test_refusals_and_their_precedence_are_pinned(ion, gen, doc, monkeypatch):
    """Return code and full ionode_last_error() text of every single defect and every pair of defects, per entry point and model,
    as the library of the commit named in the file gave them; the four rows of "null_descriptor" are the soundness fix that came
    with the single checked launch path.  Host stand-in pointers: runs only where no call could reach a device."""
    if torch.cuda.is_available():
        pytest.skip("a HIP device is visible: a call that slipped through the checks would launch with host addresses")
    _set_switches(monkeypatch, gen, {})
    assert set(doc["tables"]) == {f"{t}:{m}" for t in gen.TABLES for m in gen.MODELS.get(t, (gen.HH2, gen.NNF))}
    n = 0
    for key, table in doc["tables"].items():
        name, model = key.rsplit(":", 1)[0], int(key.rsplit(":", 1)[1])
        names = [d[0] for d in gen.defects(name, model)]
        assert names == table["defects"], key
        cases = gen.cases(name, model)
        assert [[names.index(d[0]) for d in c] for c in cases] == [[i for i in r[:2] if i >= 0] for r in table["rows"]], key
        for case, (_i, _j, rc, msg) in zip(cases, table["rows"]):
            assert gen.call(ion.capi, name, model, case) == (rc, doc["messages"][msg]), (key, [d[0] for d in case])
            n += 1
    assert n > 2500
    null = gen.null_descriptor_cases()
    assert [r[0] for r in doc["null_descriptor"]] == [t for t, _m, _c in null] == list(gen.SOLVES)
    for (table, model, case), (_t, rc, msg) in zip(null, doc["null_descriptor"]):
        assert (rc, msg) == (-1, "null descriptor") and gen.call(ion.capi, table, model, case) == (rc, msg), table
