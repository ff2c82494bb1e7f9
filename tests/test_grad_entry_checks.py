"""CPU tests of the seven backward-sweep entry points' host side: what they refuse and in which order (pinned by
tests/golden/grad_entry_checks.json), and the buffer names capi.py calls them with."""
import importlib.util
import json
import os

import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


def _generator():
    spec = importlib.util.spec_from_file_location("make_grad_entry_checks", os.path.join(GOLDEN, "make_grad_entry_checks.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    return gen


def test_entry_point_refusals_and_their_precedence_are_pinned(ion):
    """tests/golden/grad_entry_checks.json (tests/golden/make_grad_entry_checks.py): return code and ionode_grad_last_error() text
    of every single defect and every pair of defects, per entry point and model, as the library of the commit named in the file
    gave them.  Host stand-in pointers: runs only where no call could reach a device."""
    if torch.cuda.is_available():
        pytest.skip("a HIP device is visible: a call that slipped through the checks would launch with host addresses")
    gen = _generator()
    doc = json.load(open(os.path.join(GOLDEN, "grad_entry_checks.json")))
    assert set(doc["tables"]) == {f"{e}/{m}" for e in gen.ENTRIES for m in gen.served(e)}
    n = 0
    for key, table in doc["tables"].items():
        entry, model = key.split("/")[0], int(key.split("/")[1])
        names = [d[0] for d in gen.defects(entry, model)]
        assert names == table["defects"], key
        cases = gen.cases(entry, model)
        assert [[names.index(d[0]) for d in c] for c in cases] == [[i for i in r[:2] if i >= 0] for r in table["rows"]], key
        for case, (_i, _j, rc, msg) in zip(cases, table["rows"]):
            assert gen.call(ion.capi, entry, model, case) == (rc, doc["messages"][msg]), (key, [d[0] for d in case])
            n += 1
    assert n > 4000   # 29 defects at the most, all their pairs, seven entry points, two to four models each


def test_sweep_buffer_names_follow_the_header(ion):
    """capi.SWEEP_BUFFERS, from which the entry points' argtypes are generated and by which grad.py names every pointer it passes:
    the names and their order are the parameter names of include/ionode.h's prototypes."""
    protos = _generator().prototypes()
    assert len(protos) == 7
    assert {name: list(buffers) + ["stream"] for name, buffers in ion.capi.SWEEP_BUFFERS.items()} == protos
