"""The solve kernel's tail of the deferred dense output, host side (no GPU): ionode_dense_tail_plan's rank rule and usable capacity, the
switches, and the resources of the kernels that carry the expansion routine in the built library."""
import importlib
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

RECORD_BYTES = 112   # DenseRecord<2>: (4 + 5 * 2) doubles
EIGHTHS = 5          # the default gate: the first 5/8 of the tiles to end (profiles/defer_tail.md)


@pytest.fixture()
def capi(monkeypatch):
    for k in ("IONODE_DEFER_DENSE", "IONODE_DEFER_DENSE_CAP", "IONODE_DEFER_TAIL", "IONODE_DEFER_TAIL_RANK"):
        monkeypatch.delenv(k, raising=False)
    return importlib.import_module("neural-ode-ion-channels_amd").capi


def _desc(capi, *, model=2, f32=False, B=4096, Nt=100001, width=200, layers=5, exact=1, tile_waves=0, **kw):
    return capi.make_desc(model=model, state_f32=int(f32), n_state=2, n_out=Nt, n_traj=B, n_prot=B, prot_n=Nt, mlp_layers=layers,
                          mlp_width=width, n_params=8, prot_t0=0.0, prot_dt=0.1, v_oob=-80.0, rtol=1e-7, atol=1e-9, obs_g=1.0,
                          obs_e=-86.0, tile_waves=tile_waves, t_eval_t0_hint=0.0, t_eval_dt_hint=0.1, t_eval_exact=exact, **kw)


def _cap(B, Nt, f32, current):
    out_bytes = B * Nt * 2 * (4 if f32 else 8) + (B * Nt * 8 if current else 0)
    cap = min(Nt - 1, (out_bytes // 4) // (B * RECORD_BYTES))
    return 0 if cap < 64 else cap


def test_headline_shape(capi):
    d = _desc(capi)
    assert ", 4, 4, 13, 13, 8>" in capi.kernel_name(d)
    assert capi.dense_tail_plan(d, True) == {"tail_rank": 256 * EIGHTHS // 8, "usable_capacity": 5356}
    # ionode_dense_defer_plan's numbers are what they were: the counter comes out of the workspace
    assert capi.dense_defer_plan(d, True) == {"capacity": 5357, "workspace_bytes": 16 * 1024 + 4096 * 5357 * RECORD_BYTES}


@pytest.mark.parametrize("model", [2, 3])
@pytest.mark.parametrize("f32", [False, True])
@pytest.mark.parametrize("B,Nt,current", [(48, 2001, True), (48, 4001, False), (35, 2001, True), (32, 16001, True), (2048, 20001, True), (16, 2001, True)])
def test_rank_rule_and_usable_capacity(capi, model, f32, B, Nt, current):
    d = _desc(capi, model=model, f32=f32, B=B, Nt=Nt, tile_waves=4)
    cap, tiles = _cap(B, Nt, f32, current), (B + 15) // 16
    assert cap >= 64
    rank = tiles * EIGHTHS // 8          # floor(f * tiles): a single tile never expands by default
    assert capi.dense_tail_plan(d, current) == {"tail_rank": rank, "usable_capacity": cap - 1 if rank else cap}
    assert capi.dense_defer_plan(d, current) == {"capacity": cap, "workspace_bytes": ((4 * B + 15) // 16) * 16 + B * cap * RECORD_BYTES}


def test_switches_are_read_per_plan(capi, monkeypatch):
    d = _desc(capi, B=48, Nt=2001, tile_waves=4)
    cap = _cap(48, 2001, False, True)
    assert capi.dense_tail_plan(d, True) == {"tail_rank": 3 * EIGHTHS // 8, "usable_capacity": cap - 1}
    monkeypatch.setenv("IONODE_DEFER_TAIL", "0")
    assert capi.dense_tail_plan(d, True) == {"tail_rank": 0, "usable_capacity": cap}
    monkeypatch.setenv("IONODE_DEFER_TAIL", "all")
    assert capi.dense_tail_plan(d, True) == {"tail_rank": 3, "usable_capacity": cap - 1}
    monkeypatch.delenv("IONODE_DEFER_TAIL")
    monkeypatch.setenv("IONODE_DEFER_TAIL_RANK", "1")
    assert capi.dense_tail_plan(d, True) == {"tail_rank": 1, "usable_capacity": cap - 1}
    monkeypatch.setenv("IONODE_DEFER_TAIL_RANK", "7")          # at most every tile
    assert capi.dense_tail_plan(d, True)["tail_rank"] == 3
    monkeypatch.setenv("IONODE_DEFER_TAIL_RANK", "0")
    assert capi.dense_tail_plan(d, True) == {"tail_rank": 0, "usable_capacity": cap}
    monkeypatch.setenv("IONODE_DEFER_TAIL", "0")               # off is off, whatever the forced rank
    monkeypatch.setenv("IONODE_DEFER_TAIL_RANK", "2")
    assert capi.dense_tail_plan(d, True)["tail_rank"] == 0
    monkeypatch.delenv("IONODE_DEFER_TAIL")
    monkeypatch.delenv("IONODE_DEFER_TAIL_RANK")
    assert capi.dense_tail_plan(d, True)["tail_rank"] == 3 * EIGHTHS // 8
    for k in ("IONODE_DEFER_TAIL", "IONODE_DEFER_TAIL_RANK"):  # neither switch touches the workspace plan
        monkeypatch.setenv(k, "0")
        assert capi.dense_defer_plan(d, True)["capacity"] == cap
        monkeypatch.delenv(k)


def test_no_tail_where_nothing_is_deferred_or_one_record(capi, monkeypatch):
    zero = {"tail_rank": 0, "usable_capacity": 0}
    assert capi.dense_tail_plan(_desc(capi, width=100), True) == zero        # another tile: no deferral
    assert capi.dense_tail_plan(_desc(capi, B=8192), True) == zero
    assert capi.dense_tail_plan(_desc(capi, model=0), True) == zero
    monkeypatch.setenv("IONODE_DEFER_DENSE", "0")
    assert capi.dense_tail_plan(_desc(capi), True) == zero
    monkeypatch.delenv("IONODE_DEFER_DENSE")
    monkeypatch.setenv("IONODE_DEFER_DENSE_CAP", "1")                        # one record slot: none to spare for the counter
    assert capi.dense_tail_plan(_desc(capi, B=48, Nt=2001, tile_waves=4), True) == {"tail_rank": 0, "usable_capacity": 1}
    monkeypatch.setenv("IONODE_DEFER_DENSE_CAP", "2")
    assert capi.dense_tail_plan(_desc(capi, B=48, Nt=2001, tile_waves=4), True) == {"tail_rank": 3 * EIGHTHS // 8, "usable_capacity": 1}
    monkeypatch.setenv("IONODE_DEFER_DENSE_CAP", "8")
    assert capi.dense_tail_plan(_desc(capi, B=48, Nt=2001, tile_waves=4), True) == {"tail_rank": 3 * EIGHTHS // 8, "usable_capacity": 7}


@pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf") or shutil.which("c++filt") is None, reason="llvm tools")
def test_resources_of_the_kernels_that_expand(capi):
    from kernel_resources import kernel_resources
    rows = kernel_resources(capi.LIB_PATH)
    expand = [r for r in rows if "ionode_dense_expand_kernel<" in r["kernel"]]
    assert len(expand) == 2, [r["kernel"] for r in expand]
    for r in expand:
        assert r["scratch_bytes"] == 0 and r["vgpr_spill"] == 0 and r["lds_static"] == 0 and r["vgpr"] <= 128, r
    solve = [r for r in rows if "ionode_dopri5_kernel<" in r["kernel"] and r["kernel"].split("(")[0].endswith(", 4, 4, 13, 13, 8>")]
    assert len(solve) == 4, [r["kernel"] for r in solve]      # {NN-f, NN-d} x {fp64, fp32}: the kernels with the tail
    for r in solve:
        assert r["scratch_bytes"] == 0 and r["vgpr_spill"] == 0 and r["vgpr"] <= 512, r
