"""Deferred dense output of the lean N = 200 16-tile, host side (no GPU): ionode_dense_defer_plan's capacity rule and the expansion
kernel's resources in the built library."""
import importlib
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

RECORD_BYTES = 112   # DenseRecord<2>: (4 + 5 * 2) doubles


@pytest.fixture()
def capi(monkeypatch):
    for k in ("IONODE_DEFER_DENSE", "IONODE_DEFER_DENSE_CAP"):
        monkeypatch.delenv(k, raising=False)
    return importlib.import_module("neural-ode-ion-channels_amd").capi


def _desc(capi, *, model=2, f32=False, B=4096, Nt=100001, width=200, layers=5, exact=1, tile_waves=0, **kw):
    return capi.make_desc(model=model, state_f32=int(f32), n_state=2, n_out=Nt, n_traj=B, n_prot=B, prot_n=Nt, mlp_layers=layers,
                          mlp_width=width, n_params=8, prot_t0=0.0, prot_dt=0.1, v_oob=-80.0, rtol=1e-7, atol=1e-9, obs_g=1.0,
                          obs_e=-86.0, tile_waves=tile_waves, t_eval_t0_hint=0.0, t_eval_dt_hint=0.1, t_eval_exact=exact, **kw)


def _rule(B, Nt, f32, current):
    out_bytes = B * Nt * 2 * (4 if f32 else 8) + (B * Nt * 8 if current else 0)
    cap = min(Nt - 1, (out_bytes // 4) // (B * RECORD_BYTES))
    return 0 if cap < 64 else cap


def _bytes(B, cap):
    return ((4 * B + 15) // 16) * 16 + B * cap * RECORD_BYTES


def test_headline_shape_gets_5357_records(capi):
    d = _desc(capi)
    assert ", 4, 4, 13, 13, 8>" in capi.kernel_name(d)
    p = capi.dense_defer_plan(d, True)
    assert p == {"capacity": 5357, "workspace_bytes": _bytes(4096, 5357)}, p
    assert p["workspace_bytes"] <= (4096 * 100001 * 24) // 4 + 4 * 4096 + 16   # a quarter of the outputs' bytes (+ the counts)


@pytest.mark.parametrize("model", [2, 3])
@pytest.mark.parametrize("f32", [False, True])
@pytest.mark.parametrize("B,Nt,current", [(48, 2001, True), (48, 4001, False), (35, 2001, True), (2048, 20001, True), (4096, 4001, False)])
def test_capacity_rule_of_the_eligible_plans(capi, model, f32, B, Nt, current):
    d = _desc(capi, model=model, f32=f32, B=B, Nt=Nt, tile_waves=4)
    want = _rule(B, Nt, f32, current)
    assert want >= 64
    assert capi.dense_defer_plan(d, current) == {"capacity": want, "workspace_bytes": _bytes(B, want)}


def test_capacity_under_64_defers_nothing(capi):
    assert _rule(48, 21, False, True) == 0
    assert capi.dense_defer_plan(_desc(capi, B=48, Nt=21, tile_waves=4), True) == {"capacity": 0, "workspace_bytes": 0}
    # fp32 states without the current trace: 8 bytes per sample, a quarter of them over 112 -> one record per 56 outputs
    assert capi.dense_defer_plan(_desc(capi, f32=True, B=48, Nt=3583, tile_waves=4), False)["capacity"] == 0
    assert capi.dense_defer_plan(_desc(capi, f32=True, B=48, Nt=3584, tile_waves=4), False)["capacity"] == 64


def test_non_eligible_plans_defer_nothing(capi, monkeypatch):
    zero = {"capacity": 0, "workspace_bytes": 0}
    assert capi.dense_defer_plan(_desc(capi), True)["capacity"] > 0
    assert capi.dense_defer_plan(_desc(capi, width=100), True) == zero                 # another width: the N = 100 tile
    assert capi.dense_defer_plan(_desc(capi, width=500), True) == zero
    assert capi.dense_defer_plan(_desc(capi, width=150), True) == zero                 # the run-time-width tile
    assert capi.dense_defer_plan(_desc(capi, exact=0), True) == zero                   # output grid not verified: the general variant
    assert capi.dense_defer_plan(_desc(capi, B=8192), True) == zero                    # 32-trajectory tile
    assert capi.dense_defer_plan(_desc(capi, B=1024), True) == zero                    # 4-trajectory tile
    assert capi.dense_defer_plan(_desc(capi, model=0), True) == zero                   # closed-form model
    assert capi.dense_defer_plan(_desc(capi, sse_ref=4096, sse_out=8192), True) == zero   # the fused objective (never dereferenced by a plan)
    assert capi.dense_defer_plan(_desc(capi, ckpt=4096, ckpt_cap=8), True) == zero     # checkpoints: the general variant
    monkeypatch.setenv("IONODE_DEFER_DENSE", "0")
    assert capi.dense_defer_plan(_desc(capi), True) == zero                            # the switch, read per plan
    monkeypatch.setenv("IONODE_DEFER_DENSE", "1")
    assert capi.dense_defer_plan(_desc(capi), True)["capacity"] == 5357


def test_forced_capacity(capi, monkeypatch):
    monkeypatch.setenv("IONODE_DEFER_DENSE_CAP", "8")
    assert capi.dense_defer_plan(_desc(capi, B=48, Nt=2001, tile_waves=4), True) == {"capacity": 8, "workspace_bytes": _bytes(48, 8)}
    assert capi.dense_defer_plan(_desc(capi, width=100), True)["capacity"] == 0        # only where the plan defers at all
    monkeypatch.setenv("IONODE_DEFER_DENSE_CAP", "100000")
    assert capi.dense_defer_plan(_desc(capi, B=48, Nt=2001, tile_waves=4), True)["capacity"] == 2000   # at most n_out - 1
    monkeypatch.setenv("IONODE_DEFER_DENSE", "0")
    assert capi.dense_defer_plan(_desc(capi, B=48, Nt=2001, tile_waves=4), True)["capacity"] == 0


@pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf") or shutil.which("c++filt") is None, reason="llvm tools")
def test_expansion_kernel_resources(capi):
    from kernel_resources import kernel_resources
    rows = [r for r in kernel_resources(capi.LIB_PATH) if "ionode_dense_expand_kernel<" in r["kernel"]]
    assert sorted(r["kernel"].split("(")[0].split("ionode::")[-1] for r in rows) == ["ionode_dense_expand_kernel<double, 2>",
                                                                                    "ionode_dense_expand_kernel<float, 2>"]
    for r in rows:
        assert r["scratch_bytes"] == 0 and r["vgpr_spill"] == 0 and r["lds_static"] == 0 and r["vgpr"] <= 128, r
