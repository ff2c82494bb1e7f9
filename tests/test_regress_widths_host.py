"""The regression step's plan for every MLP width up to 512 (no GPU, no HIP call): ionode_regress_plan, the slab count of the
run-time-width reduce kernel, and the index maps regression.MlpRegression builds from ionode_grad_pack at widths without a tuned tile."""
import ctypes as C

import numpy as np
import pytest

TUNED = set(range(1, 17)) | set(range(97, 113)) | set(range(193, 209)) | set(range(497, 513))   # N pads to 16, 112, 208 or 512


@pytest.fixture(autouse=True)
def _no_switch(monkeypatch):
    monkeypatch.delenv("IONODE_GRAD_GENERIC", raising=False)   # (the A/B switch would send the tuned widths to the run-time-width kernels)


def test_every_width_has_a_plan_or_a_reason(ion):
    capi = ion.capi
    refused = []
    for N in range(1, 513):
        try:
            plan = capi.regress_plan(1, N)
        except capi.IonodeError as e:
            assert "LDS" in str(e), (N, str(e))
            assert N not in TUNED
            refused.append(N)
            continue
        assert plan["generic"] == (N not in TUNED), (N, plan)
        assert 1 <= plan["wg_per_cu"] <= 4 and 0 < plan["lds_bytes"] <= 160 * 1024, (N, plan)
        assert plan["wg_per_cu"] * plan["lds_bytes"] <= 160 * 1024 or plan["wg_per_cu"] == 1, (N, plan)
    assert all(N >= 449 for N in refused), refused
    assert refused == list(range(481, 497))   # 31 k-tiles with three remainder tiles' partial sums: 161 KB at any depth
    # the tuned kernels' plans are what regression.py used before the library planned it
    assert capi.regress_plan(5, 200)["wg_per_cu"] == 2 and capi.regress_plan(5, 100)["wg_per_cu"] == 2 and capi.regress_plan(5, 10)["wg_per_cu"] == 2
    assert capi.regress_plan(5, 500)["wg_per_cu"] == 1
    # deeper nets: the biases of every layer are LDS-resident, so the widest nets stop earlier (include/ionode.h states this set)
    deepest = {N: max(L for L in range(1, 16) if _served(capi, L, N)) for N in (416, 432, 448, 464, 480, 512)}
    assert deepest == {416: 15, 432: 10, 448: 15, 464: 14, 480: 7, 512: 10}


def _served(capi, L, N):
    try:
        capi.regress_plan(L, N)
        return True
    except capi.IonodeError:
        return False


@pytest.mark.parametrize("L,N", [(1, 513), (0, 64), (16, 64)])
def test_shapes_outside_the_range_are_refused(ion, L, N):
    with pytest.raises(ion.capi.IonodeError, match="outside the served shapes"):
        ion.capi.regress_plan(L, N)
    out = (C.c_int32 * 3)()
    assert ion.capi.lib().ionode_regress_plan(L, N, C.byref(out)) == -2   # IONODE_ERR_UNSUPPORTED (include/ionode.h)


def test_the_switch_plans_the_run_time_width_kernels_at_tuned_widths(ion, monkeypatch):
    capi = ion.capi
    tuned = capi.regress_plan(5, 200)
    monkeypatch.setenv("IONODE_GRAD_GENERIC", "1")
    forced = capi.regress_plan(5, 200)
    assert not tuned["generic"] and forced["generic"]
    assert capi.lib().ionode_grad_reduce_slabs(5, 200, 8276) == 512 // (5 * 2 * 1 + 1)   # two column blocks of eight tiles, one row block
    monkeypatch.setenv("IONODE_GRAD_GENERIC", "0")
    assert capi.regress_plan(5, 200) == tuned and capi.lib().ionode_grad_reduce_slabs(5, 200, 8276) == 69


def test_plan_answers_without_a_device(ion, monkeypatch):
    """ionode_regress_plan is host arithmetic (csrc/ionode_grad_capi.hip: no HIP call in it, by reading the code).  What this test can
    show is only that it answers the same with no device visible to the process as with whatever the machine has."""
    seen = ion.capi.regress_plan(5, 64), ion.capi.regress_plan(2, 300), ion.capi.regress_plan(5, 200)
    monkeypatch.setenv("HIP_VISIBLE_DEVICES", "")
    monkeypatch.setenv("ROCR_VISIBLE_DEVICES", "")
    assert (ion.capi.regress_plan(5, 64), ion.capi.regress_plan(2, 300), ion.capi.regress_plan(5, 200)) == seen
    assert seen[0] == {"generic": True, "wg_per_cu": 4, "lds_bytes": 20240}


@pytest.mark.parametrize("L,N", [(5, 64), (2, 300), (1, 464)])
def test_reduce_slab_count_at_widths_without_a_tuned_kernel(ion, L, N):
    lib = ion.capi.lib()
    for n_records in (1, 3, 63, 8276, 100000):
        n = lib.ionode_grad_reduce_slabs(L, N, n_records)
        assert n >= 1
        if n_records // 4 >= 1:
            assert n <= n_records // 4
    NT = (N + 15) // 16
    per_slab = L * ((NT + 7) // 8) * ((NT + 15) // 16) + 1   # (layer, column block, row block) jobs + the light one
    assert lib.ionode_grad_reduce_slabs(L, N, 10**6) == max(1, 512 // per_slab)   # no device: 256 compute units, two workgroups each


@pytest.mark.parametrize("L,N", [(2, 50), (3, 300)])
def test_grad_pack_places_every_weight_once_per_section(ion, L, N):
    """regression.MlpRegression's imgmap is ionode_grad_pack of the values 1..n: the image refresh after every Adam step is right only
    if each flat index lands exactly once in the forward fragment section and once in the transposed one."""
    lib = ion.capi.lib()
    n = 2 * N + N + L * (N * N + N) + N + 1
    assert n < (1 << 24)
    idx = np.arange(1, n + 1, dtype=np.float32)
    img = np.empty(lib.ionode_grad_image_floats(L, N), dtype=np.float32)
    assert lib.ionode_grad_pack(idx.ctypes.data, L, N, img.ctypes.data) == 0
    NT = (N + 15) // 16
    NP = 16 * NT
    fwd0 = 4 * NP + L * NP + NP + 4          # rows of layer 0 | hidden biases | wl, bl
    sec = L * NT * NT * 256
    assert img.size == fwd0 + 2 * sec
    m = img.astype(np.int64)
    # flat order: W0 [N][2], b0 [N], then per hidden layer W [N][N], b [N], then wl [N], bl
    hidden_w = np.concatenate([3 * N + l * (N * N + N) + np.arange(N * N) for l in range(L)]) + 1
    for name, part in (("forward", m[fwd0:fwd0 + sec]), ("transposed", m[fwd0 + sec:])):
        got = np.sort(part[part > 0])
        assert np.array_equal(got, hidden_w), name                       # each hidden weight exactly once, nothing else
        assert np.count_nonzero(part == 0) == sec - L * N * N, name     # the rest is padding
    head = m[:fwd0]
    rest = np.setdiff1d(np.arange(1, n + 1), hidden_w)                    # W0, b0, hidden biases, wl, bl
    assert np.array_equal(np.sort(head[head > 0]), rest)
