"""CPU: what the seeded sweep of the fused sum-of-squares gradient (tests/sse_cases.py, run on the card by
tests/test_gpu_sse_grad_fuzz.py) covers, measured on the generator and on the oracle's step logs, and what its references would
catch.  Oracle only: nothing here touches the library's kernels."""
import os

import numpy as np
import pytest

import kat_cases as K
import sse_cases as S

GRAD_REL_TOL = 1e-4                 # the GPU sweep's tolerance against the checker
POWER_MARGIN = 10 * GRAD_REL_TOL    # a mutated reference must be this far (relative L2) from the true one
SEEDS = range(S.N_SEEDS)


@pytest.fixture(scope="module")
def cases():
    return [S.case(seed) for seed in SEEDS]


@pytest.fixture(scope="module")
def survey(oracle, cases):
    """Per seed: the oracle's status and step counters of the batch, and the samples per accepted step of every checked row."""
    out = []
    for c in cases:
        o = S.oracle_batch(oracle, c)
        per_row = {}
        for b in S.checked_rows(c, o["status"]):
            _, steps = S.accepted_steps_of(oracle, c, b)
            per_row[b] = max(n for _, n in S.samples_per_step(c.te, steps))
        out.append(dict(status=o["status"], stats=o["stats"], most_samples=per_row))
    return out


def test_the_generator_covers_what_the_sweep_is_for(cases):
    def seen(f):
        return {f(c) for c in cases}
    assert seen(lambda c: c.model) == {K.MODEL_HH2, K.MODEL_MARKOV6} and seen(lambda c: c.f32) == {False, True}
    assert seen(lambda c: c.B) == set(S.BATCHES)
    assert seen(lambda c: c.P) == {1, 2, 5}
    assert any(c.pot is None and c.P > 1 and c.B % c.P != 0 for c in cases), "prot_of_traj = None with B not a multiple of P"
    assert any(c.pot is not None for c in cases)
    assert seen(lambda c: c.prot_t is None) == {False, True}
    assert seen(lambda c: c.prot_t0) == {0.0, 10.0} and seen(lambda c: c.prot_dt) == {0.5, 1.0, 2.0}
    assert seen(lambda c: c.kind) == set(S.GRID_KINDS)
    assert {(c.model, c.f32) for c in cases if c.kind == "dense"} == {(m, f) for m in (K.MODEL_HH2, K.MODEL_MARKOV6) for f in (False, True)}
    assert any(c.kind == "beyond" and c.prot_t is not None for c in cases), "explicit protocol times with a grid beyond the protocol"
    for c in cases:
        if c.kind == "beyond":
            assert c.te[-1] > c.t_last
        if c.kind == "two":
            assert c.te.size == 2
        if c.kind == "exact" and c.prot_t is None:
            assert np.array_equal(c.te, c.prot_t0 + np.arange(c.te.size) * c.prot_dt)
        assert c.f32 <= (c.max_step > 0), "fp32 state always gets a dt cap"
    assert seen(lambda c: c.rtol) == {1e-5, 1e-7, 1e-9} and seen(lambda c: c.atol) == {1e-7, 1e-9}
    assert seen(lambda c: (c.max_steps > 0, c.max_total_steps > 0)) == {(False, False), (True, False), (False, True)}
    assert seen(lambda c: c.nan_row is None) == {False, True}
    assert {c.cap_kind for c in cases if not c.f32} == {"stable", "random", "none"}
    assert seen(lambda c: c.obs["obs_g"]) == {1.0, 0.7, 1.3} and seen(lambda c: c.obs["obs_e"]) == {-86.0, -80.0}
    assert seen(lambda c: (c.model, c.obs["obs_open_state_only"])) == {(m, o) for m in (K.MODEL_HH2, K.MODEL_MARKOV6) for o in (False, True)}
    assert any(c.model == K.MODEL_HH2 and c.f32 and c.obs["obs_g"] != 1.0 and not c.obs["obs_open_state_only"] for c in cases), \
        "the (S)obs_g * gate cast of the HH gate in fp32 state"
    assert seen(lambda c: c.ckpt_cap) == {4, None}
    assert all(c.ref.shape == (c.P, c.te.size) and c.w.shape == (c.B,) for c in cases)


def test_the_cases_reach_the_kernel_branches(cases, survey):
    most = [max(s["most_samples"].values()) for s in survey if s["most_samples"]]
    assert any(m > 64 for m in most) and any(m > 128 for m in most), most   # the sweep's second pass of 64 lanes, and its third
    split = beside = 0
    for c, s in zip(cases, survey):
        ok = s["status"] == 0
        limit = s["status"] == 3   # STATUS_MAX_STEPS
        if limit.any() and ok.any():
            split += 1
            beside += bool(s["stats"][limit, 0].max() > s["stats"][ok, 0].max())
    assert split >= 4, split       # a step limit trips inside a batch that also has successful rows
    assert beside >= 1             # ... and a failed row holds the batch's largest accepted-step count
    # checkpoint regrowth from ckpt_cap = 4: some such case needs more than 4 accepted steps
    assert any(c.ckpt_cap == 4 and s["stats"][s["status"] == 0, 0].max() > 4 for c, s in zip(cases, survey))
    # the NaN starts fail alone
    assert all(s["status"][c.nan_row] != 0 for c, s in zip(cases, survey) if c.nan_row is not None)


def test_the_sweep_stays_honest(cases, survey):
    """Conditions, not measurements: no case is empty, most trajectories succeed, and the GPU sweep cannot skip."""
    n = ok = 0
    for c, s in zip(cases, survey):
        assert (s["status"] == 0).any(), f"seed {c.seed}: every trajectory fails"
        assert s["most_samples"], f"seed {c.seed}: no row for the checker"
        n, ok = n + c.B, ok + int((s["status"] == 0).sum())
    assert ok >= 0.75 * n, (ok, n)
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_gpu_sse_grad_fuzz.py")) as f:
        text = f.read()
    assert "pytest.skip" not in text and "mark.skip" not in text and "xfail" not in text


def _applies(mutation, c, s, b):
    if mutation == "drop_sample0":
        return True
    if mutation == "ref_row0":
        return S.prot_index(c, b) != 0
    if mutation == "first64_only":
        return s["most_samples"][b] > 64
    if mutation == "last_v_beyond":
        return c.kind == "beyond"
    if mutation == "swap_gate":
        return c.model == K.MODEL_HH2 and not c.obs["obs_open_state_only"]
    if mutation == "no_obs_g":
        return c.obs["obs_g"] != 1.0
    raise AssertionError(mutation)


@pytest.mark.parametrize("mutation", S.MUTATIONS)
def test_the_references_would_expose_the_mistake(oracle, cases, survey, mutation):
    """The first seed (and its first checked row) where the mutation applies: the wrong reference's dL/dp or dL/dy0 is further
    than 10 x the gradient tolerance from the true one, so a kernel making that mistake fails the GPU sweep on this seed."""
    pick = next(((c, b) for c, s in zip(cases, survey) for b in sorted(s["most_samples"]) if _applies(mutation, c, s, b)), None)
    assert pick is not None, "no seed of the range exercises this branch"
    c, b = pick
    true, wrong = S.reference_gradient(oracle, c, b), S.reference_gradient(oracle, c, b, mutate=mutation)
    d = max(S.rel_l2(wrong[0], true[0]), S.rel_l2(wrong[1], true[1]))   # dL/dp and dL/dy0 apart, as the GPU sweep compares them
    print(f"{mutation}: seed {c.seed} row {b}: relative L2 {d:.3e}")
    assert d > POWER_MARGIN, (mutation, c.seed, b, d)
