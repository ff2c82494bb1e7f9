"""CPU: what the checker of the fused sum-of-absolute-errors gradient (tests/sae_cases.py, used on the card by
tests/test_gpu_sae_grad.py) would catch, on the drawn cases of tests/sse_cases.py -- the role tests/test_sse_fuzz_cases.py plays for
the squares.  Oracle and torch replay only: nothing here touches the library's kernels."""
import numpy as np
import pytest

import sae_cases as A
import sse_cases as S

GRAD_REL_TOL = 1e-4                 # the GPU tests' tolerance against the checker
POWER_MARGIN = 10 * GRAD_REL_TOL    # a wrong weight must move the gradient this far (relative L2) from the true one
SEEDS = (0, 3, 10)                  # HH 2-state fp64, 6-state fp32, HH 2-state fp32 on the dense grid


def _first_checked_row(oracle, c):
    rows = S.checked_rows(c, S.oracle_batch(oracle, c)["status"])
    assert rows, f"seed {c.seed}: no row for the checker"
    return rows[0]


@pytest.fixture(scope="module")
def picks(oracle):
    out = []
    for seed in SEEDS:
        c = S.case(seed)
        out.append((c, _first_checked_row(oracle, c)))
    assert {(c.model, c.f32) for c, _ in out} == {(0, False), (1, True), (0, True)} and out[-1][0].kind == "dense"
    return out


def _apart(a, b):
    return max(S.rel_l2(a[0], b[0]), S.rel_l2(a[1], b[1]))   # dL/dp and dL/dy0 apart, as the GPU tests compare them


def test_sample_weights():
    i, ref = np.array([1.0, -2.0, 0.5, np.nan, 3.0]), np.array([0.0, 0.0, 0.5, 0.0, 4.0])
    assert np.array_equal(A.sample_weights(i, ref), [1.0, -1.0, 0.0, np.nan, -1.0], equal_nan=True)   # torch.sign's values
    assert np.array_equal(A.sample_weights(i, ref, "sign0_is_1")[:3], [1.0, -1.0, 1.0])
    assert A.sign_flips([1.0, -1.0, 0.5], [1.0, 1.0, 0.5], np.zeros(3)) == 1


@pytest.mark.parametrize("wrong", ["plus_one", "two_r"])
def test_the_checker_would_expose_a_wrong_weight(oracle, picks, wrong):
    """+1 for every sample (the sign dropped) and 2 r (the squares' weight under the absolute values' kind): on each picked case the
    gradient moves by more than 10 x the GPU tolerance."""
    for c, b in picks:
        true, bad = A.reference_gradient(oracle, c, b), A.reference_gradient(oracle, c, b, wrong=wrong)
        d = _apart(bad, true)
        print(f"{wrong}: seed {c.seed} row {b}: relative L2 {d:.3e}; the replay's own sign differs at {true[2]} samples")
        assert d > POWER_MARGIN, (wrong, c.seed, b, d)


def test_the_checker_would_expose_sign_of_zero_taken_as_one(oracle, picks):
    """A reference trace that equals the kernel's current at every fourth sample: sign(0) = 1 there moves the gradient by more than
    10 x the GPU tolerance; with sign(0) = 0 those samples drop out."""
    for c, b in picks:
        row = A.ref_with_exact_zeros(oracle, c, b)
        i_kernel = A.kernel_current(oracle, c, b, S.accepted_steps_of(oracle, c, b)[0]["y"][0])
        zeros = int((i_kernel == row).sum())
        assert zeros >= (c.te.size + 3) // 4
        true = A.reference_gradient(oracle, c, b, ref_row=row)
        bad = A.reference_gradient(oracle, c, b, wrong="sign0_is_1", ref_row=row)
        d = _apart(bad, true)
        print(f"sign0_is_1: seed {c.seed} row {b}: {zeros} exact zeros, relative L2 {d:.3e}")
        assert d > POWER_MARGIN, (c.seed, b, d)

