"""The inputs of tests/test_gpu_rate_edges.py, checked on the oracle alone (no GPU): every batch the GPU test compares must contain
what makes the comparison mean something -- trajectories that integrate with rates that underflow or vanish, trajectories that fail at
once, one that fails late, and healthy physical rows.  The statuses come from the oracle; nothing here writes them down."""
import numpy as np
import pytest

import kat_cases as K
import rate_edge_cases as R


def test_the_rows_reach_the_arguments_they_are_meant_to():
    """Row by row: the extreme exponent arguments on the two protocols are the ones the range cases of exp() need."""
    pv = R.protocols()
    assert pv.shape == (2, 600) and np.array_equal(pv[R.POS], -pv[R.NEG]) and sorted(set(pv[R.NEG])) == [-103.5, -100.0, -80.0, -60.0, -20.0]
    assert R.T_EVAL[0] == 0.0 and R.T_EVAL[-1] == 598.0 and R.T_EVAL.size == 300
    for model in (K.MODEL_HH2, K.MODEL_MARKOV6, K.MODEL_NND):
        p = R.rows(model)
        assert p.shape == (R.N_ROWS, 12 if model == K.MODEL_MARKOV6 else 8)
        lo = lambda r, i: float((p[r, i] * pv[R.NEG]).min())
        assert lo(1, 5) == pytest.approx(-745.2) and -745.2 < -745.1332191019412       # beyond the last subnormal: exp() returns 0
        assert lo(6, 5) == pytest.approx(-733.815) and lo(6, 5) > -745.1332191019412    # a subnormal result
        assert lo(3, 5) == pytest.approx(-931.5) and lo(8, 5) == pytest.approx(-765.9)
        assert float((p[1, 5] * pv[R.POS]).max()) > 709.782712893384                    # ... and overflow on the negated protocol
        assert np.isnan(p[7, 4]) and 0 < p[12, 4] < 2.2250738585072014e-308
        assert lo(13, 5) < -2.0 ** 53 and p[14, 7] > np.finfo(np.float64).max / 20.0 and sorted(R.TILE_ORDER) == list(range(R.N_ROWS))
        for r in R.PHYSICAL:
            assert np.array_equal(p[r], R.base_params(model))
    # which rows count as out of range follows the exponents the model reads: NN-f ignores p0 .. p3
    picks = [(r, R.NEG) for r in range(R.N_ROWS)]
    assert R.batch(K.MODEL_NND, picks)[2].tolist() == [r in (1, 2, 3, 4, 5, 6, 8, 9, 12, 13, 14) for r in range(R.N_ROWS)]
    assert R.batch(K.MODEL_NNF, picks)[2].tolist() == [r in (1, 3, 4, 6, 8, 9, 12, 13, 14) for r in range(R.N_ROWS)]


def test_the_mixed_batches_put_physical_rows_in_a_wavefront_of_their_own():
    for picks, wave, n_mixed in ((R.MIX64, 64, 64), (R.MIX16, 16, 32)):
        for model in (K.MODEL_HH2, K.MODEL_MARKOV6, K.MODEL_NNF, K.MODEL_NND):
            _, _, oor, row = R.batch(model, picks)
            for w in range(0, n_mixed, wave):
                assert oor[w:w + wave].any() and not oor[w:w + wave].all()     # takes the general exp, with in-range lanes beside
            assert not oor[n_mixed:].any() and np.isin(row[n_mixed:], R.PHYSICAL).all()   # takes the in-range exp


_solved = {}


@pytest.mark.parametrize("case", R.GPU_CASES, ids=[c[0] for c in R.GPU_CASES])
def test_every_gpu_case_is_not_vacuous(oracle, case):
    name, model, f32, net, picks, _tile_waves, _frag, _frag_lean, at_once = case
    key = (model, f32, net, tuple(picks))
    if key not in _solved:        # cases that differ in the tile only share a solve
        _, _, oor, row, _, o = R.oracle_solve(oracle, model, f32, net, picks)
        _solved[key] = (o["status"], o["stats"], oor, row)
    counts = R.not_vacuous(*_solved[key], at_once=at_once)
    print(name, "out-of-range and status 0: %d, failed: %d, of them late: %d, physical: %d" % counts)
