"""GPU: the multi-exponential fit kernels against their host mirrors, bit for bit -- the objective on the host test's cases (every
lane and wavefront boundary, both kinds, the empty segment, the overflow row, an active permutation) and on 67 runs x lambda = 64
rows, the evaluation, one whole fit, and fit_activation(fitter="cmaes").  The CPU-path fits are computed once (expfit_cases)."""
import numpy as np
import pytest

import expfit_cases as E

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("n_params", [7, 5])
def test_objective_kernel_equals_the_host_mirror(gpu, n_params):
    case = E.objective_case(n_params)
    for active in (None, E.ACTIVE):
        host, dev = E.run_objective(case, "cpu", active), E.run_objective(case, gpu, active)
        assert E.same_bits(dev[0], host[0]) and E.same_bits(dev[1], host[1]), active
    lam = case["lam"]
    value, status = E.run_objective(case, gpu)
    assert value[E.OVERFLOW_ROW[0] * lam + E.OVERFLOW_ROW[1]] == np.inf
    assert (value.reshape(-1, lam)[E.EMPTY] == np.inf).all() and (status.reshape(-1, lam)[E.EMPTY] == 1).all() and status.sum() == lam


def test_objective_kernel_on_67_runs_of_64_candidates(gpu):
    case = E.objective_case(7, seed=1, seg_of_run=tuple(r % 9 for r in range(67)), lam=64, overflow=(16, 63))
    host, dev = E.run_objective(case, "cpu"), E.run_objective(case, gpu)
    assert host[0].shape == (67 * 64,) and np.isfinite(host[0]).sum() > 3500
    assert E.same_bits(dev[0], host[0]) and E.same_bits(dev[1], host[1])
    order = tuple(np.random.default_rng(2).permutation(67)[:41])
    host, dev = E.run_objective(case, "cpu", order), E.run_objective(case, gpu, order)
    assert E.same_bits(dev[0], host[0]) and E.same_bits(dev[1], host[1])


@pytest.mark.parametrize("n_params", [7, 5])
def test_eval_kernel_equals_the_host_mirror(gpu, n_params):
    x, t_list = E.eval_case(n_params)
    host, dev = E.run_eval(x, t_list, "cpu"), E.run_eval(x, t_list, gpu)
    for q in range(3):
        for g in range(len(t_list)):
            assert E.same_bits(dev[q][g], host[q][g]), (q, g)
    assert np.abs(host[2][5]).max() > 0


def test_a_whole_fit_equals_the_cpu_path(gpu):
    """Recovery cases 0 and 2, restarts 3, max_iter 200, compact_every 4: x, rmse, flag and iters bit for bit."""
    host, dev = E.whole_fit("cpu"), E.whole_fit(str(gpu))
    assert host[0].shape == (2, 7) and host[2].shape == (2, 4) and (host[3][:, :, 0] > 50).all()
    for name, a, b in zip(("x", "rmse", "flag", "iters"), dev, host):
        assert E.same_bits(a, b), name


def test_fit_activation_with_the_cmaes_fitter_equals_the_cpu_path(gpu):
    host, dev = E.protocol_fit("cpu"), E.protocol_fit(str(gpu))
    assert dev[3] == host[3] and [k[2] for k in host[3]] == E.small_protocol()["kinds"]
    for q in range(3):
        assert E.same_bits(dev[q], host[q]), q
