"""-m gpu: the Levenberg-Marquardt step kernel (ionode_lm_step) against its host mirror (ionode_lm_step_host: the same routine
compiled for the host) on the drawn cases of tests/test_lm_host.py -- state, flags, iteration counts and the trial tensor after each
of two consecutive calls, bit for bit.  One lane per candidate, 64 per workgroup: C = 1 and 5 are a ragged wavefront, 67 is two
workgroups."""
import numpy as np
import pytest

import lm_cases as L

pytestmark = pytest.mark.gpu
ACTIVE = [66, 5, 0, 31, 64, 2, 17]


def _compare(host, dev, what):
    for k, (h, d) in enumerate(zip(host, dev)):
        for name, a, b in zip(("state", "flag", "iters", "trial"), h, d):
            if not L.same_bits(a, b):
                bad = np.argwhere(np.ascontiguousarray(a).view(np.uint8).reshape(a.shape[0], -1) != np.ascontiguousarray(b).view(np.uint8).reshape(b.shape[0], -1))
                raise AssertionError(f"{what}: call {k}: {name} differs from the host mirror, first at row {bad[0][0]} (byte {bad[0][1]})")


@pytest.mark.parametrize("C_", L.C_CASES)
@pytest.mark.parametrize("log", [False, True])
@pytest.mark.parametrize("P", L.P_CASES)
@pytest.mark.parametrize("nf", L.NF_CASES)
def test_kernel_equals_the_host_mirror(gpu, nf, P, log, C_):
    case = L.draw(100 * nf + 10 * P + C_ + int(log), C_, nf, P, log=log)     # test_lm_host.py::test_step_algebra's draw
    _compare(L.run_sequence(case), L.run_sequence(case, device=gpu), (nf, P, log, C_))
    if C_ == 67:
        _compare(L.run_sequence(case, active=ACTIVE), L.run_sequence(case, device=gpu, active=ACTIVE), (nf, P, log, "active"))


@pytest.mark.parametrize("log", [False, True])
def test_kernel_equals_the_host_mirror_on_the_box_and_on_every_exit(gpu, log):
    """The projection, the held variables, a failed trajectory, an indefinite matrix (retries, then stalled), a NaN start, every
    other flag: the paths the plain draws do not take."""
    capi = L.mods()[0]
    case = L.draw(7, 67, 4, 3, log=log, bounds=True)
    case["evals"][0]["jtr"] *= 300.0
    case["evals"][1]["status"][5 * 3 + 1] = 3
    for t in range(9 * 3, 10 * 3):
        case["evals"][0]["jtj"][t][np.ix_(case["free"], case["free"])] = -np.eye(4)
    case["x0"][11, 2] = np.nan
    case["evals"][0]["status"][11 * 3] = 2
    case["x0"][13] = case["hi"]          # starts on the upper bounds: held where the gradient points outwards
    case["x0"][14] = case["lo"]
    for fields in ({}, dict(gtol=1e300), dict(xtol=1e300), dict(ftol=1.0), dict(lam_max=1.5e-6), dict(max_iter=1)):
        d = capi.IonodeLmDesc.from_buffer_copy(case["desc"])
        for k, v in fields.items():
            setattr(d, k, v)
        c = dict(case, desc=d)
        host = L.run_sequence(c, lam_init=1e-6)
        if not fields:
            flags = set(host[1][1].tolist())
            assert capi.LM_STALLED in flags and capi.LM_NONFINITE in flags and capi.LM_RUNNING in flags
            delta = capi.lm_state_views(host[0][0], 4)["delta"]
            assert (delta[13] == 0).any() or (delta[14] == 0).any()   # a held variable
        _compare(host, L.run_sequence(c, device=gpu, lam_init=1e-6), fields)
