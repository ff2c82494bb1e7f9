"""No GPU: the refusals the three optimiser steps share (csrc/ionode_step_capi.hpp), through ionode_lm_step_host,
ionode_cmaes_step_host and ionode_mcmc_step_host: the return code and the exact message of each.  The strings were recorded from the
library as it was when every step unit carried its own copy of these checks; they are written out here, not computed."""
import ctypes as C
import importlib

import numpy as np
import pytest

ERR_ARG = -1
K, P, NF, NPAR = 2, 1, 2, 8

BUFFERS = {"lm": "sse, jtr, jtj, status, state, flag, iters, trial", "cmaes": "value, status, state, flag, iters, trial",
           "mcmc": "value, status, state, flag, iters, trial"}
COUNTS = {"lm": "n_cand, n_active <= n_cand, n_prot and max_iter must be positive",
          "cmaes": "n_run, n_active <= n_run, n_prot, max_iter and unchanged_iters must be positive",
          "mcmc": "n_chain, n_active <= n_chain, n_prot and max_iter must be positive"}
SHARED = {
    "null_buffer": "ionode_{x}_step_host: required buffer is NULL ({buffers})",
    "n_free_0": "ionode_{x}_step_host: n_free = 0 outside 1 .. 12",
    "n_free_13": "ionode_{x}_step_host: n_free = 13 outside 1 .. 12",
    "free_index": "ionode_{x}_step_host: free index 8 outside the model's 8 parameters",
    "lo_above_hi": "ionode_{x}_step_host: bounds of free parameter 1: lo > hi (or NaN)",
    "nan_bound": "ionode_{x}_step_host: bounds of free parameter 0: lo > hi (or NaN)",
    "zero_lo_log": "ionode_{x}_step_host: log_parameters needs positive bounds (free parameter 0)",
    "n_active": "ionode_{x}_step_host: {counts}",
}


def _call(ion, step, case):
    """One *_step_host call on a complete tiny problem (K = 2, P = 1, two free parameters of eight, log parameters, the box
    0.1 .. 10) with the one defect `case` names."""
    capi = ion.capi
    fit, cmaes, mcmc = (importlib.import_module(f"{ion.__name__}.{m}") for m in ("fit", "cmaes", "mcmc"))
    box = dict(log_parameters=True, lo=[0.1, 0.1], hi=[10.0, 10.0], max_iter=5)
    base, x0 = np.linspace(1.0, 2.0, NPAR), np.ones((K, NF))
    if step == "lm":
        d = fit.lm_desc(K, P, NPAR, (0, 1), base, gtol=1e-8, xtol=1e-8, ftol=1e-8, **box)
        state, flag, iters, trial = fit.lm_init(x0, d, 1e-3)
        rows = K * P
        a = dict(sse=np.zeros(rows), jtr=np.zeros((rows, NPAR)), jtj=np.zeros((rows, NPAR, NPAR)), status=np.zeros(rows, dtype=np.int32))
        order = ("sse", "jtr", "jtj", "status", "state", "flag", "iters", "trial")
    elif step == "cmaes":
        d = cmaes.cmaes_desc(K, None, P, NPAR, (0, 1), base, **box)
        state, flag, iters, trial = cmaes.cmaes_init(x0, d)
        rows = K * getattr(d, "lambda") * P
        a = dict(value=np.zeros(rows), status=np.zeros(rows, dtype=np.int32))
        order = ("value", "status", "state", "flag", "iters", "trial")
    else:
        d = mcmc.mcmc_desc(K, P, NPAR, (0, 1), base, n_samples=10, sigma=0.1, **box)
        state, flag, iters, trial, samples = mcmc.mcmc_init(x0, d)
        rows = K * P
        a = dict(value=np.zeros(rows), status=np.zeros(rows, dtype=np.int32), samples=samples)
        order = ("value", "status", "state", "flag", "iters", "trial", "samples")
    a.update(state=state, flag=flag, iters=iters, trial=trial)
    before = {k: v.copy() for k, v in a.items()}
    if case == "null_buffer":
        a["state"] = None
    elif case == "n_free_0":
        d.n_free = 0
    elif case == "n_free_13":
        d.n_free = 13
    elif case == "free_index":
        d.free_idx[1] = NPAR
    elif case == "lo_above_hi":
        d.lo[1] = 20.0
    elif case == "nan_bound":
        d.lo[0] = float("nan")
    elif case == "zero_lo_log":
        d.lo[0] = 0.0
    elif case == "n_active":
        d.n_active = K + 1
    else:
        assert case is None
    ptrs = [None if a[n] is None else C.c_void_p(a[n].ctypes.data) for n in order]
    rc = getattr(capi.lib(), f"ionode_{step}_step_host")(C.byref(d), None, *ptrs)
    msg = capi.lib().ionode_grad_last_error().decode()
    untouched = all(a[k] is None or np.array_equal(a[k], before[k], equal_nan=True) for k in before)
    return rc, msg, untouched


@pytest.mark.parametrize("step", ["lm", "cmaes", "mcmc"])
def test_shared_refusals_keep_their_code_and_their_text(ion, step):
    rc, _, _ = _call(ion, step, None)
    assert rc == 0   # the problem itself is served: each refusal below is that of its one defect
    for case, text in SHARED.items():
        rc, msg, untouched = _call(ion, step, case)
        assert rc == ERR_ARG, (step, case, rc, msg)
        assert msg == text.format(x=step, buffers=BUFFERS[step], counts=COUNTS[step]), (step, case, msg)
        assert untouched, (step, case)
