"""-m gpu: the manifold-MALA step kernel (ionode_mala_step) against its host mirror (ionode_mala_step_host: the same per-chain routine
compiled for the host) on the drawn cases of tests/test_mala_host.py -- state, flags, counters, the trial tensor and the samples after
each of six consecutive calls (the start's evaluation and five tells), bit for bit -- and whole runs on the real Gauss-Newton
evaluation against the same runs driven in lock-step through the host mirror.  One lane per chain: K = 64 fills a wavefront, K = 67
needs a second workgroup with three live lanes."""
import importlib

import numpy as np
import pytest
import torch

import cmaes_cases as L
import kat_cases as K_
import mala_cases as M
import mcmc_cases as MC

pytestmark = pytest.mark.gpu
ACTIVE = [66, 5, 0, 31, 64, 2, 17]
NAMES = ("state", "flag", "iters", "trial", "samples")


def _compare(host, dev, what):
    assert len(host) == len(dev)
    for k, (h, d) in enumerate(zip(host, dev)):
        for name, a, b in zip(NAMES, h, d):
            if a is None and b is None:
                continue
            if not M.same_bits(a, b):
                bad = np.argwhere(np.ascontiguousarray(a).view(np.uint8).reshape(a.shape[0], -1) != np.ascontiguousarray(b).view(np.uint8).reshape(b.shape[0], -1))
                raise AssertionError(f"{what}: call {k}: {name} differs from the host mirror, first at row {bad[0][0]} (byte {bad[0][1]})")


@pytest.mark.parametrize("K", [1, 64, 67])
@pytest.mark.parametrize("log", [False, True])
@pytest.mark.parametrize("n,ss", M.DIMS)
def test_kernel_equals_the_host_mirror(gpu, n, ss, log, K):
    P = 3 if log else 1
    case = M.draw(M.case_seed(n, ss, P, log, K), K, n, P, log=log, ss=ss)
    host = M.run_sequence(case)
    assert (host[-1][1] == 0).all() and (K == 1 or 0 < host[-1][2][:, 1].sum() < 5 * K)   # the sequences accept and reject
    _compare(host, M.run_sequence(case, device=gpu), (n, ss, log, K))
    if K == 67:
        _compare(M.run_sequence(case, active=ACTIVE), M.run_sequence(case, device=gpu, active=ACTIVE), (n, ss, log, "active"))


@pytest.mark.parametrize("name", sorted(M.path_cases()))
def test_kernel_equals_the_host_mirror_on_every_path(gpu, name):
    """The box (outside proposals from its corner), failed statuses, a start that cannot be evaluated, lies outside or has a metric that
    does not factor, trial metrics that do not factor (zero, NaN), every stop flag with the frozen chains' repeated rows, thinning, a
    capped and an absent sample buffer: the paths the plain draws do not take."""
    capi = M.mods()[0]
    case, kw = M.path_cases()[name]
    host = M.run_sequence(case, **kw)
    want = {"max_iter_2": {capi.MALA_MAXITER}, "bad_start": {0, capi.MALA_NONFINITE}, "start_outside": {0, capi.MALA_NONFINITE},
            "degenerate_start": {0, capi.MALA_DEGENERATE}}.get(name, {0})
    assert set(host[-1][1].tolist()) == want
    _compare(host, M.run_sequence(case, device=gpu, **kw), name)


# ---- whole runs on the real evaluation, against the host mirror in lock-step ----

def _run_and_lockstep(ion, gpu, model, x0, pv, te, data, iters, *, base, free, bounds, y0, **kw):
    """(mala.sample on the GPU: samples, flag, iters and the final state; the same run with every iteration's gauss_newton outputs
    copied to the host and given to ionode_mala_step_host: the same four)."""
    capi, ma = M.mods()
    sens = importlib.import_module("neural-ode-ion-channels_amd.sensitivity")
    steploop = importlib.import_module("neural-ode-ion-channels_amd.steploop")
    solve_kw = dict(prot_t0=0.0, prot_dt=0.1, rtol=L.HH_RTOL, atol=L.HH_ATOL, max_step=0.0, obs_open_state_only=kw.pop("obs_open_state_only", False))
    last = {}
    smp, rate, flag, its = ma.sample(model, x0, pv, data, te, base_params=base, free=free, bounds=bounds, y0=y0, state_dtype=torch.float64, seed=3,
                                     max_iter=iters, device=gpu, callback=lambda it, st, fl, i: last.update(state=st), **solve_kw, **kw)
    dev_run = (smp.cpu().numpy(), flag.cpu().numpy(), its.cpu().numpy(), last["state"].cpu().numpy())
    P, Nt, Kc = pv.shape[0], te.shape[0], x0.shape[0]
    desc = ma.mala_desc(Kc, P, capi.n_params(model), list(free), base, log_parameters=True, lo=bounds[0], hi=bounds[1], n_samples=P * Nt, max_iter=iters,
                        sigma=kw.get("sigma"), sigma_bounds=kw.get("sigma_bounds"), seed=3)
    state, hflag, hits, trial, samples = (torch.from_numpy(a) for a in ma.mala_init(x0, desc, 1.0))
    pvt, tet, ref, pot, y0t = steploop.problem_tensors(pv, te, data, y0, Kc * P, torch.float64, torch.device(gpu))
    for _ in range(iters + 1):
        out = sens.gauss_newton(model, trial.to(gpu), pvt, y0t, tet, ref, prot_of_traj=pot, obs_g=1.0, obs_e=-86.0, max_total_steps=1_000_000, **solve_kw)
        sse, jtr, jtj, status = (t.cpu().contiguous() for t in out)
        ma.mala_step(desc, None, sse, jtr, jtj, status.to(torch.int32), state, hflag, hits, trial, samples)
    return dev_run, (samples.numpy(), hflag.numpy(), hits.numpy(), state.numpy())


def _data(ion, gpu, model, truth, pv, te, y0, sigma, **kw):
    """The two current traces of the GPU solve at the known parameters plus seeded noise of standard deviation sigma (a number, or a
    function of the clean traces).  Returns (data, sigma)."""
    sol = ion.batched.solve(model, np.tile(truth, (2, 1)), pv, list(y0), te, prot_t0=0.0, prot_dt=0.1, prot_of_traj=np.arange(2, dtype=np.int32),
                            state_dtype=torch.float64, rtol=L.HH_RTOL, atol=L.HH_ATOL, current=True, device=gpu, **kw)
    assert (sol.status.cpu().numpy() == 0).all()
    clean = sol.i.cpu().numpy()
    sigma = float(sigma(clean)) if callable(sigma) else float(sigma)
    return clean + sigma * np.random.default_rng(MC.HH_NOISE_SEED).normal(size=clean.shape), sigma


def test_hh_run_equals_the_lock_step_host_run_bit_for_bit(ion, gpu):
    """HH 2-state, cmaes_cases.hh_problem()'s two 200 ms step protocols, 201 output samples, noise of sigma 0.1 from the fixed seed,
    p1 .. p4 in log parameters plus sigma, 8 chains, 30 iterations."""
    capi = ion.capi
    pb = L.hh_problem()
    te = np.linspace(0.0, 200.0, 201)
    data, _ = _data(ion, gpu, capi.MODEL_HH2, pb["true"], pb["pv"], te, (0.0, 1.0), MC.HH_NOISE_SIGMA)
    dev, host = _run_and_lockstep(ion, gpu, capi.MODEL_HH2, MC.hh_starts(pb, 8), pb["pv"], te, data, 30, base=pb["true"], free=L.HH_FREE,
                                  bounds=(pb["lo"], pb["hi"]), y0=(0.0, 1.0), sigma_bounds=MC.HH_SIGMA_BOUNDS)
    s = dev[0]
    print("accepted", dev[2][:, 1].tolist(), "sigma", s[:, -1, 4].tolist(), "log-posterior", s[:, 0, 5].tolist(), "->", s[:, -1, 5].tolist())
    assert (dev[1] == capi.MALA_MAXITER).all() and (dev[2][:, 0] == 30).all() and s.shape == (8, 31, 6) and np.isfinite(s).all()
    assert 0 < dev[2][:, 1].sum() < 8 * 30
    for name, a, b in zip(("samples", "flag", "iters", "state"), dev, host):
        assert M.same_bits(a, b), name


def test_six_state_run_equals_the_lock_step_host_run_bit_for_bit(ion, gpu):
    """The 6-state model, three of its rate amplitudes free in log parameters, the open state observed, sigma fixed at the noise's: 8
    chains, 12 iterations."""
    capi = ion.capi
    pb = L.hh_problem()
    te = np.linspace(0.0, 200.0, 201)
    free, y0 = (0, 4, 8), (0.0, 1.0, 0.0, 0.0, 0.0, 0.0)
    truth = K_.P_M6.copy()
    data, sigma = _data(ion, gpu, capi.MODEL_MARKOV6, truth, pb["pv"], te, y0, lambda clean: 0.01 * np.abs(clean).max(), obs_open_state_only=True)
    x0 = truth[None, list(free)] * np.exp(0.01 * np.random.default_rng(29).normal(size=(8, 3)))
    dev, host = _run_and_lockstep(ion, gpu, capi.MODEL_MARKOV6, x0, pb["pv"], te, data, 12, base=truth, free=free,
                                  bounds=(truth[list(free)] / 3.0, truth[list(free)] * 3.0), y0=y0, sigma=sigma, obs_open_state_only=True)
    s = dev[0]
    print("accepted", dev[2][:, 1].tolist(), "log-posterior", s[:, 0, 3].tolist(), "->", s[:, -1, 3].tolist())
    assert (dev[1] == capi.MALA_MAXITER).all() and (dev[2][:, 0] == 12).all() and s.shape == (8, 13, 4) and np.isfinite(s).all()
    for name, a, b in zip(("samples", "flag", "iters", "state"), dev, host):
        assert M.same_bits(a, b), name
