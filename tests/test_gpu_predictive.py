"""-m gpu: the predictive bands' kernels (ionode_predictive_accumulate, ionode_predictive_quantiles) against their host mirrors -- the same
element routines compiled for the host -- on the seeded synthetic cases of tests/test_predictive_host.py, bit for bit: mean, m2, min, max,
count, the column store with its +inf slots, and the quantiles; with and without noise, in one chunk and in chunks of 7 draws (a chunk
that is no multiple of the 32-draw tile, sample counts that are no multiple of the 64-sample workgroup, more than one workgroup a
protocol at Nt = 130).  One case at the cap of 16 384 draws for the full-LDS sort, and one real solve with failing draws."""
import numpy as np
import pytest
import torch

import cmaes_cases as L
import kat_cases as K
import predictive_cases as PC
import rate_edge_cases as RE

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]


def _differs(host, dev):
    return [k for k in host if (host[k] is None) != (dev[k] is None) or (host[k] is not None and not L.same_bits(host[k], dev[k]))]


@pytest.mark.parametrize("S,Nt,P", PC.SHAPES)
def test_kernels_equal_the_host_mirrors(gpu, S, Nt, P):
    case = PC.make(S, Nt, P)
    for noise in (False, True):
        for chunk in (None, 7):
            kw = dict(chunk=chunk, noise=noise, sigma=case.sigma if noise else None, seed=5)
            assert _differs(PC.run(case, **kw), PC.run(case, device=gpu, **kw)) == [], (noise, chunk)
    kw = dict(chunk=7, noise=True, sigma=0.3, seed=6, store=False, draw_offset=1000)      # moments only, one sigma, a shard's offset
    assert _differs(PC.run(case, **kw), PC.run(case, device=gpu, **kw)) == []


def test_the_cap_sorts_in_full_lds(gpu, ion):
    """S_cap = 16 384 draws, three samples, one protocol: the quantile kernel's largest instantiation, 128 KiB of keys in LDS, with
    failed draws at both ends and in the middle and noise on; chunks of 5000 draws."""
    capi = ion.capi
    case = PC.make(capi.PREDICTIVE_MAX_DRAWS, 3, 1)
    assert case.s_cap == 16384 and capi.predictive_plan(1, 3, case.s_cap)["lds_bytes"] == 131072 and case.fail.sum() == 3
    kw = dict(chunk=5000, noise=True, sigma=case.sigma, seed=9)
    host, dev = PC.run(case, **kw), PC.run(case, device=gpu, **kw)
    assert _differs(host, dev) == [] and dev["count"].tolist() == [16381] and np.isfinite(dev["quant"]).all()
    assert (np.diff(dev["quant"][0], axis=0) >= 0).all()


def test_real_solve_with_failing_draws(gpu, ion):
    """HH 2-state, fp64 state, the two rate-edge protocols (tests/rate_edge_cases.py) on 201 samples, 24 draws of (p2, p6): 22 around the
    physical values and two from the rate-edge table (rows 2 and 1: an exponent of 7.2, whose exp() overflows on the positive protocol and
    underflows on the negative one).  bands in chunks of 5 draws against the plain batched.solve(current=True) of all 48 rows plus the host mirror
    on its trace, bit for bit; the failed draws are absent from their protocol's count."""
    capi, pr = PC.mods()
    S, P, Nt = 24, 2, 201
    rng = np.random.default_rng(12)
    base = K.P_HH.copy()
    d = base[None, [1, 5]] * np.exp(0.05 * rng.normal(size=(S, 2)))
    d[3], d[17] = (7.2, base[5]), (base[1], 7.2)
    d = np.concatenate([d, 0.05 + 0.1 * rng.random((S, 1))], axis=1)
    te = np.linspace(0.0, 598.0, Nt)
    kw = dict(base_params=base, free=(1, 5), prot_t0=0.0, prot_dt=1.0, state_dtype=torch.float64, device=gpu)
    b = pr.bands(capi.MODEL_HH2, d, RE.protocols(), te, chunk_bytes=5 * P * Nt * 8, noise=True, seed=2, quantiles=PC.Q, **kw)
    rows = np.tile(base, (S, 1))
    rows[:, [1, 5]] = d[:, :2]
    sol = ion.batched.solve(capi.MODEL_HH2, np.repeat(rows, P, axis=0), RE.protocols(), torch.tensor([[0.0, 1.0]], dtype=torch.float64), te, prot_t0=0.0,
                            prot_dt=1.0, prot_of_traj=np.tile(np.arange(P, dtype=np.int32), S), rtol=1e-7, atol=1e-9, max_total_steps=1_000_000,
                            current=True, device=gpu)      # (states and all: the plain solve's current trace)
    status = sol.status.cpu().numpy().astype(np.int32)
    failed = (status.reshape(S, P) != 0)
    print("failed (draw, protocol):", np.argwhere(failed).tolist())
    assert failed[3].any() and failed[17].any() and failed.sum(axis=0).max() == 2 and not failed[[k for k in range(S) if k not in (3, 17)]].any()
    st = pr.new_state(P, Nt, S, "cpu")
    pr.accumulate(st, sol.i.cpu().contiguous(), torch.from_numpy(status), draw_base=0, sigma=torch.from_numpy(np.ascontiguousarray(d[:, 2])), noise=True, seed=2)
    want = pr.finish(st, PC.Q, S, pr.quantile_pass(st, PC.Q))
    assert b.count.cpu().tolist() == (S - failed.sum(axis=0)).tolist() == want.count.tolist()
    for name in ("mean", "min", "max", "m2", "quantiles"):
        assert L.same_bits(getattr(b, name).cpu().numpy(), getattr(want, name).numpy()), name
    # sd is torch's sqrt(m2 / (count - 1)) on either device, not the kernels': a division and a square root, each good to an ulp
    assert (np.abs(b.sd.cpu().numpy() / want.sd.numpy() - 1.0) <= 4 * PC.U).all()
    assert torch.isfinite(b.quantiles).all() and (b.sd > 0).all()
