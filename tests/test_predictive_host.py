"""No GPU: the posterior predictive bands through their host mirrors (ionode_predictive_accumulate_host, ionode_predictive_quantiles_host:
the kernels' element routines compiled for the host) on the seeded synthetic cases of tests/predictive_cases.py -- moments and order
statistics against numpy, independence of the chunking, the noise, the pooling of sampler output, the refusals -- and predictive.bands /
objective.population_predictive end to end with the CPU oracle as the solver.  tests/test_gpu_predictive.py holds the kernels to these
mirrors bit for bit."""
import ctypes as C
import importlib
import os
import re
import socket
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import cmaes_cases as L
import predictive_cases as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("ionode_predictive_plan", "ionode_predictive_accumulate", "ionode_predictive_accumulate_host", "ionode_predictive_quantiles",
           "ionode_predictive_quantiles_host")


def _obj():
    return importlib.import_module("neural-ode-ion-channels_amd.objective")


# ---- the entry points ----

def test_header_declares_the_entry_points_and_the_abi_stays_10(ion):
    capi = ion.capi
    hdr = open(os.path.join(ROOT, "include", "ionode.h")).read()
    lib = C.CDLL(capi.LIB_PATH)
    for entry in ENTRIES:
        assert re.search(rf"\bint\s+{entry}\s*\(", hdr) and entry in capi.EXPORTS and getattr(lib, entry) is not None
    assert capi.ABI_VERSION == 10 and capi.lib().ionode_abi_version() == 10 and re.search(r"#define\s+IONODE_ABI_VERSION\s+10\b", hdr)
    for name, val in (("MAX_DRAWS", capi.PREDICTIVE_MAX_DRAWS), ("MAX_Q", capi.PREDICTIVE_MAX_Q), ("TAG", capi.PREDICTIVE_TAG)):
        assert int(re.search(rf"#define\s+IONODE_PREDICTIVE_{name}\s+(\w+?)u?\s", hdr).group(1), 0) == val
    body = re.sub(r"/\*.*?\*/", "", hdr[hdr.index("typedef struct ionode_predictive_desc {"):hdr.index("} ionode_predictive_desc;")], flags=re.S)
    names = [n.strip() for decl in re.findall(r"(?:int32_t|int64_t|double)\s+([^;]+);", body) for n in decl.split(",")]
    assert names == [f[0] for f in capi.IonodePredictiveDesc._fields_]
    # the tag is no step's: their fourth word is pair + 65536 * attempt with a handful of attempts
    assert capi.PREDICTIVE_TAG == 65536 * PC.TAG_ATTEMPT and PC.TAG_ATTEMPT > 1000
    text = open(os.path.join(ROOT, "neural-ode-ion-channels_amd", "csrc", "ionode_predictive.hpp")).read()
    for user in ("CMA-ES", "Metropolis", "MALA", "ensemble"):
        assert user in text   # the header comment lists the tags in use


# ---- moments and quantiles against numpy ----

@pytest.mark.parametrize("S,Nt,P", PC.SHAPES)
def test_moments_and_quantiles_against_numpy(ion, S, Nt, P):
    """Bounds, for m surviving draws of a column and M = max |x| over them, u = 2^-53:
    min, max, count exact.
    |mean - np.mean| <= 4 m u M.  Welford's step mean_n = mean_(n-1) + (x_n - mean_(n-1)) / n rounds three times: the difference (at most
    u |d|, |d| <= 2 M), the quotient (u |d| / n) and the sum (u M); the error carried in is damped by (1 - 1 / n).  So with e_n = a_n u M:
    a_1 = 0 (the first step is exact) and a_n <= (1 - 1 / n) a_(n-1) + 1 + 4 / n, which stays below n / 2 + 4; numpy's pairwise sum and
    its division add at most (log2 m + 2) u M; together below 4 m for every m >= 2 (m = 2: 1 + 4 + 1 + 2 = 8).
    sd within 1e-12 relative: the cases are N(1, 1) with a few planted zeros, denormals and repeats -- m2 is a sum of m non-negative
    terms d (x - mean) each good to a few u of (2 M)^2, the sum itself to m u: (4 m + 8) u M^2 / m2 per unit of m2, below 1e-13 here.
    Quantiles: the value equals the header's formula evaluated in numpy on np.sort's elements, BIT FOR BIT -- so the two order
    statistics used are np.sort's, exactly -- and agrees with np.quantile(method="linear") to 4 u max(|x_lo|, |x_hi|) (numpy
    interpolates by another formula, each side rounding at most twice)."""
    case = PC.make(S, Nt, P)
    out = PC.run(case)
    want_count = (~case.fail).sum(axis=0)
    assert out["count"].dtype == np.int64 and out["count"].tolist() == want_count.tolist()
    seen = set()
    for p in range(P):
        xs = PC.survivors(case, p)
        m = xs.shape[0]
        seen.add(min(m, 2))
        if m == 0:                                       # nothing survived: the fresh state, NaN quantiles, no fault
            assert (out["mean"][p] == 0).all() and (out["m2"][p] == 0).all() and (out["min"][p] == np.inf).all() and (out["max"][p] == -np.inf).all()
            assert np.isnan(out["quant"][p]).all()
            continue
        M = np.abs(xs).max(axis=0)
        assert np.array_equal(out["min"][p], xs.min(axis=0)) and np.array_equal(out["max"][p], xs.max(axis=0))
        err = np.abs(out["mean"][p] - xs.mean(axis=0))
        assert (err <= 4 * m * PC.U * M).all(), (err / (PC.U * M + 1e-300)).max()
        if m >= 2:
            sd, ref = np.sqrt(out["m2"][p] / (m - 1)), xs.std(axis=0, ddof=1)
            assert (np.abs(sd - ref) <= 1e-12 * ref).all(), np.abs(sd / ref - 1).max()
        else:
            assert (out["m2"][p] == 0).all() and np.array_equal(out["mean"][p], xs[0])   # (0 + (-0 - 0) / 1 is +0: equal, not the same bits)
        srt = PC.key_sort(xs)
        assert np.array_equal(srt, np.sort(xs, axis=0))   # (the keys' order is the values'; it also orders -0 before +0)
        for j, q in enumerate(PC.Q):
            val, xlo, xhi = PC.quantile_statement(srt, q)
            assert L.same_bits(out["quant"][p, j], val), (p, q)
            assert (np.abs(out["quant"][p, j] - np.quantile(xs, q, axis=0, method="linear")) <= 4 * PC.U * np.maximum(np.abs(xlo), np.abs(xhi))).all()
            if m == 1:
                assert np.array_equal(out["quant"][p, j], xs[0])      # (-0 comes back as -0 + 0 (-0 - -0) = +0: equal)
    # the column store: the survivors' values in their slots, +inf in a failed draw's and in the slots never written
    cols = out["cols"]
    assert cols.shape == (P, Nt, case.s_cap)
    x = case.trace.reshape(S, P, Nt)
    for p in range(P):
        want = np.where(case.fail[:, p][None, :], np.inf, x[:, p].T)
        assert L.same_bits(cols[p, :, :S], np.ascontiguousarray(want)) and (cols[p, :, S:] == np.inf).all()
    if P == 3:
        assert seen == ({0, 1, 2} if S >= 5 else {0, 1})   # none, one and many survivors are all there


def test_bands_finish_gives_nan_where_the_issue_says(ion):
    """count = 0: NaN everywhere; one survivor: sd NaN and every quantile equal to it."""
    _, pr = PC.mods()
    case = PC.make(33, 37, 3)
    st = pr.new_state(3, 37, case.s_cap, "cpu")
    pr.accumulate(st, torch.from_numpy(case.trace), torch.from_numpy(case.status), draw_base=0)
    b = pr.finish(st, PC.Q, 33, pr.quantile_pass(st, PC.Q))
    assert b.count.tolist() == [30, 0, 1] and b.n_draws == 33 and b.q == PC.Q
    for t in (b.mean[1], b.sd[1], b.min[1], b.max[1], b.quantiles[1], b.sd[2]):
        assert torch.isnan(t).all()
    one = torch.from_numpy(PC.survivors(case, 2)[0])
    assert all(torch.equal(b.quantiles[2, j], one) for j in range(5)) and torch.equal(b.mean[2], one) and torch.equal(b.min[2], one)
    xs = PC.survivors(case, 0)
    assert np.allclose(b.sd[0].numpy(), xs.std(axis=0, ddof=1), rtol=1e-12, atol=0) and not torch.isnan(b.quantiles[0]).any()


# ---- the chunking does not matter ----

@pytest.mark.parametrize("noise", [False, True])
@pytest.mark.parametrize("S,Nt,P", [(33, 37, 3), (100, 130, 1), (5, 1, 3)])
def test_chunks_of_1_7_and_all_give_the_same_bits(ion, S, Nt, P, noise):
    case = PC.make(S, Nt, P)
    kw = dict(noise=noise, sigma=case.sigma if noise else None, seed=11)
    whole = PC.run(case, **kw)
    assert PC.same_bits(whole, PC.run(case, chunk=1, **kw)) and PC.same_bits(whole, PC.run(case, chunk=7, **kw))
    lean = PC.run(case, chunk=7, store=False, **kw)        # without the column store: the same moments
    assert all(L.same_bits(lean[k], whole[k]) for k in ("mean", "m2", "min", "max", "count")) and lean["cols"] is None
    assert noise == (not PC.same_bits(whole, PC.run(case)))


# ---- the noise ----

def test_noise_is_standard_normal_scales_per_draw_and_is_fixed_by_the_seed(ion):
    capi, pr = PC.mods()
    S, Nt, P = 100, 130, 2
    case = PC.make(S, Nt, P, seed=5)
    case.status[:] = 0
    case.trace[:] = 1.0 + np.random.default_rng(6).normal(size=case.trace.shape)
    case.fail[:] = False
    sigma0 = 0.1
    clean, noisy = PC.run(case)["cols"], PC.run(case, noise=True, sigma=sigma0, seed=3)["cols"]
    z = ((noisy - clean) / sigma0).reshape(-1)
    n = z.size
    print(f"n {n}: mean {z.mean():.5f} (bound {5 / np.sqrt(n):.5f}), variance {z.var():.5f} - 1 (bound {5 * np.sqrt(2 / n):.5f})")
    assert n >= 20000 and abs(z.mean()) <= 5 / np.sqrt(n) and abs(z.var() - 1.0) <= 5 * np.sqrt(2.0 / n)
    # on a zero trace the stored value is sigma z itself: the deviate is the generator's, and a per-draw sigma scales draw by draw
    zero = PC.make(S, Nt, P, seed=5)
    zero.status[:], zero.trace[:], zero.fail[:] = 0, 0.0, False
    one, per = PC.run(zero, noise=True, sigma=1.0, seed=3)["cols"], PC.run(zero, noise=True, sigma=zero.sigma, seed=3)["cols"]
    assert L.same_bits(per, one * zero.sigma[None, None, :])
    assert np.allclose(one, z.reshape(P, Nt, S), rtol=0, atol=1e-14 / sigma0)
    for draw, p, k in ((0, 0, 0), (99, 1, 129), (17, 1, 64), (50, 0, 1)):
        assert one[p, k, draw] == PC.normal(3, draw, p, k)
    # a function of the draw's index among all draws: draw_offset shifts it
    shifted = PC.run(zero, noise=True, sigma=1.0, seed=3, draw_offset=7)["cols"]
    assert L.same_bits(shifted[:, :, :S - 7], one[:, :, 7:])
    # two seeds differ, the same seed repeats
    assert L.same_bits(one, PC.run(zero, noise=True, sigma=1.0, seed=3)["cols"]) and not L.same_bits(one, PC.run(zero, noise=True, sigma=1.0, seed=4)["cols"])
    assert L.same_bits(PC.run(zero, noise=True, sigma=0.0, seed=3)["cols"], np.zeros((P, Nt, S)))


# ---- predictive.draws ----

def test_draws_selects_what_rhat_selects(ion):
    capi, pr = PC.mods()
    mc = importlib.import_module("neural-ode-ion-channels_amd.mcmc")
    rng = np.random.default_rng(2)
    K, R, n = 5, 21, 3
    s = rng.normal(size=(K, R, n + 1))
    flag = np.full(K, capi.MCMC_MAXITER, dtype=np.int32)
    flag[3] = capi.MCMC_DEGENERATE          # a stopped chain: its rows after the stop were never recorded
    s[3, 9:] = np.nan
    s[1, 17:] = np.nan                      # a NaN tail on a chain that counts
    kept = mc.kept(s, flag, 0.5)
    assert kept.shape == (4, 11, n) and L.same_bits(kept, s[[0, 1, 2, 4], 10:, :n])
    d = pr.draws(s, flag, burn=0.5)
    want = s[[0, 1, 2, 4], 10:, :n].reshape(-1, n)
    want = want[~np.isnan(want).any(axis=1)]
    assert d.shape == (44 - 4, n) and L.same_bits(d, want) and d.flags["C_CONTIGUOUS"]
    # rhat judges the same rows
    r = mc.rhat(s[:, :17], flag, burn=0.0)
    h = mc.kept(s[:, :17], flag, 0.0)
    W, B = h.var(axis=1, ddof=1).mean(axis=0), h.mean(axis=1).var(axis=0, ddof=1)
    assert np.allclose(r, np.sqrt((16 / 17 * W + B) / W), rtol=1e-14)
    # thin: every second kept row of each chain; flag None: all chains (the stopped one gives what it recorded); torch input
    d2 = pr.draws(torch.from_numpy(s), torch.from_numpy(flag), burn=0.5, thin=2)
    w2 = s[[0, 1, 2, 4], 10::2, :n].reshape(-1, n)
    assert L.same_bits(d2, w2[~np.isnan(w2).any(axis=1)])
    assert pr.draws(s, None, burn=0.0).shape == (5 * 21 - 12 - 4, n)
    # max_draws: an evenly spaced subset, first row included, order kept
    d7 = pr.draws(s, flag, burn=0.5, max_draws=7)
    idx = np.floor(np.arange(7) * (40 / 7)).astype(int)
    assert L.same_bits(d7, want[idx]) and L.same_bits(pr.draws(s, flag, burn=0.5, max_draws=40), want)
    with pytest.raises(capi.IonodeError, match="thin"):
        pr.draws(s, flag, thin=0)


# ---- refusals ----

def test_refusals_by_name(ion):
    capi, pr = PC.mods()
    plan = capi.predictive_plan(2, 20001, 16384)
    assert plan == {"lds_bytes": 131072, "cols_bytes": 8 * 2 * 20001 * 16384, "sort_log2": 14} and plan["lds_bytes"] <= 160 * 1024
    assert capi.predictive_plan(1, 1, 1)["lds_bytes"] == 16 and capi.predictive_plan(3, 7, 33)["lds_bytes"] == 512
    assert capi.predictive_plan(3, 7, 100, 8 * 3 * 7 * 100)["cols_bytes"] == 16800
    with pytest.raises(capi.IonodeError, match=r"s_cap = 16385 .* exceed 16384.*max_draws"):
        capi.predictive_plan(1, 3, 16385)
    with pytest.raises(capi.IonodeError, match=r"column store \[3\]\[7\]\[100\] takes 16800 bytes, above budget_bytes = 16799.*max_draws"):
        capi.predictive_plan(3, 7, 100, 16799)
    case = PC.make(5, 37, 3)
    tr, stt = torch.from_numpy(case.trace), torch.from_numpy(case.status)
    st = pr.new_state(3, 37, 5, "cpu")
    with pytest.raises(capi.IonodeError, match="noise without sigma"):
        pr.accumulate(st, tr, stt, draw_base=0, noise=True)
    with pytest.raises(capi.IonodeError, match=r"draws 1 \.\. 5 do not fit the column store's s_cap = 5"):
        pr.accumulate(st, tr, stt, draw_base=1)
    with pytest.raises(capi.IonodeError, match=r"q\[1\] = 1\.5 outside \[0, 1\]"):
        pr.quantile_pass(st, (0.5, 1.5))
    with pytest.raises(capi.IonodeError, match=r"q\[0\] = nan outside"):
        pr.quantile_pass(st, (float("nan"),))
    with pytest.raises(capi.IonodeError, match="n_q = 17 outside 1 .. 16"):
        pr.quantile_pass(st, (0.5,) * 17)
    with pytest.raises(capi.IonodeError, match="status: expected a contiguous torch.int32"):
        pr.accumulate(st, tr, stt.long(), draw_base=0)
    with pytest.raises(capi.IonodeError, match=r"trace \[n \* 3, 37\] expected"):
        pr.accumulate(st, tr[:, :36].contiguous(), stt, draw_base=0)
    assert (st["count"] == 0).all() and (st["mean"] == 0).all() and torch.isinf(st["cols"]).all()     # nothing was touched
    lib = capi.lib()
    d = capi.IonodePredictiveDesc(n_prot=3, n_out=37, n_draw=5, s_cap=5)
    assert lib.ionode_predictive_accumulate_host(C.byref(d), None, None, None, None, None, None, None, None, None) == -1
    assert "required buffer is NULL (trace, status, mean, m2, min, max, count)" in lib.ionode_grad_last_error().decode()
    assert lib.ionode_predictive_accumulate(None, None, None, None, None, None, None, None, None, None, None) == -1     # refused before any HIP call
    assert "null descriptor" in lib.ionode_grad_last_error().decode()
    # the driver: a draw width that is neither nf nor nf + 1, noise without sigma, q outside [0, 1], sigma twice, too many draws, the budget
    kw = dict(base_params=np.full(8, 1.0), free=(0, 1, 2), solver=lambda *a, **k: None, device="cpu")
    args = (np.zeros((2, 10)), np.arange(5.0))
    for bad, extra, text in ((np.ones((4, 5)), {}, r"draws \[S, 3\] or \[S, 4\] \(sigma last\) expected for 3 free parameters, got \(4, 5\)"),
                             (np.ones((4, 3)), dict(noise=True), "noise without sigma"),
                             (np.ones((4, 3)), dict(quantiles=(0.5, -0.1)), r"every q must lie in \[0, 1\]"),
                             (np.ones((4, 4)), dict(sigma=0.1), "one of them"),
                             (np.ones((16385, 3)), {}, "exceed 16384.*max_draws"),
                             (np.ones((100, 3)), dict(budget_bytes=1000), "above budget_bytes = 1000"),
                             (np.ones((4, 3)), dict(max_step="auto"), "max_step must be a number"),
                             (np.ones((4, 3)), dict(coordinates="u"), "coordinates")):
        with pytest.raises(capi.IonodeError, match=text):
            pr.bands(capi.MODEL_HH2, bad, *args, **{**kw, **extra})


# ---- end to end: the CPU oracle as the solver ----

HH_S = 6


def _hh(oracle):
    pb = L.hh_problem()
    rng = np.random.default_rng(8)
    x = pb["true"][None, :4] * np.exp(0.05 * rng.normal(size=(HH_S, 4)))
    d = np.concatenate([x, 0.05 + 0.1 * rng.random((HH_S, 1))], axis=1)      # sigma rides as the last column
    kw = dict(base_params=pb["true"], free=L.HH_FREE, prot_dt=pb["prot_dt"], state_dtype=torch.float64, rtol=L.HH_RTOL, atol=L.HH_ATOL, device="cpu")
    return pb, d, kw, pb["te"][::10]


def test_bands_end_to_end_with_the_cpu_oracle_as_the_solver(ion, oracle):
    """HH 2-state, cmaes_cases.hh_problem()'s two protocols on 201 samples, six draws around the known parameters with their own sigma:
    bands in chunks of two draws against numpy on the traces the same solver gives for all draws at once."""
    capi, pr = PC.mods()
    pb, d, kw, te = _hh(oracle)
    calls = []
    b = pr.bands(capi.MODEL_HH2, d, pb["pv"], te, solver=PC.current_solver(oracle, calls), chunk_bytes=2 * 2 * 201 * 8, max_step=0.0, **kw)
    assert calls == [4, 4, 4] and b.n_draws == HH_S and b.count.tolist() == [HH_S, HH_S] and b.quantiles.shape == (2, 3, 201)
    p = np.repeat(np.tile(pb["true"], (HH_S, 1)), 2, axis=0)
    p[:, :4] = np.repeat(d[:, :4], 2, axis=0)
    sol = PC.current_solver(oracle)(capi.MODEL_HH2, torch.from_numpy(p), torch.from_numpy(pb["pv"]), torch.zeros(12, 2), torch.from_numpy(te), prot_t0=0.0,
                                    prot_dt=pb["prot_dt"], prot_of_traj=torch.from_numpy(np.tile(np.arange(2, dtype=np.int32), HH_S)), rtol=L.HH_RTOL,
                                    atol=L.HH_ATOL, max_step=0.0, current=True, states=False, sse_ref=torch.zeros(2, 201))
    i = sol.i.numpy().reshape(HH_S, 2, 201)
    scale = np.abs(i).max()
    assert np.abs(b.mean.numpy() - i.mean(axis=0)).max() <= 4 * HH_S * PC.U * scale
    assert np.allclose(b.sd.numpy(), i.std(axis=0, ddof=1), rtol=1e-9, atol=1e-14 * scale)   # (columns where all draws nearly agree: absolute)
    assert np.array_equal(b.min.numpy(), i.min(axis=0)) and np.array_equal(b.max.numpy(), i.max(axis=0))
    want = np.quantile(i, (0.025, 0.5, 0.975), axis=0, method="linear").transpose(1, 0, 2)
    assert np.abs(b.quantiles.numpy() - want).max() <= 4 * PC.U * scale
    assert (b.quantiles[:, 0] <= b.quantiles[:, 1]).all() and (b.quantiles[:, 1] <= b.quantiles[:, 2]).all() and scale > 1.0
    # the prediction band: wider than the credible band, the same whatever the chunking, moved by the seed
    noisy = [pr.bands(capi.MODEL_HH2, d, pb["pv"], te, solver=PC.current_solver(oracle), chunk_bytes=c, noise=True, seed=s, max_step=0.0, **kw)
             for c, s in ((1, 1), (1 << 30, 1), (1 << 30, 2))]
    assert torch.equal(noisy[0].quantiles, noisy[1].quantiles) and torch.equal(noisy[0].m2, noisy[1].m2)
    assert not torch.equal(noisy[1].quantiles, noisy[2].quantiles)
    assert (noisy[0].sd.mean() > b.sd.mean()) and (noisy[0].max - noisy[0].min).mean() > (b.max - b.min).mean()
    # the search space's coordinates (log x, log sigma) give the same trial rows and noise levels up to exp(log x): each of the two
    # functions is good to an ulp, so the relative difference is at most (|log x| + 2) u, |log x| < 14 here.  Moments only: no store.
    u = np.concatenate([np.log(d[:, :4]), np.log(d[:, 4:])], axis=1)
    rows = []

    def recording(model, params, prot_v, y0, t_eval, **k):
        rows.append(params.numpy().copy())
        return PC.current_solver(oracle)(model, params, prot_v, y0, t_eval, **k)

    bu = pr.bands(capi.MODEL_HH2, u, pb["pv"], te, solver=recording, coordinates="search", quantiles=None, noise=True, seed=1, max_step=0.0, **kw)
    assert bu.quantiles is None and len(rows) == 1 and rows[0].shape == p.shape and np.abs(rows[0] / p - 1.0).max() <= 16 * PC.U
    x, sig = pr.parameters(u, 4, coordinates="search")
    assert np.abs(sig / d[:, 4] - 1.0).max() <= 16 * PC.U and np.array_equal(x, rows[0][::2, :4]) and (bu.sd.mean() > b.sd.mean())


def test_population_predictive_resolves_the_step_cap_once_and_equals_bands(ion, oracle):
    capi, pr = PC.mods()
    obj = _obj()
    pb, d, kw, te = _hh(oracle)
    seen = []

    def solver(model, params, prot_v, y0, t_eval, **k):
        seen.append(k["max_step"])
        return PC.current_solver(oracle)(model, params, prot_v, y0, t_eval, **k)

    kw = {k: v for k, v in kw.items() if k != "device"}
    b = obj.population_predictive(d, pb["pv"], te, solver=solver, device="cpu", chunk_bytes=3 * 2 * 201 * 8, **kw)
    cap = seen[0]
    assert len(seen) == 2 and seen[1] == cap and isinstance(cap, float) and cap > 0.0      # "auto": one number, the same in every chunk
    one = pr.bands(capi.MODEL_HH2, d, pb["pv"], te, solver=PC.current_solver(oracle), max_step=cap, device="cpu", **kw)
    for name in ("mean", "sd", "min", "max", "quantiles", "count", "m2"):
        assert torch.equal(getattr(b, name), getattr(one, name)), name
    assert "REFUSED" in obj.population_predictive.__doc__ and "rank order" in obj.population_predictive.__doc__.lower()


# ---- two ranks under gloo: shards of 3 + 3, the moments merged in rank order, quantiles refused ----

def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _synthetic_solver(case_traces, P):
    """A stand-in that looks its rows up: parameter 0 of a row is the draw's index."""
    from types import SimpleNamespace

    def solver(model, params, prot_v, y0, t_eval, **kw):
        idx = params[:, 0].long()
        pot = kw["prot_of_traj"].long()
        i = case_traces[idx, pot]
        assert kw["current"] is True and kw["states"] is False
        return SimpleNamespace(i=i.contiguous(), status=(idx % 5 == 3).to(torch.int32) * 2)
    return solver


def _sharded(quantiles, noise):
    obj = _obj()
    S, P, Nt = 11, 2, 37
    traces = torch.from_numpy(1.0 + np.random.default_rng(9).normal(size=(S, P, Nt)))
    d = np.arange(S, dtype=np.float64)[:, None]
    return traces, obj.population_predictive(d, np.zeros((P, 10)), np.arange(float(Nt)), base_params=np.full(8, 1.0), free=(0,), log_parameters=False,
                                             sigma=0.2 if noise else None, noise=noise, seed=4, quantiles=quantiles, max_step=0.0,
                                             solver=_synthetic_solver(traces, P), device="cpu", chunk_bytes=4 * P * Nt * 8)


def _worker(rank, world, port, q):
    for p in (ROOT, os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist_mod = importlib.import_module("neural-ode-ion-channels_amd.distributed")
    capi = importlib.import_module("neural-ode-ion-channels_amd.capi")
    d = dist_mod.init_process_group()
    _, b = _sharded(None, True)
    refused = ""
    try:
        _sharded((0.5,), False)
    except capi.IonodeError as e:
        refused = str(e)
    q.put((rank, {k: getattr(b, k).numpy() for k in ("mean", "sd", "min", "max", "count")}, refused))
    d.barrier()
    d.destroy_process_group()


@pytest.mark.timeout(300)
def test_two_ranks_merge_the_moments_in_rank_order(ion):
    traces, one = _sharded(None, True)
    assert one.count.tolist() == [9, 9]          # draws 3 and 8 fail
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = {r: (out, refused) for r, out, refused in (q.get(timeout=240) for _ in range(2))}
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for r in (0, 1):
        out, refused = got[r]
        assert "exact quantiles need all draws of a column on one device and the group has 2 ranks" in refused
        assert np.array_equal(out["count"], one.count.numpy()) and np.array_equal(out["min"], one.min.numpy()) and np.array_equal(out["max"], one.max.numpy())
        # the pairwise merge rounds differently from one walk over all draws: a few units in the last place of values of order one
        assert np.abs(out["mean"] - one.mean.numpy()).max() <= 16 * PC.U * 4.0 and np.allclose(out["sd"], one.sd.numpy(), rtol=1e-13, atol=0)
    assert all(L.same_bits(got[0][0][k], got[1][0][k]) for k in got[0][0])     # every rank holds the same bands
