"""No GPU: the adaptive-Metropolis step through its host mirror ionode_mcmc_step_host -- the per-chain routine the kernel runs, compiled
for the host.  Header / binding / library agreement, every refusal, the step's algebra on seeded cases against the numpy statement of
tests/mcmc_cases.py, the paths (flags, frozen chains, the box, failures, thinning), and a chain's independence of its company."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import mcmc_cases as M

ROOT = os.path.join(os.path.dirname(__file__), "..")
ENTRIES = ("ionode_mcmc_step", "ionode_mcmc_step_host")
ERR_ARG = -1
NAMES = ["d", "active", "value", "status", "state", "flag", "iters", "trial", "samples"]
EPS = M.EPS
INF = float("inf")


def _header():
    return open(os.path.join(ROOT, "include", "ionode.h")).read()


def test_header_prototypes_and_library_agree(ion):
    capi, hdr = ion.capi, _header()
    assert "#define IONODE_ABI_VERSION 10" in hdr and capi.ABI_VERSION == 10 and capi.lib().ionode_abi_version() == 10
    for entry, extra in zip(ENTRIES, (["stream"], [])):
        args = re.search(r"\bint\s+%s\s*\(([^;]*)\);" % entry, hdr).group(1).split(",")
        restype, argtypes = capi.PROTOTYPES[entry]
        assert restype is C.c_int and len(argtypes) == len(args) and [a.split()[-1].lstrip("*") for a in args] == NAMES + extra
        assert entry in capi.EXPORTS and getattr(C.CDLL(capi.LIB_PATH), entry) is not None
    body = hdr[hdr.index("typedef struct ionode_mcmc_desc {"):hdr.index("} ionode_mcmc_desc;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names, sizes = [], 0
    for ctype, decl in re.findall(r"(int32_t|int64_t|double)\s+([^;]+);", body):
        for n in decl.split(","):
            names.append(re.sub(r"\[.*?\]", "", n).strip())
            sizes += (4 if ctype == "int32_t" else 8) * (capi.LM_MAX_FREE if "[" in n else 1)
    assert names == [f[0] for f in capi.IonodeMcmcDesc._fields_] and sizes == C.sizeof(capi.IonodeMcmcDesc)   # (no padding anywhere)
    assert names[:12] == ["n_chain", "n_active", "n_prot", "n_params", "n_free", "log_parameters", "sample_sigma", "max_iter", "adapt_start", "thin",
                          "sample_cap", "chain_base"]
    const = dict(re.findall(r"#define IONODE_MCMC_(\w+) (\S+)", hdr))
    assert len(const) == 10
    for k, v in const.items():
        assert float(v) == getattr(capi, "MCMC_" + k), k
    assert capi.MCMC_MAX_DIM == 13 == capi.LM_MAX_FREE + 1 and set(capi.MCMC_FLAG_TEXT) == set(range(4))
    assert capi.mcmc_state_doubles(4) == 4 + 20 + 32 and capi.mcmc_state_doubles(13) == 407
    st = np.zeros((3, capi.mcmc_state_doubles(5)))
    views = capi.mcmc_state_views(st, 4, 1)
    for k, name in enumerate(views):   # the views tile the state: writing k + 1 into view k leaves no word unwritten
        views[name][:] = k + 1
    assert (st == 0).sum() == 0 and sorted(np.unique(st).tolist()) == list(range(1, 12))
    assert views["C"].shape == (3, 5, 5) and views["L"].shape == (3, 5, 5) and views["xt"].shape == (3, 5)
    assert capi.mcmc_state_views(np.zeros((2, capi.mcmc_state_doubles(4))), 4, 0)["u"].shape == (2, 4)


def _call(capi, case, *, entry="ionode_mcmc_step_host", null=(), **fields):
    d = capi.IonodeMcmcDesc.from_buffer_copy(case["desc"])
    for k, v in fields.items():
        if isinstance(v, tuple):
            getattr(d, k)[v[0]] = v[1]
        else:
            setattr(d, k, v)
    state, flag, iters, trial, samples = M.start(case)
    rows = trial.shape[0]
    a = dict(active=None, value=torch.ones(rows, dtype=torch.float64), status=torch.zeros(rows, dtype=torch.int32), state=state, flag=flag,
             iters=iters, trial=trial, samples=samples)
    ptrs = [None if (n in null or a[n] is None) else C.c_void_p(a[n].data_ptr()) for n in NAMES[1:]]
    tail = (None,) if entry == "ionode_mcmc_step" else ()
    rc = getattr(capi.lib(), entry)(None if "d" in null else C.byref(d), *ptrs, *tail)
    return rc, capi.lib().ionode_grad_last_error().decode(), (state, flag, iters, trial, samples)


def test_refusals_come_before_anything_is_touched(ion):
    capi = ion.capi
    nan = float("nan")
    sampled, fixed = M.draw(0, 3, 5, 2, log=True, ss=1), M.draw(0, 3, 4, 2, log=True, ss=0)
    entries = ("ionode_mcmc_step_host",) if torch.cuda.is_available() else ENTRIES   # (with a device a call that slipped through would launch on host addresses)
    for entry in entries:
        tried = [(sampled, dict(null=("d",)), "null descriptor")]
        tried += [(sampled, dict(null=(name,)), "required buffer is NULL") for name in NAMES[2:8]]
        tried += [(sampled, dict(n_free=nf), "n_free") for nf in (0, 13, -1)]
        tried += [(sampled, dict(n_params=npar), "n_params") for npar in (0, 13)]
        tried += [(sampled, dict(free_idx=(1, bad)), "free index") for bad in (-1, 12)]
        tried += [(sampled, dict(lo=(2, 3.0), hi=(2, 2.0)), "lo > hi"), (sampled, dict(lo=(1, nan)), "lo > hi"), (sampled, dict(hi=(1, nan)), "lo > hi")]
        tried += [(sampled, dict(hi=(0, INF)), "infinite bound"), (fixed, dict(log_parameters=0, lo=(3, -INF)), "infinite bound")]
        tried += [(sampled, dict(lo=(0, lo)), "positive bounds") for lo in (0.0, -1.0)]
        tried += [(sampled, dict(sigma_lo=0.0), "sigma_lo"), (sampled, dict(sigma_lo=-1.0), "sigma_lo"), (sampled, dict(sigma_lo=30.0), "sigma_lo"),
                  (sampled, dict(sigma_hi=INF), "sigma_lo"), (sampled, dict(sigma_lo=nan), "sigma_lo")]
        tried += [(fixed, dict(sigma=s), "fixed sigma") for s in (0.0, -0.1, nan, INF)]
        tried += [(sampled, dict(eta=eta), "eta") for eta in (0.5, 0.0, 1.0001, nan)]
        tried += [(sampled, dict(target_accept=ta), "target_accept") for ta in (0.0, 1.0, -0.2, nan)]
        tried += [(sampled, dict(thin=th), "thin") for th in (0, -1)]
        tried += [(sampled, {f: 0}, "must be positive") for f in ("n_chain", "n_active", "n_prot", "max_iter")]
        tried += [(sampled, dict(n_active=4), "must be positive")]
        for case, fields, text in tried:
            before = [t.numpy().copy() for t in M.start(case)]
            rc, msg, after = _call(capi, case, entry=entry, **fields)
            assert rc == ERR_ARG and entry in msg and text in msg, (fields, rc, msg)
            assert all(M.same_bits(a.numpy(), b) for a, b in zip(after, before)), fields
    for case, fields in ((fixed, dict(log_parameters=0, lo=(0, -1.0))), (sampled, dict(null=("samples",))), (sampled, dict(eta=1.0)),
                         (fixed, dict(sigma_lo=-1.0, sigma_hi=nan))):   # fine: a negative bound without the logarithm, no samples, eta = 1, sigma's bounds unused
        assert _call(capi, case, **fields)[0] == 0, fields


# ---- the step's algebra against the numpy statement ----

def _views(capi, state, case):
    return capi.mcmc_state_views(state, case["nf"], case["ss"])


def _seed(n, ss, P, log, K):
    return 1000 * n + 100 * ss + 10 * P + K + int(log)


@pytest.mark.parametrize("K", [1, 5])
@pytest.mark.parametrize("log", [False, True])
@pytest.mark.parametrize("P", [1, 3])
@pytest.mark.parametrize("n,ss", M.DIMS)
def test_step_algebra(ion, n, ss, P, log, K):
    """Every call of a drawn sequence: from the library's state before it, the numpy statement's state after it, compared with the
    library's.  (n, ss) runs over the coordinates 1, 4, 12, 13 with sigma fixed and sampled where 1 <= n - ss <= 12 free parameters remain.)

    Rounding bounds.  A sum of k products of stored numbers differs from any other order of it by at most k eps times the sum of the
    terms' magnitudes, and the library's exp and log are within 2 ulp of numpy's.  lp: three terms.  mu, C, log_lambda: three terms
    each, gamma carrying exp and log's 4 ulp.  The proposal goes through the Cholesky factor, whose computed form satisfies
    |L L^T - A| <= (n + 1) eps |L| |L|^T (Higham, Accuracy and Stability, theorem 10.3), so two factorisations of one matrix differ by that
    backward error times the condition of A; ut adds n products per coordinate."""
    capi = ion.capi
    case = M.draw(_seed(n, ss, P, log, K), K, n, P, log=log, ss=ss)
    d = case["desc"]
    snaps = M.run_sequence(case)
    init = M.start(case)
    before = _views(capi, init[0].numpy(), case)
    iters_before = init[2].numpy()
    ulo, uhi, xlo, xhi = M.box(case)
    accepted, margins, worst = 0, [], {}
    for t, ev in enumerate(case["evals"]):
        S = M.values(case, ev)
        after = _views(capi, snaps[t][0], case)
        assert (snaps[t][1] == 0).all() and (snaps[t][2][:, 0] == t + 1).all()
        for c in range(K):
            b = M.state_dict(before, c)
            want, info = M.step(case, b, c, t, S[c])
            assert info["flag"] == 0
            got = M.state_dict(after, c)
            if t:
                margins.append(info["margin"] / (1.0 + abs(info["lp_t"]) + abs(b["lp"])))
                assert snaps[t][2][c, 1] - iters_before[c, 1] == int(info["accept"]), (t, c)          # the decision
                assert abs(after["alpha"][c] - info["alpha"]) <= 4 * EPS
                accepted += int(info["accept"])
                if info["accept"]:
                    assert M.same_bits(got["u"], b["ut"]) and M.same_bits(got["x"], b["xt"])
                else:
                    assert M.same_bits(got["u"], b["u"]) and M.same_bits(got["x"], b["x"]) and got["lp"] == b["lp"]
            ls = abs(np.log(d.sigma)) if not ss else np.abs(b["ut"][-1])
            lp_scale = d.n_samples * ls + (0.5 * S[c] * np.exp(2 * ls) if np.isfinite(S[c]) else 0.0) + abs(b["lp"])
            u_scale = np.abs(got["u"]).max() + np.abs(b["mu"]).max()
            dd = np.abs(got["u"] - got["mu"]).max()
            cond = np.linalg.cond(want["C"] + d.epsilon * np.eye(n))
            lam = np.exp(got["log_lambda"])
            checks = {"lp": (got["lp"], want["lp"], 8 * EPS * (1.0 + lp_scale)),
                      "mu": (got["mu"], want["mu"], 8 * EPS * u_scale),
                      "C": (got["C"], want["C"], 8 * EPS * (np.abs(b["C"]).max() + dd * dd + 2 * u_scale * dd)),
                      "log_lambda": (got["log_lambda"], want["log_lambda"], 8 * EPS * (1.0 + abs(b["log_lambda"]))),
                      "L": (got["L"], want["L"], 4 * (n + 1) * EPS * cond * np.abs(want["L"]).max()),
                      "ut": (got["ut"], want["ut"], 4 * (n + 1) * EPS * (cond * np.abs(want["L"]).max() * np.abs(info["z"]).sum() + np.abs(got["u"]).max()))}
            for name, (g, w, bound) in checks.items():
                err = float(np.abs(np.asarray(g) - np.asarray(w)).max())
                worst[name] = max(worst.get(name, 0.0), err / bound)
                assert err <= bound, (name, t, c, err, bound)
            assert np.array_equal(got["C"], got["C"].T) and (np.triu(got["L"], 1) == 0).all()
            if t < case["desc"].adapt_start:
                assert M.same_bits(got["mu"], b["mu"]) and M.same_bits(got["C"], b["C"]) and got["log_lambda"] == 0.0
            assert got["outside"] == want["outside"] == (not ((got["ut"] >= ulo) & (got["ut"] <= uhi)).all())
            if not got["outside"]:
                assert np.allclose(got["xt"], M.to_x(case, got["ut"]), rtol=4 * EPS, atol=0) and (got["xt"] >= xlo).all() and (got["xt"] <= xhi).all()
            assert lam > 0
            row = snaps[t][4][c, t]
            assert M.same_bits(row, np.append(got["x"], got["lp"]))                                   # the record: in the parameters
        rows = np.tile(case["base"], (K * P, 1))
        rows[:, case["free"]] = np.repeat(after["xt"][:, :case["nf"]], P, axis=0)
        assert M.same_bits(snaps[t][3], rows)                                                         # the trial rows: sigma never enters
        before, iters_before = after, snaps[t][2]
    assert np.isnan(snaps[-1][4][:, M.CALLS:]).all()
    print("accepted", accepted, "of", 5 * K, "smallest margin", min(margins), "worst error over bound", {k: float("%.3g" % x) for k, x in worst.items()})
    # no case is left out: the numpy statement's own margins, with these seeds, are all above the issue's 1e-9 (1 + |lp_t| + |lp|)
    assert min(margins) >= 1e-9


def test_the_drawn_cases_accept_and_reject():
    """The numpy statement alone over the seeds of test_step_algebra: both decisions occur, often."""
    acc = tot = 0
    for n, ss in M.DIMS:
        case = M.draw(_seed(n, ss, 3, True, 5), 5, n, 3, log=True, ss=ss)
        for c in range(5):
            rows, a = M.reference_chain(lambda x: 3.0, case["x0"][c], case=case, chain=c, iters=5, scale=0.1)
            acc, tot = acc + a, tot + 5
    assert 0 < acc < tot


# ---- paths ----

def _frozen(snaps, t, who, case):
    """from call t on nothing of the flagged chains moves, and their trial rows repeat their current x"""
    capi = M.mods()[0]
    K, P, nf = case["K"], case["P"], case["nf"]
    for a, b in zip(snaps[t][:3], snaps[t + 1][:3]):
        assert M.same_bits(a[who], b[who])
    if snaps[t][4] is not None:
        assert M.same_bits(snaps[t][4][who], snaps[t + 1][4][who])
    x = _views(capi, snaps[t + 1][0], case)["x"]
    want = np.tile(case["base"], (K * P, 1))
    want[:, case["free"]] = np.repeat(x[:, :nf], P, axis=0)
    got = snaps[t + 1][3].reshape(K, P, -1)
    assert M.same_bits(got[who], want.reshape(K, P, -1)[who]) and M.same_bits(snaps[t][3].reshape(K, P, -1)[who], got[who])


def test_every_flag_is_reachable_and_a_stopped_chain_is_frozen(ion):
    capi = ion.capi
    paths = M.path_cases()
    every = np.arange(5)
    case, kw = paths["max_iter_2"]
    s = M.run_sequence(case, **kw)
    assert (s[1][1] == 0).all() and (s[2][1] == capi.MCMC_MAXITER).all() and (s[2][2][:, 0] == 2).all()
    assert np.isfinite(s[2][4][:, :3]).all() and np.isnan(s[-1][4][:, 3:]).all()       # rows 0, 1, 2 recorded, nothing after
    for t in (2, 3, 4):
        _frozen(s, t, every, case)
    case, kw = paths["bad_start"]
    s = M.run_sequence(case, **kw)
    assert s[0][1].tolist() == [0, 0, capi.MCMC_NONFINITE, capi.MCMC_NONFINITE, 0] and (s[0][2][[2, 3]] == 0).all()
    v = _views(capi, s[0][0], case)
    assert (v["lp"][[2, 3]] == -INF).all() and np.isfinite(v["lp"][[0, 1, 4]]).all()
    _frozen(s, 0, np.array([2, 3]), case)
    assert (s[-1][1][[0, 1, 4]] == 0).all() and (s[-1][2][[0, 1, 4], 0] == M.CALLS).all()
    case, kw = paths["start_outside"]
    s = M.run_sequence(case, **kw)
    assert s[0][1].tolist() == [0, 0, 0, 0, capi.MCMC_NONFINITE] and np.isfinite(_views(capi, s[0][0], case)["lp"][4])
    _frozen(s, 0, np.array([4]), case)
    case, kw = paths["degenerate"]
    s = M.run_sequence(case, **kw)
    assert (s[0][1] == capi.MCMC_DEGENERATE).all() and (_views(capi, s[0][0], case)["L"] == 0).all()
    _frozen(s, 0, every, case)
    # ... and a covariance that stops being finite on the way: the chain is flagged at the call that sees it, the factor stays
    case, _ = paths["plain"]
    _, mc = M.mods()
    desc = capi.IonodeMcmcDesc.from_buffer_copy(case["desc"])
    state, flag, iters, trial, smp = M.start(case)
    feed = [(torch.from_numpy(e["value"].copy()), torch.from_numpy(e["status"].copy())) for e in case["evals"]]
    mc.mcmc_step(desc, None, *feed[0], state, flag, iters, trial, smp)
    good = state.numpy().copy()
    _views(capi, state.numpy(), case)["log_lambda"][1] = INF
    _views(capi, state.numpy(), case)["C"][3, 2, 2] = -1.0
    mc.mcmc_step(desc, None, *feed[1], state, flag, iters, trial, smp)
    assert flag.tolist() == [0, capi.MCMC_DEGENERATE, 0, capi.MCMC_DEGENERATE, 0]
    assert M.same_bits(_views(capi, state.numpy(), case)["L"][[1, 3]], _views(capi, good, case)["L"][[1, 3]])
    assert np.isfinite(state.numpy()[[0, 2, 4]]).all()


def test_an_outside_proposal_is_rejected_without_its_value_and_a_failed_status_rejects(ion):
    capi = ion.capi
    paths = M.path_cases()
    case, kw = paths["corner"]
    s = M.run_sequence(case, **kw)
    K, P, nf = case["K"], case["P"], case["nf"]
    n_out = n_in = 0
    for t in range(M.CALLS - 1):
        b, a = _views(capi, s[t][0], case), _views(capi, s[t + 1][0], case)
        rows = np.tile(case["base"], (K * P, 1))
        rows[:, case["free"]] = np.repeat(np.where(b["outside"][:, None] != 0, b["x"], b["xt"])[:, :nf], P, axis=0)
        assert M.same_bits(s[t][3], rows)                        # outside: the rows repeat the current x
        for c in range(K):
            if b["outside"][c]:
                n_out += 1                                       # the value 0 would have been accepted with certainty
                assert a["alpha"][c] == 0.0 and s[t + 1][2][c, 1] == s[t][2][c, 1] and M.same_bits(a["u"][c], b["u"][c]) and a["lp"][c] == b["lp"][c]
                assert M.same_bits(b["xt"][c], b["x"][c])
            else:
                n_in += 1
                assert a["alpha"][c] == 1.0 and s[t + 1][2][c, 1] == s[t][2][c, 1] + 1 and M.same_bits(a["u"][c], b["ut"][c]) and a["lp"][c] == 0.0
    print("proposals outside the box", n_out, "inside", n_in)
    assert n_out >= 10 and n_in >= 1 and (s[-1][1] == 0).all()
    case, kw = paths["failed_status"]
    s = M.run_sequence(case, **kw)
    v0, v = _views(capi, s[0][0], case), _views(capi, s[-1][0], case)
    assert (s[-1][2][:, 1] == 0).all() and (s[-1][1] == 0).all() and (v["alpha"] == 0.0).all() and (v["outside"] == 0).all()
    assert M.same_bits(v["u"], v0["u"]) and M.same_bits(v["lp"], v0["lp"])
    assert (v["log_lambda"] < 0).all()                           # ... and the scale shrinks: alpha = 0 against the target


def test_thin_and_sample_cap_are_honoured_and_samples_may_be_null(ion):
    capi = ion.capi
    paths = M.path_cases()
    plain = M.run_sequence(*paths["plain"][:1])
    case, kw = paths["thin_2_cap_2"]
    s = M.run_sequence(case, **kw)
    assert s[-1][4].shape[1] == 2
    assert M.same_bits(s[-1][4][:, 0], plain[-1][4][:, 0]) and M.same_bits(s[-1][4][:, 1], plain[-1][4][:, 2])   # rows 0 and 2; 4 is beyond the cap
    none = M.run_sequence(*paths["no_samples"][:1], **paths["no_samples"][1])
    for a, b in zip(none, plain):
        assert a[4] is None and all(M.same_bits(x, y) for x, y in zip(a[:4], b[:4]))
    # the sampled sigma is recorded as sigma, and stays within its bounds
    sig = plain[-1][4][:, :M.CALLS, case["nf"]]
    assert (sig >= case["sigma_bounds"][0]).all() and (sig <= case["sigma_bounds"][1]).all()
    assert np.allclose(sig[:, 0], case["x0"][:, -1], rtol=0, atol=0)


# ---- independence ----

@pytest.mark.parametrize("n,P", [(4, 3), (13, 1), (1, 3)])
def test_a_chain_does_not_depend_on_its_company(ion, n, P):
    """Alone (its index carried by chain_base), inside K = 67, and through an active list (another slot order, a subset): the same bits."""
    capi = ion.capi
    ss = 1 if n == 13 else 0
    case = M.draw(23 + n, 67, n, P, log=True, ss=ss)
    whole = M.run_sequence(case)
    active = [66, 5, 0, 31, 64, 2, 17]
    listed = M.run_sequence(case, active=active)
    init = [t.numpy() for t in M.start(case)]
    for k in range(M.CALLS):
        for c in range(67):   # chains outside the list keep their initial state
            if c not in active:
                assert M.same_bits(listed[k][0][c], init[0][c]) and listed[k][1][c] == 0 and (listed[k][2][c] == 0).all()
                assert M.same_bits(listed[k][4][c], init[4][c])
        for s, c in enumerate(active):
            assert all(M.same_bits(listed[k][i][c], whole[k][i][c]) for i in (0, 1, 2, 4))
            assert M.same_bits(listed[k][3][s * P:(s + 1) * P], whole[k][3][c * P:(c + 1) * P])
    for c in (0, 5, 66):
        rows = slice(c * P, (c + 1) * P)
        d = capi.IonodeMcmcDesc.from_buffer_copy(case["desc"])
        d.n_chain, d.n_active, d.chain_base = 1, 1, c
        alone = dict(case, K=1, x0=case["x0"][c:c + 1], desc=d, evals=[{k: v[rows] for k, v in ev.items()} for ev in case["evals"]])
        single = M.run_sequence(alone)
        for k in range(M.CALLS):
            assert all(M.same_bits(single[k][i][0], whole[k][i][c]) for i in (0, 1, 2, 4)) and M.same_bits(single[k][3], whole[k][3][rows])
    d = capi.IonodeMcmcDesc.from_buffer_copy(case["desc"])
    d.seed = case["desc"].seed + 1
    assert not M.same_bits(M.run_sequence(dict(case, desc=d))[-1][0], whole[-1][0])        # the seed matters
