"""No GPU: the manifold-MALA step through its host mirror ionode_mala_step_host -- the per-chain routine the kernel runs, compiled for
the host.  Header / binding / library agreement, every refusal, the step's algebra on seeded cases against the numpy statement of
tests/mala_cases.py, the paths (flags, frozen chains, the box, failures, metrics that do not factor, thinning), and a chain's
independence of its company."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import mala_cases as M

ROOT = os.path.join(os.path.dirname(__file__), "..")
ENTRIES = ("ionode_mala_step", "ionode_mala_step_host")
ERR_ARG = -1
NAMES = ["d", "active", "sse", "jtr", "jtj", "status", "state", "flag", "iters", "trial", "samples"]
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
    lm = re.search(r"\bint\s+ionode_lm_step_host\s*\(([^;]*)\);", hdr).group(1).split(",")
    mc = re.search(r"\bint\s+ionode_mcmc_step_host\s*\(([^;]*)\);", hdr).group(1).split(",")
    assert [a.split()[-1].lstrip("*") for a in lm][1:6] == NAMES[1:6] and [a.split()[-1].lstrip("*") for a in mc][4:] == NAMES[6:]
    body = hdr[hdr.index("typedef struct ionode_mala_desc {"):hdr.index("} ionode_mala_desc;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names, sizes = [], 0
    for ctype, decl in re.findall(r"(int32_t|int64_t|double)\s+([^;]+);", body):
        for n in decl.split(","):
            names.append(re.sub(r"\[.*?\]", "", n).strip())
            sizes += (4 if ctype == "int32_t" else 8) * (capi.LM_MAX_FREE if "[" in n else 1)
    assert names == [f[0] for f in capi.IonodeMalaDesc._fields_] and sizes == C.sizeof(capi.IonodeMalaDesc)   # (no padding anywhere)
    assert names[-4:] == ["free_idx", "base", "lo", "hi"]                                                     # the box every step descriptor has
    const = dict(re.findall(r"#define IONODE_MALA_(\w+) (\S+)", hdr))
    assert len(const) == 11
    for k, v in const.items():
        assert float(v) == getattr(capi, "MALA_" + k), k
    assert set(capi.MALA_FLAG_TEXT) == set(range(4))
    assert capi.mala_state_doubles(4) == 6 + 20 + 16 and capi.mala_state_doubles(13) == 6 + 65 + 169
    st = np.zeros((3, capi.mala_state_doubles(5)))
    views = capi.mala_state_views(st, 4, 1)
    for k, name in enumerate(views):   # the views tile the state: writing k + 1 into view k leaves no word unwritten
        views[name][:] = k + 1
    assert (st == 0).sum() == 0 and sorted(np.unique(st).tolist()) == list(range(1, 13))
    assert views["L"].shape == (3, 5, 5) and views["grad"].shape == (3, 5)
    assert capi.mala_state_views(np.zeros((2, capi.mala_state_doubles(4))), 4, 0)["u"].shape == (2, 4)


def _call(capi, case, *, entry="ionode_mala_step_host", null=(), **fields):
    d = capi.IonodeMalaDesc.from_buffer_copy(case["desc"])
    for k, v in fields.items():
        if isinstance(v, tuple):
            getattr(d, k)[v[0]] = v[1]
        else:
            setattr(d, k, v)
    state, flag, iters, trial, samples = M.start(case)
    ev = case["evals"][0]
    a = dict(active=None, state=state, flag=flag, iters=iters, trial=trial, samples=samples, **{k: torch.from_numpy(v.copy()) for k, v in ev.items()})
    ptrs = [None if (n in null or a[n] is None) else C.c_void_p(a[n].data_ptr()) for n in NAMES[1:]]
    tail = (None,) if entry == "ionode_mala_step" else ()
    rc = getattr(capi.lib(), entry)(None if "d" in null else C.byref(d), *ptrs, *tail)
    return rc, capi.lib().ionode_grad_last_error().decode(), (state, flag, iters, trial, samples)


def test_refusals_come_before_anything_is_touched(ion):
    capi = ion.capi
    nan = float("nan")
    sampled, fixed = M.draw(0, 3, 5, 2, log=True, ss=1), M.draw(0, 3, 4, 2, log=True, ss=0)
    entries = ("ionode_mala_step_host",) if torch.cuda.is_available() else ENTRIES   # (with a device a call that slipped through would launch on host addresses)
    for entry in entries:
        tried = [(sampled, dict(null=("d",)), "null descriptor")]
        tried += [(sampled, dict(null=(name,)), "required buffer is NULL") for name in NAMES[2:10]]
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
        tried += [(sampled, dict(ridge=r), "ridge") for r in (-1e-9, nan, INF)]
        tried += [(sampled, dict(n_samples=ns), "n_samples") for ns in (0.0, -2.0, nan, INF)]
        tried += [(sampled, dict(thin=th), "thin") for th in (0, -1)]
        tried += [(sampled, {f: 0}, "must be positive") for f in ("n_chain", "n_active", "n_prot", "max_iter")]
        tried += [(sampled, dict(n_active=4), "must be positive")]
        for case, fields, text in tried:
            before = [t.numpy().copy() for t in M.start(case)]
            rc, msg, after = _call(capi, case, entry=entry, **fields)
            assert rc == ERR_ARG and entry in msg and text in msg, (fields, rc, msg)
            assert all(M.same_bits(a.numpy(), b) for a, b in zip(after, before)), fields
    for case, fields in ((fixed, dict(log_parameters=0, lo=(0, -1.0))), (sampled, dict(null=("samples",))), (sampled, dict(eta=1.0)),
                         (fixed, dict(sigma_lo=-1.0, sigma_hi=nan)), (sampled, dict(ridge=0.0))):
        assert _call(capi, case, **fields)[0] == 0, fields   # fine: a negative bound without the logarithm, no samples, eta = 1, sigma's bounds unused, no ridge


# ---- the step's algebra against the numpy statement ----

def _views(capi, state, case):
    return capi.mala_state_views(state, case["nf"], case["ss"])


def _abs_sums(case, ev):
    """the protocol sums of the magnitudes: what a sum over the protocols in another order may differ by, per eps"""
    return M.reduce(case, dict(sse=np.abs(ev["sse"]), jtr=np.abs(ev["jtr"]), jtj=np.abs(ev["jtj"]), status=ev["status"]))


def _bounds(case, d, b, want, info, t, P, gabs):
    """Rounding bounds of one call, stated from n (and P).  With c = n + P + 6:
    a sum of k products of stored numbers differs from another order of it by at most k eps times the sum of the magnitudes, and the
    library's exp and log are within 2 ulp of numpy's.  lp: three terms.  grad_j: P + 3 operations on sum_p |jtr| x_j / sigma^2.  G: the
    same on its entries, a relative perturbation (P + 6) eps; the computed Cholesky factor satisfies |L L^T - G| <= (n + 1) eps |L| |L|^T
    (Higham, Accuracy and Stability, theorem 10.3), so two factors of two such matrices differ by 4 c eps cond(G) max|L|.  ld sums n
    logarithms of the diagonal: n times that relative error, and 8 eps per term.  A triangular or a full solve with the factor carries
    the same c eps cond(G) relative error (theorem 8.5 with the factor's own), which bounds d = G^-1 grad, the drift and the step;
    v = L_t^T (u - mu_t) adds (n + 1) eps |L_t^T| |u - mu_t| and the rounding of u - mu_t itself, 4 eps (|u| + |ut|).  The ratio adds
    its four terms' own 8 eps.  log_eps inherits the ratio's bound through alpha = exp(min(ratio, 0)) <= 1, whose derivative is <= 1."""
    n = case["n"]
    c = n + P + 6
    out = {}
    taken = (t == 0 and info["flag"] == 0) or info["accept"]
    cond = np.linalg.cond(info["G_t"]) if info["ok"] else 1.0
    ue = b["u"] if t == 0 else b["ut"]
    ls = abs(ue[-1]) if case["ss"] else abs(np.log(d.sigma))
    S_term = 0.5 * info["S"] * np.exp(2 * ls) if np.isfinite(info["S"]) else 0.0
    lp_b = 8 * EPS * (1.0 + d.n_samples * ls + S_term)
    out["lp"] = lp_b if taken else 0.0
    ld_b = lambda Lf: 4 * n * c * EPS * cond + 8 * EPS * float((1.0 + np.abs(np.log(np.diag(Lf)))).sum())   # noqa: E731
    ratio_b = None
    if t and info["alpha"] is not None and "v" in info:
        Lt, v, eps = info["Lt"], info["v"], info["eps"]
        h = 0.5 * eps * eps
        r = b["u"] - (b["ut"] + h * info["dvec"])
        dr = 4 * EPS * (np.abs(b["u"]) + np.abs(b["ut"])) + 8 * c * EPS * cond * h * np.linalg.norm(info["dvec"])
        dv = np.abs(Lt).T @ dr + 8 * c * EPS * cond * (np.abs(Lt).T @ np.abs(r))
        dq = 2.0 * float(np.abs(v) @ dv) + 8 * n * EPS * info["q"]
        ratio_b = (lp_b + 8 * EPS * (1.0 + abs(info["lp_t"]) + abs(b["lp"]) + abs(b["lqf"]) + abs(info["ld_t"]) + n * abs(b["log_eps"]))
                   + ld_b(Lt) + dq / (2.0 * eps * eps))
    out["ratio"] = ratio_b
    le_b = 8 * EPS * (1.0 + abs(b["log_eps"])) + (0.0 if ratio_b is None else ratio_b)
    out["log_eps"] = le_b if t else 0.0
    if info["flag"] == 0:
        Lc = want["L"]
        condc = np.linalg.cond(Lc @ Lc.T)
        cc = max(cond, condc)
        scale = np.exp(-2 * ls) * (np.abs(b["xt"] if t else b["x"])[:case["nf"]] if case["log"] else 1.0)
        out["grad"] = 8 * c * EPS * np.max(gabs * scale) + (8 * EPS * (d.n_samples + 2 * S_term) if case["ss"] else 0.0) if taken else 0.0
        out["L"] = 4 * c * EPS * cond * np.abs(Lc).max() if taken else 0.0
        out["ld"] = ld_b(Lc) if taken else 0.0
        step = want["ut"] - want["u"]
        out["ut"] = (8 * c * EPS * cc + 4 * out["log_eps"]) * np.linalg.norm(step) + 4 * EPS * np.abs(want["u"]).max()
        out["lqf"] = out["ld"] + n * out["log_eps"] + 8 * EPS * (1.0 + abs(want["ld"]) + n * abs(want["log_eps"]) + float(info["z"] @ info["z"]))
    return out


def _algebra(ion, n, ss, P, log, K, assert_it=True):
    """Every call of a drawn sequence: from the library's state before it, the numpy statement's state after it, compared with the
    library's.  Returns (decisions, decisions left out because the statement's own margin is below the bound, accepted, worst error over bound)."""
    capi = ion.capi
    case = M.draw(M.case_seed(n, ss, P, log, K), K, n, P, log=log, ss=ss)
    d = case["desc"]
    snaps = M.run_sequence(case) if assert_it else None
    init = M.start(case)
    state = init[0].numpy()
    iters_before = init[2].numpy()
    ulo, uhi, xlo, xhi = M.box(case)
    decisions = left_out = accepted = 0
    worst = {}
    for t, ev in enumerate(case["evals"]):
        S, gx, Hx = M.reduce(case, ev)
        _, gabs, _ = _abs_sums(case, ev)
        before = _views(capi, state, case)
        if assert_it:
            after = _views(capi, snaps[t][0], case)
            assert (snaps[t][1] == 0).all() and (snaps[t][2][:, 0] == t + 1).all()
        nxt = state.copy()
        nv = _views(capi, nxt, case)
        for c in range(K):
            b = M.state_dict(before, c)
            want, info = M.step(case, b, c, t, S[c], gx[c], Hx[c])
            info["S"] = S[c]
            assert info["flag"] == 0
            bnd = _bounds(case, d, b, want, info, t, P, gabs[c])
            close = False
            if t:
                decisions += 1
                accepted += int(info["accept"])
                close = bnd["ratio"] is not None and info["margin"] < bnd["ratio"]
                left_out += int(close)
            if not assert_it:       # the statement alone: it carries its own chain forward
                for k in ("u", "ut", "x", "xt", "grad", "L"):
                    nv[k][c] = want[k]
                for k in ("lp", "log_eps", "ld", "lqf"):
                    nv[k][c] = want[k]
                nv["outside"][c] = float(want["outside"])
                continue
            if close:
                continue
            got = M.state_dict(after, c)
            if t:
                assert snaps[t][2][c, 1] - iters_before[c, 1] == int(info["accept"]), (t, c)          # the decision
                assert abs(after["alpha"][c] - info["alpha"]) <= 4 * EPS + bnd["ratio"] if bnd["ratio"] is not None else after["alpha"][c] == 0.0
                if info["accept"]:
                    assert M.same_bits(got["u"], b["ut"]) and M.same_bits(got["x"], b["xt"])
                else:
                    assert M.same_bits(got["u"], b["u"]) and M.same_bits(got["x"], b["x"]) and got["lp"] == b["lp"]
                    assert M.same_bits(got["L"], b["L"]) and M.same_bits(got["grad"], b["grad"]) and got["ld"] == b["ld"]
            for name in ("lp", "log_eps", "grad", "L", "ld", "ut", "lqf"):
                err = float(np.abs(np.asarray(got[name]) - np.asarray(want[name])).max())
                if bnd[name] > 0:
                    worst[name] = max(worst.get(name, 0.0), err / bnd[name])
                assert err <= bnd[name], (name, t, c, err, bnd[name])
            assert (np.triu(got["L"], 1) == 0).all()
            assert got["outside"] == want["outside"] == (not ((got["ut"] >= ulo) & (got["ut"] <= uhi)).all())
            if not got["outside"]:
                assert np.allclose(got["xt"], M.to_x(case, got["ut"]), rtol=4 * EPS, atol=0) and (got["xt"] >= xlo).all() and (got["xt"] <= xhi).all()
            row = snaps[t][4][c, t]
            assert M.same_bits(row, np.append(got["x"], got["lp"]))                                   # the record: in the parameters
        if assert_it:
            rows = np.tile(case["base"], (K * P, 1))
            rows[:, case["free"]] = np.repeat(after["xt"][:, :case["nf"]], P, axis=0)
            assert M.same_bits(snaps[t][3], rows)                                                     # the trial rows: sigma never enters
            state, iters_before = snaps[t][0], snaps[t][2]
        else:
            state = nxt
    if assert_it:
        assert np.isnan(snaps[-1][4][:, M.CALLS:]).all()
    return decisions, left_out, accepted, worst


GRID = [(n, ss, P, log, K) for n, ss in M.DIMS for P in (1, 3) for log in (False, True) for K in (1, 5)]


@pytest.fixture(scope="module")
def statement_alone(ion):
    """The numpy statement alone over the whole drawn set, before anything is asserted on the library: how many decisions have a
    margin |log w - log ratio| below their rounding bound (they may be left out: at most 1 in 50), and that both decisions occur."""
    tot = out = acc = 0
    for n, ss, P, log, K in GRID:
        dcs, lo, a, _ = _algebra(ion, n, ss, P, log, K, assert_it=False)
        tot, out, acc = tot + dcs, out + lo, acc + a
    print("numpy statement alone: decisions", tot, "accepted", acc, "left out for their margin", out)
    return tot, out, acc


def test_the_drawn_cases_accept_and_reject_and_few_margins_are_below_their_bounds(statement_alone):
    tot, out, acc = statement_alone
    assert tot == sum(5 * K for *_, K in GRID) and 50 * out <= tot
    assert 0.2 * tot < acc < 0.8 * tot


@pytest.mark.parametrize("K", [1, 5])
@pytest.mark.parametrize("log", [False, True])
@pytest.mark.parametrize("P", [1, 3])
@pytest.mark.parametrize("n,ss", M.DIMS)
def test_step_algebra(ion, statement_alone, n, ss, P, log, K):
    """(n, ss) runs over the issue's set (1,0), (2,1), (4,0), (5,1), (8,0), (12,0), (13,1); the bounds are _bounds'."""
    tot, out, _ = statement_alone
    assert 50 * out <= tot
    dcs, lo, acc, worst = _algebra(ion, n, ss, P, log, K)
    print("decisions", dcs, "accepted", acc, "left out", lo, "worst error over bound", {k: float("%.3g" % x) for k, x in worst.items()})


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
    assert (s[1][1] == 0).all() and (s[2][1] == capi.MALA_MAXITER).all() and (s[2][2][:, 0] == 2).all()
    assert np.isfinite(s[2][4][:, :3]).all() and np.isnan(s[-1][4][:, 3:]).all()       # rows 0, 1, 2 recorded, nothing after
    for t in (2, 3, 4):
        _frozen(s, t, every, case)
    case, kw = paths["bad_start"]
    s = M.run_sequence(case, **kw)
    assert s[0][1].tolist() == [0, 0, capi.MALA_NONFINITE, capi.MALA_NONFINITE, 0] and (s[0][2][[2, 3]] == 0).all()
    v = _views(capi, s[0][0], case)
    assert (v["lp"][[2, 3]] == -INF).all() and np.isfinite(v["lp"][[0, 1, 4]]).all() and (v["L"][[2, 3]] == 0).all()
    _frozen(s, 0, np.array([2, 3]), case)
    assert (s[-1][1][[0, 1, 4]] == 0).all() and (s[-1][2][[0, 1, 4], 0] == M.CALLS).all()
    case, kw = paths["start_outside"]
    s = M.run_sequence(case, **kw)
    assert s[0][1].tolist() == [0, 0, 0, 0, capi.MALA_NONFINITE] and np.isfinite(_views(capi, s[0][0], case)["lp"][4])
    _frozen(s, 0, np.array([4]), case)
    case, kw = paths["degenerate_start"]                  # J^T J = 0 with ridge 0, and a NaN entry: the start's metric does not factor
    s = M.run_sequence(case, **kw)
    v = _views(capi, s[0][0], case)
    assert s[0][1].tolist() == [0, capi.MALA_DEGENERATE, 0, capi.MALA_DEGENERATE, 0] and (v["L"][[1, 3]] == 0).all() and np.isfinite(v["lp"]).all()
    assert (v["grad"][[1, 3]] == 0).all() and (s[0][2][[1, 3]] == 0).all()
    _frozen(s, 0, np.array([1, 3]), case)
    assert (s[-1][1][[0, 2, 4]] == 0).all()
    # ... and with the default ridge a zero J^T J factors (the floor keeps the diagonal positive), so only the NaN stops its chain
    s = M.run_sequence(M.with_desc(case, ridge=2.0 ** -20), **kw)
    assert s[0][1].tolist() == [0, 0, 0, capi.MALA_DEGENERATE, 0]


def test_a_trial_metric_that_does_not_factor_is_a_rejection_and_leaves_the_stored_factor(ion):
    capi = ion.capi
    case, kw = M.path_cases()["bad_trial_metric"]
    s = M.run_sequence(case, **kw)
    assert all((snap[1] == 0).all() for snap in s)                              # nobody stops
    for t in (1, 2, 3):
        b, a = _views(capi, s[t - 1][0], case), _views(capi, s[t][0], case)
        for c in (1, 3):                                                        # S = 0 there: without the metric's failure a certain acceptance
            assert a["alpha"][c] == 0.0 and s[t][2][c, 1] == s[t - 1][2][c, 1] and b["outside"][c] == 0.0
            for name in ("u", "x", "grad", "L"):
                assert M.same_bits(a[name][c], b[name][c]), name
            assert a["lp"][c] == b["lp"][c] and a["ld"][c] == b["ld"][c] and a["log_eps"][c] < b["log_eps"][c]
            assert not M.same_bits(a["ut"][c], b["ut"][c])                      # ... and the chain goes on proposing
    assert np.isfinite(s[-1][0]).all() and (s[-1][2][:, 0] == M.CALLS).all()
    assert (s[-1][2][[1, 3], 1] <= 2).all() and s[-1][2][:, 1].sum() > 0


def test_an_outside_proposal_is_rejected_without_its_values_and_a_failed_status_rejects(ion):
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
                n_out += 1                                       # the sum 0 would have been accepted with certainty
                assert a["alpha"][c] == 0.0 and s[t + 1][2][c, 1] == s[t][2][c, 1] and M.same_bits(a["u"][c], b["u"][c]) and a["lp"][c] == b["lp"][c]
                assert M.same_bits(b["xt"][c], b["x"][c]) and M.same_bits(a["L"][c], b["L"][c]) and M.same_bits(a["grad"][c], b["grad"][c])
            else:
                n_in += 1
    print("proposals outside the box", n_out, "inside", n_in)
    assert n_out >= 10 and (s[-1][1] == 0).all()
    case, kw = paths["failed_status"]
    s = M.run_sequence(case, **kw)
    v0, v = _views(capi, s[0][0], case), _views(capi, s[-1][0], case)
    assert (s[-1][2][:, 1] == 0).all() and (s[-1][1] == 0).all() and (v["alpha"] == 0.0).all() and (v["outside"] == 0).all()
    assert M.same_bits(v["u"], v0["u"]) and M.same_bits(v["lp"], v0["lp"]) and M.same_bits(v["L"], v0["L"])
    assert (v["log_eps"] < 0).all()                              # ... and the step shrinks: alpha = 0 against the target


def test_thin_and_sample_cap_are_honoured_and_samples_may_be_null(ion):
    paths = M.path_cases()
    plain = M.run_sequence(*paths["plain"][:1])
    case, kw = paths["thin_2_cap_2"]
    s = M.run_sequence(case, **kw)
    assert s[-1][4].shape[1] == 2
    assert M.same_bits(s[-1][4][:, 0], plain[-1][4][:, 0]) and M.same_bits(s[-1][4][:, 1], plain[-1][4][:, 2])   # rows 0 and 2; 4 is beyond the cap
    none = M.run_sequence(*paths["no_samples"][:1], **paths["no_samples"][1])
    for a, b in zip(none, plain):
        assert a[4] is None and all(M.same_bits(x, y) for x, y in zip(a[:4], b[:4]))
    sig = plain[-1][4][:, :M.CALLS, case["nf"]]                  # the sampled sigma is recorded as sigma, and stays within its bounds
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
        d = capi.IonodeMalaDesc.from_buffer_copy(case["desc"])
        d.n_chain, d.n_active, d.chain_base = 1, 1, c
        alone = dict(case, K=1, x0=case["x0"][c:c + 1], desc=d, evals=[{k: v[rows] for k, v in ev.items()} for ev in case["evals"]])
        single = M.run_sequence(alone)
        for k in range(M.CALLS):
            assert all(M.same_bits(single[k][i][0], whole[k][i][c]) for i in (0, 1, 2, 4)) and M.same_bits(single[k][3], whole[k][3][rows])
    d = capi.IonodeMalaDesc.from_buffer_copy(case["desc"])
    d.seed = case["desc"].seed + 1
    assert not M.same_bits(M.run_sequence(dict(case, desc=d))[-1][0], whole[-1][0])        # the seed matters
