"""No GPU: the ensemble step through its host mirror ionode_ensemble_step_host -- the per-ensemble routine the kernel runs, compiled
for the host.  Header / binding / library agreement, every refusal, the step's algebra on seeded cases against the numpy statement of
tests/ensemble_cases.py, the paths (flags, frozen ensembles, the box, failures, thinning, the iteration cap), an ensemble's independence
of its company, and the moves' affine invariance, bit for bit."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import ensemble_cases as N

ROOT = os.path.join(os.path.dirname(__file__), "..")
ENTRIES = ("ionode_ensemble_step", "ionode_ensemble_step_host")
ERR_ARG = -1
NAMES = ["d", "value", "status", "state", "flag", "iters", "accepted", "trial", "samples"]
EPS = N.EPS
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
    body = hdr[hdr.index("typedef struct ionode_ensemble_desc {"):hdr.index("} ionode_ensemble_desc;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names, sizes = [], 0
    for ctype, decl in re.findall(r"(int32_t|int64_t|double)\s+([^;]+);", body):
        for n in decl.split(","):
            names.append(re.sub(r"\[.*?\]", "", n).strip())
            sizes += (4 if ctype == "int32_t" else 8) * (capi.LM_MAX_FREE if "[" in n else 1)
    assert names == [f[0] for f in capi.IonodeEnsembleDesc._fields_] and sizes == C.sizeof(capi.IonodeEnsembleDesc)   # (no padding anywhere)
    assert names[:12] == ["n_ens", "n_walkers", "n_prot", "n_params", "n_free", "log_parameters", "sample_sigma", "max_iter", "thin", "sample_cap",
                          "ensemble_base", "move"]
    const = dict(re.findall(r"#define IONODE_ENSEMBLE_(\w+) (\S+)", hdr))
    assert len(const) == 10
    for k, v in const.items():
        assert float(v) == getattr(capi, "ENSEMBLE_" + k), k
    assert capi.ENSEMBLE_MAX_WALKERS >= 1024 and set(capi.ENSEMBLE_FLAG_TEXT) == set(range(3)) and capi.ENSEMBLE_MOVES == {"stretch": 0, "de": 1}
    assert capi.ensemble_state_doubles(4) == 19 and capi.ensemble_state_doubles(13) == 55
    st = np.zeros((3, 6, capi.ensemble_state_doubles(5)))
    views = capi.ensemble_state_views(st, 4, 1)
    for k, name in enumerate(views):   # the views tile the state: writing k + 1 into view k leaves no word unwritten
        views[name][:] = k + 1
    assert (st == 0).sum() == 0 and sorted(np.unique(st).tolist()) == list(range(1, 8))
    assert views["xt"].shape == (3, 6, 5) and views["lp"].shape == (3, 6)
    assert (N.ROLE_ASK, N.ROLE_ACCEPT, N.ROLE_JITTER, N.ROLE_SPREAD) == (capi.ENSEMBLE_ROLE_ASK, capi.ENSEMBLE_ROLE_ACCEPT, capi.ENSEMBLE_ROLE_JITTER,
                                                                        capi.ENSEMBLE_ROLE_SPREAD)


def _call(capi, case, *, entry="ionode_ensemble_step_host", null=(), **fields):
    d = capi.IonodeEnsembleDesc.from_buffer_copy(case["desc"])
    for k, v in fields.items():
        if isinstance(v, tuple):
            getattr(d, k)[v[0]] = v[1]
        else:
            setattr(d, k, v)
    state, flag, iters, accepted, trial, samples = N.start(case)
    rows = trial.shape[0]
    a = dict(value=torch.ones(rows, dtype=torch.float64), status=torch.zeros(rows, dtype=torch.int32), state=state, flag=flag, iters=iters,
             accepted=accepted, trial=trial, samples=samples)
    ptrs = [None if (n in null or a[n] is None) else C.c_void_p(a[n].data_ptr()) for n in NAMES[1:]]
    tail = (None,) if entry == "ionode_ensemble_step" else ()
    rc = getattr(capi.lib(), entry)(None if "d" in null else C.byref(d), *ptrs, *tail)
    return rc, capi.lib().ionode_grad_last_error().decode(), (state, flag, iters, accepted, trial, samples)


def test_refusals_come_before_anything_is_touched(ion):
    capi = ion.capi
    nan = float("nan")
    sampled, fixed = N.draw(0, 2, 12, 5, 2, log=True, ss=1, move="stretch"), N.draw(0, 2, 10, 4, 2, log=True, ss=0, move="de")
    one = N.draw(0, 2, 4, 1, 2, log=True, ss=0, move="stretch")
    entries = ("ionode_ensemble_step_host",) if torch.cuda.is_available() else ENTRIES   # (with a device a call that slipped through would launch on host addresses)
    for entry in entries:
        tried = [(sampled, dict(null=("d",)), "null descriptor")]
        tried += [(sampled, dict(null=(name,)), "required buffer is NULL") for name in NAMES[1:8]]
        tried += [(sampled, dict(n_free=nf), "n_free") for nf in (0, 13, -1)]
        tried += [(sampled, dict(n_params=npar), "n_params") for npar in (0, 13)]
        tried += [(sampled, dict(free_idx=(1, bad)), "free index") for bad in (-1, 12)]
        tried += [(sampled, dict(lo=(2, 3.0), hi=(2, 2.0)), "lo > hi"), (sampled, dict(lo=(1, nan)), "lo > hi"), (sampled, dict(hi=(1, nan)), "lo > hi")]
        tried += [(sampled, dict(hi=(0, INF)), "infinite bound"), (fixed, dict(log_parameters=0, lo=(3, -INF)), "infinite bound")]
        tried += [(sampled, dict(lo=(0, lo)), "positive bounds") for lo in (0.0, -1.0)]
        tried += [(sampled, dict(sigma_lo=0.0), "sigma_lo"), (sampled, dict(sigma_lo=-1.0), "sigma_lo"), (sampled, dict(sigma_lo=30.0), "sigma_lo"),
                  (sampled, dict(sigma_hi=INF), "sigma_lo"), (sampled, dict(sigma_lo=nan), "sigma_lo")]
        tried += [(fixed, dict(sigma=s), "fixed sigma") for s in (0.0, -0.1, nan, INF)]
        tried += [(sampled, dict(thin=th), "thin") for th in (0, -1)]
        tried += [(sampled, {f: 0}, "must be positive") for f in ("n_ens", "n_prot", "max_iter")]
        tried += [(sampled, dict(max_iter=1 << 30), "2^30")]
        tried += [(sampled, dict(n_walkers=11), "odd"), (sampled, dict(n_walkers=13), "odd"), (sampled, dict(n_walkers=-2), "odd")]
        tried += [(sampled, dict(n_walkers=10), "affinely span"), (fixed, dict(n_walkers=8), "affinely span"), (sampled, dict(n_walkers=0), "affinely span")]
        tried += [(one, dict(n_walkers=2, move=1), "two partners"), (one, dict(n_walkers=2), "affinely span"), (sampled, dict(n_walkers=capi.ENSEMBLE_MAX_WALKERS + 2), "above")]
        tried += [(sampled, dict(a=a), "stretch scale") for a in (1.0, 0.5, -2.0, nan, INF)]
        tried += [(fixed, dict(gamma=g), "gamma") for g in (nan, INF, -INF)]
        tried += [(fixed, dict(jitter=j), "jitter") for j in (-1e-9, nan, INF)]
        tried += [(sampled, dict(move=m), "unknown move") for m in (2, -1)]
        tried += [(sampled, dict(sample_cap=-1), "sample_cap"), (sampled, dict(n_samples=0.0), "n_samples"), (sampled, dict(n_samples=nan), "n_samples")]
        tried += [(sampled, dict(n_ens=1 << 28, n_prot=8), "rows")]
        for case, fields, text in tried:
            before = [t.numpy().copy() for t in N.start(case)]
            rc, msg, after = _call(capi, case, entry=entry, **fields)
            assert rc == ERR_ARG and entry in msg and text in msg, (fields, rc, msg)
            assert all(N.same_bits(a.numpy(), b) for a, b in zip(after, before)), fields
    # fine: a negative bound without the logarithm, no samples, jitter 0, gamma 0 or negative, the stretch's settings unused by DE, sigma's bounds unused
    for case, fields in ((fixed, dict(log_parameters=0, lo=(0, -1.0))), (sampled, dict(null=("samples",))), (fixed, dict(jitter=0.0)),
                         (fixed, dict(gamma=-0.5)), (fixed, dict(sigma_lo=-1.0, sigma_hi=nan)), (one, dict(move=1))):
        assert _call(capi, case, **fields)[0] == 0, fields


# ---- the step's algebra against the numpy statement ----

def _views(capi, state, case):
    return capi.ensemble_state_views(state, case["nf"], case["ss"])


def _seed(n, ss, P, log, E, extra, move):
    return 10000 * n + 1000 * ss + 100 * P + 10 * E + 2 * int(log) + 4 * int(extra > 0) + int(move == "de")


@pytest.mark.parametrize("extra", [0, 6])
@pytest.mark.parametrize("E", [1, 3])
@pytest.mark.parametrize("log", [False, True])
@pytest.mark.parametrize("P", [1, 3])
@pytest.mark.parametrize("move", N.MOVES)
@pytest.mark.parametrize("n,ss", N.DIMS)
def test_step_algebra(ion, n, ss, move, P, log, E, extra):
    """Four calls of a drawn sequence: from the library's state before a call, the numpy statement's state after it, compared with the
    library's.  W = 2 (n + 1), the least a descriptor may have, and six more.

    Rounding bounds.  The library's exp and log are within 2 ulp of libm's.  lp: three terms, one exp.  The stretch's ut is two
    operations on stored numbers and a z of four; the DE move's three products.  lq = (n - 1) log z.  Each is bounded by 8 eps times the
    sum of its terms' magnitudes.  u, x and lp of a told walker are COPIES of what the ask left: bit for bit."""
    capi = ion.capi
    W = 2 * (n + 1) + extra
    case = N.draw(_seed(n, ss, P, log, E, extra, move), E, W, n, P, log=log, ss=ss, move=move)
    H, nf, d = case["H"], case["nf"], case["desc"]
    snaps = N.run_sequence(case, calls=4)
    init = N.start(case)
    before, acc_before = _views(capi, init[0].numpy(), case), init[3].numpy()
    ulo, uhi, xlo, xhi = N.box(case)
    margins, accepted, told, outside, worst = [], 0, 0, 0, {}
    for t in range(4):
        ev = case["evals"][t]
        items = W if t == 0 else H
        S = N.sums(P, ev, E * items).reshape(E, items)
        state, flag, iters, acc, trial, smp = snaps[t]
        after = _views(capi, state, case)
        assert (flag == 0).all() and (iters[:, 0] == t + 1).all() and (iters[:, 1] == t // 2).all()
        for e in range(E):
            b = N.state_dict(before, e)
            want, info = N.step(case, b, e, t, S[e])
            got = N.state_dict(after, e)
            assert info["flag"] == 0
            for k, w in enumerate(info["told"]):
                if np.isfinite(info["margin"][k]):                                                        # (a proposal with alpha = 0 has no margin)
                    margins.append(info["margin"][k] / (1.0 + abs(info["lp_t"][k]) + abs(b["lp"][w]) + abs(b["lq"][w])))
                assert acc[e, w] - acc_before[e, w] == int(info["accept"][k]), (t, e, w)                 # the decision
                accepted, told = accepted + int(info["accept"][k]), told + 1
                if info["accept"][k]:
                    assert N.same_bits(got["u"][w], b["ut"][w]) and N.same_bits(got["x"][w], b["xt"][w])
                    ls = abs(b["ut"][w, nf]) if ss else abs(np.log(d.sigma))
                    scale = d.n_samples * ls + 0.5 * S[e][k] * np.exp(2 * ls)
                    assert abs(got["lp"][w] - want["lp"][w]) <= 8 * EPS * (1.0 + scale)
                else:
                    assert N.same_bits(got["u"][w], b["u"][w]) and N.same_bits(got["x"][w], b["x"][w]) and got["lp"][w] == b["lp"][w]
            rest = [w for w in range(W) if w not in info["told"]]
            assert N.same_bits(got["u"][rest], b["u"][rest]) and N.same_bits(got["x"][rest], b["x"][rest]) and (acc[e, rest] == acc_before[e, rest]).all()
            if t == 0:
                ls = np.abs(b["u"][:, nf]) if ss else abs(np.log(d.sigma))
                assert (np.abs(got["lp"] - want["lp"]) <= 8 * EPS * (1.0 + d.n_samples * ls + 0.5 * S[e] * np.exp(2 * ls))).all()
            asked = sorted(info["partners"])
            assert asked == list(range((t % 2) * H, (t % 2) * H + H))
            for w in asked:
                mag = np.abs(got["u"]).max() * (2.0 + 2.0 * d.a + 2.0 * abs(d.gamma)) + d.jitter * 10.0
                checks = {"ut": (got["ut"][w], want["ut"][w], 8 * EPS * mag), "lq": (got["lq"][w], want["lq"][w], 8 * EPS * (1.0 + abs(want["lq"][w])))}
                for name, (g, wnt, bound) in checks.items():
                    err = float(np.abs(np.asarray(g) - np.asarray(wnt)).max())
                    worst[name] = max(worst.get(name, 0.0), err / bound)
                    assert err <= bound, (name, t, e, w, err, bound)
                inside = bool(((got["ut"][w] >= ulo) & (got["ut"][w] <= uhi)).all())
                assert got["outside"][w] == want["outside"][w] == (0.0 if inside else 1.0)
                outside += int(not inside)
                if inside:
                    assert np.allclose(got["xt"][w], N.to_x(case, got["ut"][w]), rtol=4 * EPS, atol=0) and (got["xt"][w] >= xlo).all() and (got["xt"][w] <= xhi).all()
                else:
                    assert N.same_bits(got["xt"][w], got["x"][w])
            others = [w for w in range(W) if w not in asked]
            for name in ("ut", "xt", "lq", "outside"):
                assert N.same_bits(got[name][others], b[name][others]), name
            if t % 2 == 0:                                                                                # the record: in the parameters, all W
                assert N.same_bits(smp[e, :, t // 2], np.concatenate([got["x"], got["lp"][:, None]], axis=1))
        h = t % 2
        assert N.same_bits(trial[:E * H * P], N.trial_of(case, after["xt"][:, h * H:(h + 1) * H].reshape(E * H, n), E * H))   # sigma never enters
        before, acc_before = after, acc
    assert np.isnan(snaps[-1][5][:, :, 2:]).all()
    print("accepted", accepted, "of", told, "outside", outside, "smallest margin", min(margins), "worst error over bound", {k: float("%.3g" % x) for k, x in worst.items()})
    # no case is left out: the numpy statement's own margins, with these seeds, are far above what rounding could turn
    assert min(margins) >= 1e-9


def test_the_drawn_cases_accept_and_reject():
    """The numpy statement alone: both decisions occur, often, for both moves."""
    for move in N.MOVES:
        acc = tot = 0
        for n, ss in N.DIMS:
            case = N.draw(_seed(n, ss, 3, True, 1, 0, move), 1, 2 * (n + 1), n, 3, log=True, ss=ss, move=move)
            rows, a = N.reference_run(lambda x: 3.0 + x[0], case["x0"][0], case=case, iters=3)
            acc, tot = acc + a.sum(), tot + 3 * case["W"]
        assert 0.2 * tot < acc < 0.9 * tot, (move, acc, tot)


# ---- paths ----

def _frozen(snaps, t, who, case):
    """from call t on nothing of the flagged ensembles moves, and their H slots of the trial rows repeat the current x of half 0"""
    capi = N.mods()[0]
    E, H, P, n = case["E"], case["H"], case["P"], case["n"]
    for i in (0, 1, 2, 3, 5):
        if snaps[t][i] is not None:
            assert N.same_bits(snaps[t][i][who], snaps[t + 1][i][who]), i
    x = _views(capi, snaps[t + 1][0], case)["x"]
    want = N.trial_of(case, x[:, :H].reshape(E * H, n), E * H).reshape(E, H * P, -1)
    got = snaps[t + 1][4][:E * H * P].reshape(E, H * P, -1)
    assert N.same_bits(got[who], want[who]) and N.same_bits(snaps[t][4][:E * H * P].reshape(E, H * P, -1)[who], got[who])


def test_the_iteration_cap_comes_after_exactly_two_max_iter_plus_one_calls(ion):
    capi = ion.capi
    paths = N.path_cases()
    every = np.arange(3)
    case, kw = paths["max_iter_2"]
    s = N.run_sequence(case, **kw)
    assert all((s[t][1] == 0).all() for t in range(4)) and (s[4][1] == capi.ENSEMBLE_MAXITER).all()
    assert s[4][2].tolist() == [[4, 2]] * 3 and s[3][2].tolist() == [[4, 1]] * 3
    assert np.isfinite(s[4][5][:, :, :3]).all() and np.isnan(s[4][5][:, :, 3:]).all()                      # rows 0, 1, 2 recorded, nothing after
    plain = N.run_sequence(*paths["plain"][:1])
    views, pviews = _views(capi, s[4][0], case), _views(capi, plain[4][0], case)
    for name in ("u", "x", "lp"):
        assert N.same_bits(views[name], pviews[name])                                                       # the last call still tells half 1
    assert N.same_bits(s[4][3], plain[4][3]) and N.same_bits(views["ut"], _views(capi, s[3][0], case)["ut"])   # ... and asks nothing
    case, kw = paths["max_iter_1"]
    s = N.run_sequence(case, **kw)
    assert [int(x[1][0]) for x in s] == [0, 0, capi.ENSEMBLE_MAXITER, capi.ENSEMBLE_MAXITER, capi.ENSEMBLE_MAXITER]
    assert s[2][2].tolist() == [[2, 1]] * 3
    for t in (2, 3):
        _frozen(s, t, every, case)


def test_a_bad_start_freezes_only_its_own_ensemble(ion):
    capi = ion.capi
    paths = N.path_cases()
    plain = N.run_sequence(*paths["plain"][:1])
    for name, who in (("bad_start", 1), ("start_outside", 2)):
        case, kw = paths[name]
        s = N.run_sequence(case, **kw)
        want = [0, 0, 0]
        want[who] = capi.ENSEMBLE_NONFINITE
        assert s[0][1].tolist() == want and s[0][2][who].tolist() == [0, 0] and (s[0][3][who] == 0).all()
        lp = _views(capi, s[0][0], case)["lp"]
        assert np.isfinite(np.delete(lp, who, axis=0)).all()
        if name == "bad_start":
            assert lp[1, 7] == -INF and np.isfinite(np.delete(lp[1], 7)).all()                              # every lp is set all the same
        else:
            assert np.isfinite(lp[2]).all()
        assert np.isfinite(s[0][5][who, :, 0, :-1]).all() and np.isnan(s[-1][5][who, :, 1:]).all()          # row 0 is the starts'
        for t in range(N.CALLS - 1):
            _frozen(s, t, np.array([who]), case)
        others = [e for e in range(3) if e != who]
        assert (s[-1][1][others] == 0).all() and (s[-1][2][others, 0] == N.CALLS).all()
        if name == "bad_start":
            for i in (0, 1, 2, 3, 5):
                assert N.same_bits(s[-1][i][others], plain[-1][i][others])                                  # the others do not notice


def test_an_outside_proposal_is_rejected_without_its_value_and_a_failed_status_rejects(ion):
    capi = ion.capi
    paths = N.path_cases()
    case, kw = paths["corner"]
    s = N.run_sequence(case, **kw)
    E, H, P, n = case["E"], case["H"], case["P"], case["n"]
    n_out = n_in = 0
    for t in range(N.CALLS - 1):
        b, a = _views(capi, s[t][0], case), _views(capi, s[t + 1][0], case)
        h = t % 2
        half = slice(h * H, (h + 1) * H)
        pts = np.where(b["outside"][:, half, None] != 0, b["x"][:, half], b["xt"][:, half])
        assert N.same_bits(s[t][4][:E * H * P], N.trial_of(case, pts.reshape(E * H, n), E * H))          # outside: the rows repeat the current x
        for e in range(E):
            for w in range(h * H, (h + 1) * H):
                if b["outside"][e, w]:
                    n_out += 1                                                                             # the value 0 would have been accepted by many
                    assert s[t + 1][3][e, w] == s[t][3][e, w] and N.same_bits(a["u"][e, w], b["u"][e, w]) and a["lp"][e, w] == b["lp"][e, w]
                    assert N.same_bits(b["xt"][e, w], b["x"][e, w])
                else:
                    n_in += 1
    print("proposals outside the box", n_out, "inside", n_in)
    assert n_out >= 5 and n_in >= 5 and (s[-1][1] == 0).all() and s[-1][3].sum() > 0
    case, kw = paths["failed_status"]
    s = N.run_sequence(case, **kw)
    v0, v = _views(capi, s[0][0], case), _views(capi, s[-1][0], case)
    assert (s[-1][3] == 0).all() and (s[-1][1] == 0).all() and (v["outside"] == 0).all()
    assert N.same_bits(v["u"], v0["u"]) and N.same_bits(v["lp"], v0["lp"]) and not N.same_bits(v["ut"], v0["ut"])


def test_thin_and_sample_cap_are_honoured_and_samples_may_be_null(ion):
    paths = N.path_cases()
    case7 = N.with_desc(paths["plain"][0], max_iter=50)
    rng = np.random.default_rng(2)
    E, W, H, P = case7["E"], case7["W"], case7["H"], case7["P"]
    evals = list(case7["evals"]) + [dict(value=rng.uniform(1.0, 5.0, E * H * P) / P, status=np.zeros(E * H * P, dtype=np.int32)) for _ in range(4)]
    plain = N.run_sequence(case7, evals=evals)                                                              # nine calls: four full iterations
    s = N.run_sequence(N.with_desc(case7, thin=2, sample_cap=2), evals=evals)
    assert s[-1][5].shape[2] == 2 and np.isfinite(plain[-1][5][:, :, :5]).all()
    assert N.same_bits(s[-1][5][:, :, 0], plain[-1][5][:, :, 0]) and N.same_bits(s[-1][5][:, :, 1], plain[-1][5][:, :, 2])   # rows 0 and 2; 4 is beyond the cap
    for i in range(5):
        assert N.same_bits(s[-1][i], plain[-1][i])
    none = N.run_sequence(*paths["no_samples"][:1], **paths["no_samples"][1])
    short = N.run_sequence(*paths["plain"][:1])
    for a, b in zip(none, short):
        assert a[5] is None and all(N.same_bits(x, y) for x, y in zip(a[:5], b[:5]))
    # the sampled sigma is recorded as sigma, and stays within its bounds
    case = paths["plain"][0]
    sig = short[-1][5][:, :, :3, case["nf"]]
    assert (sig >= case["sigma_bounds"][0]).all() and (sig <= case["sigma_bounds"][1]).all()
    assert np.array_equal(sig[:, :, 0], case["x0"][:, :, -1])


# ---- independence ----

@pytest.mark.parametrize("move", N.MOVES)
@pytest.mark.parametrize("n,P", [(4, 3), (13, 1), (1, 3)])
def test_an_ensemble_does_not_depend_on_its_company(ion, n, P, move):
    """Ensemble e of a three-ensemble call, and the same ensemble alone with its index carried by ensemble_base: the same bits."""
    capi = ion.capi
    ss = 1 if n == 13 else 0
    W = 2 * (n + 1) + 2
    case = N.draw(23 + n, 3, W, n, P, log=True, ss=ss, move=move)
    whole = N.run_sequence(case)
    H = W // 2
    for e in range(3):
        d = capi.IonodeEnsembleDesc.from_buffer_copy(case["desc"])
        d.n_ens, d.ensemble_base = 1, e
        evals = [{k: v.reshape(3, -1)[e].copy() for k, v in ev.items()} for ev in case["evals"]]
        alone = dict(case, E=1, x0=case["x0"][e:e + 1], desc=d, evals=evals)
        single = N.run_sequence(alone)
        for k in range(N.CALLS):
            assert all(N.same_bits(single[k][i][0], whole[k][i][e]) for i in (0, 1, 2, 3, 5)), (e, k)
            assert N.same_bits(single[k][4][:H * P], whole[k][4][e * H * P:(e + 1) * H * P])
    d = capi.IonodeEnsembleDesc.from_buffer_copy(case["desc"])
    d.seed = case["desc"].seed + 1
    assert not N.same_bits(N.run_sequence(dict(case, desc=d))[-1][0], whole[-1][0])                         # the seed matters
    assert not N.same_bits(whole[-1][0][0], whole[-1][0][1])


# ---- affine invariance ----

def _quadratic_run(ion, move, scales, iters=30, E=2, W=12, n=4):
    """Linear parameters, S = (x / c - m)^T A (x / c - m) with the coordinates scaled by c: the chains of the scaled problem, divided by
    c.  Every scaled quantity is the unscaled one times a power of two, so each operation of the rule rounds alike."""
    capi, en = N.mods()
    rng = np.random.default_rng(8)
    G = rng.normal(size=(n, n))
    A = G @ G.T + n * np.eye(n)
    m = rng.uniform(-1.0, 1.0, n)
    c = np.asarray(scales, dtype=np.float64)
    x0 = (m + rng.normal(scale=0.5, size=(E, W, n))) * c
    free = [3, 0, 6, 5]

    def solver(model, params, prot_v, y0, t_eval, **kw):
        x = params.numpy()[:, free] / c
        val = np.array([float((r - m) @ A @ (r - m)) for r in x])
        return N.M.SimpleNamespace(sse=torch.from_numpy(val), sae=None, status=torch.zeros(len(val), dtype=torch.int32))

    smp, rate, flag, iters_ = en.sample(capi.MODEL_HH2, x0, np.zeros((1, 4)), np.zeros((1, 5)), np.arange(5.0), base_params=np.full(8, 9.0), free=free,
                                        log_parameters=False, bounds=((m - 8.0) * c, (m + 8.0) * c), sigma=1.0, move=move, jitter=0.0, seed=12,
                                        max_iter=iters, solver=solver, device="cpu", state_dtype=torch.float64)
    assert (flag.numpy() == capi.ENSEMBLE_MAXITER).all()
    s = smp.numpy().copy()
    s[..., :n] /= c
    return s, rate.numpy()


@pytest.mark.parametrize("move", N.MOVES)
def test_the_moves_are_affine_invariant_bit_for_bit(ion, move):
    """The sharp test of the move: scale every coordinate, its box and the target's precision by powers of two -- the chains scaled
    back are the unscaled run's bit for bit, the accept counters included.  (An adaptive-Metropolis chain with a fixed initial
    proposal scale could not pass this.)"""
    ref, ref_rate = _quadratic_run(ion, move, [1.0, 1.0, 1.0, 1.0])
    got, rate = _quadratic_run(ion, move, [2.0 ** 3, 2.0 ** -5, 2.0 ** 11, 2.0 ** -2])
    assert np.isfinite(ref).all() and 0.1 < ref_rate.mean() < 0.9
    assert N.same_bits(got, ref) and N.same_bits(rate, ref_rate)
    moved = (ref[:, :, 1:, :4] != ref[:, :, :-1, :4]).any(axis=3)
    assert moved.any(axis=2).all()                                                                            # every walker moved
