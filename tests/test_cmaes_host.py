"""No GPU: the CMA-ES step through its host mirror ionode_cmaes_step_host -- the phase functions the kernel runs, compiled for the
host.  Header / binding / library agreement, every refusal, the generator, one generation's algebra on seeded cases against the numpy
statement of tests/cmaes_cases.py, the stop flags, and convergence on analytic objectives."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

import cmaes_cases as L

ROOT = os.path.join(os.path.dirname(__file__), "..")
ENTRIES = ("ionode_cmaes_step", "ionode_cmaes_step_host")
ERR_ARG = -1
NAMES = ["d", "active", "value", "status", "state", "flag", "iters", "trial"]
EPS = L.EPS


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
    for entry in ("ionode_cmaes_draw_host", "ionode_cmaes_log_host"):
        assert entry in capi.EXPORTS and getattr(C.CDLL(capi.LIB_PATH), entry) is not None
    body = hdr[hdr.index("typedef struct ionode_cmaes_desc {"):hdr.index("} ionode_cmaes_desc;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names, sizes = [], 0
    for ctype, decl in re.findall(r"(int32_t|int64_t|double)\s+([^;]+);", body):
        for n in decl.split(","):
            names.append(re.sub(r"\[.*?\]", "", n).strip())
            sizes += (4 if ctype == "int32_t" else 8) * (capi.LM_MAX_FREE if "[" in n else 1)
    assert names == [f[0] for f in capi.IonodeCmaesDesc._fields_] and sizes == C.sizeof(capi.IonodeCmaesDesc)   # (no padding anywhere)
    const = dict(re.findall(r"#define IONODE_CMAES_(\w+) (\S+)", hdr))
    assert len(const) == 23
    for k, v in const.items():
        assert float(v) == getattr(capi, "CMAES_" + k), k
    assert set(capi.CMAES_FLAG_TEXT) == set(range(6))
    assert capi.cmaes_state_doubles(4, 8) == 12 + 32 + 48 + 16 + 64 and capi.cmaes_state_doubles(12, 64) == 2204
    assert [capi.cmaes_default_lambda(n) for n in (1, 4, 12)] == [4, 8, 11]
    st = np.zeros((3, capi.cmaes_state_doubles(5, 6)))
    views = capi.cmaes_state_views(st, 5, 6)
    for k, name in enumerate(views):   # the views tile the state: writing k into view k leaves no word unwritten but the rotation's three
        views[name][:] = k + 1
    assert (st == 0).sum() == 3 * 3 and views["pop"].shape == (3, 6, 5) and views["C"].shape == (3, 5, 5)


def _call(capi, case, *, entry="ionode_cmaes_step_host", null=(), **fields):
    d = capi.IonodeCmaesDesc.from_buffer_copy(case["desc"])
    for k, v in fields.items():
        if isinstance(v, tuple):
            getattr(d, k)[v[0]] = v[1]
        else:
            setattr(d, k, v)
    state, flag, iters, trial = L.start(case)
    rows = trial.shape[0]
    a = dict(active=None, value=torch.zeros(rows, dtype=torch.float64), status=torch.zeros(rows, dtype=torch.int32), state=state, flag=flag,
             iters=iters, trial=trial)
    ptrs = [None if (n in null or a[n] is None) else C.c_void_p(a[n].data_ptr()) for n in NAMES[1:]]
    tail = (None,) if entry == "ionode_cmaes_step" else ()
    rc = getattr(capi.lib(), entry)(None if "d" in null else C.byref(d), *ptrs, *tail)
    return rc, capi.lib().ionode_grad_last_error().decode(), (state, flag, iters, trial)


def test_refusals_come_before_anything_is_touched(ion):
    capi = ion.capi
    case = L.draw(0, 3, 4, 8, 2, log=True)
    before = [t.numpy().copy() for t in L.start(case)]
    entries = ("ionode_cmaes_step_host",) if torch.cuda.is_available() else ENTRIES   # (with a device a call that slipped through would launch on host addresses)
    for entry in entries:
        tried = [(dict(null=("d",)), "null descriptor")]
        tried += [(dict(null=(name,)), "required buffer is NULL") for name in NAMES[2:]]
        tried += [(dict(n_free=nf), "n_free") for nf in (0, 13, -1)]
        tried += [({"lambda": lam}, "lambda") for lam in (1, 65, 0, -3)]
        tried += [(dict(free_idx=(1, bad)), "free index") for bad in (-1, 8)]
        tried += [(dict(lo=(2, 3.0), hi=(2, 2.0)), "lo > hi"), (dict(lo=(1, float("nan"))), "lo > hi")]
        tried += [(dict(lo=(0, lo)), "positive bounds") for lo in (0.0, -1.0)]
        tried += [(dict(n_params=npar), "n_params") for npar in (0, 13)]
        tried += [({f: 0}, "must be positive") for f in ("n_run", "n_active", "n_prot", "max_iter", "unchanged_iters")]
        tried += [(dict(n_active=4), "must be positive")]
        for fields, text in tried:
            rc, msg, after = _call(capi, case, entry=entry, **fields)
            assert rc == ERR_ARG and entry in msg and text in msg, (fields, rc, msg)
            assert all(L.same_bits(a.numpy(), b) for a, b in zip(after, before)), fields
    rc, msg, _ = _call(capi, case, log_parameters=0, lo=(0, -1.0))   # a negative bound is fine without the logarithm
    assert rc == 0


# ---- the generator ----

def _philox_numpy(ctr, key):
    """An independent Philox4x32-10 on numpy uint64 arrays: ctr [N, 4], key [N, 2] -> [N, 4]."""
    c = [ctr[:, i].astype(np.uint64) for i in range(4)]
    k = [key[:, i].astype(np.uint64) for i in range(2)]
    m = np.uint64(0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k[0], p1 & m, (p0 >> np.uint64(32)) ^ c[3] ^ k[1], p0 & m]
        k = [(k[0] + np.uint64(0x9E3779B9)) & m, (k[1] + np.uint64(0xBB67AE85)) & m]
    return np.stack(c, axis=1)


def _draw(capi, seed, run, gen, cand, pair, attempt):
    w, z = (C.c_uint32 * 4)(), (C.c_double * 2)()
    capi.lib().ionode_cmaes_draw_host(int(seed), int(run), int(gen), int(cand), int(pair), int(attempt), C.byref(w), C.byref(z))
    return list(w), tuple(z)


def test_philox_words_against_two_independent_implementations_and_the_known_answer(ion):
    capi = ion.capi
    # Random123's known-answer vector for the all-zero counter and key (kat_vectors: philox4x32 10 rounds)
    assert _draw(capi, 0, 0, 0, 0, 0, 0)[0] == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    assert L.philox4x32([0, 0, 0, 0], [0, 0]) == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    rng = np.random.default_rng(1)
    idx = np.stack([rng.integers(0, 2 ** 31, 200), rng.integers(0, 2 ** 20, 200), rng.integers(0, 64, 200), rng.integers(0, 6, 200),
                    rng.integers(0, 9, 200)], axis=1)
    seeds = rng.integers(-2 ** 63, 2 ** 63, 200)
    useed = seeds.astype(np.uint64)
    ctr = np.stack([idx[:, 0], idx[:, 1], idx[:, 2], idx[:, 3] + 65536 * idx[:, 4]], axis=1)
    key = np.stack([useed & np.uint64(0xFFFFFFFF), useed >> np.uint64(32)], axis=1)
    want = _philox_numpy(ctr, key)
    for i in range(200):
        words, z = _draw(capi, seeds[i], *idx[i])
        assert words == want[i].tolist() == L.draw_words(seeds[i], *idx[i])
        assert z == L.normal_pair(seeds[i], *idx[i])          # the numpy statement's generator is the library's, bit for bit


def test_the_deterministic_logarithm(ion):
    capi = ion.capi
    log = capi.lib().ionode_cmaes_log_host
    rng = np.random.default_rng(2)
    x = np.concatenate([2.0 ** rng.uniform(-1074.0, 0.0, 20000), rng.uniform(0.0, 1.0, 20000), 1.0 - 2.0 ** rng.uniform(-53.0, -1.0, 5000),
                        rng.uniform(1.0, 64.5, 2000), [5e-324, 2.2250738585072014e-308, 1.0, 0.5, 2.0 ** -0.5, 2.0 ** 0.5]])
    got = np.array([log(float(v)) for v in x])
    want = np.log(x)
    ulp = np.abs(got - want) / np.spacing(np.abs(want))
    worst = float(ulp[want != 0].max())
    print("cm_log against numpy.log: worst difference", worst, "ulp over", x.size, "inputs")
    # measured on the CPU: 2.0 ulp at worst (the quotient s and the polynomial each round once, numpy.log itself is within 1 ulp); twice that
    assert worst <= 4.0 and log(1.0) == 0.0
    assert all(log(float(v)) == L.det_log(float(v)) for v in x[::37])
    assert log(0.0) == -np.inf and np.isnan(log(-1.0)) and np.isnan(log(float("nan"))) and log(float("inf")) == np.inf


def test_a_hundred_thousand_normal_deviates(ion):
    capi = ion.capi
    N = 100000
    z, u = np.empty(N), np.empty(N)
    for i in range(N // 2):
        words, pair = _draw(capi, 99, i // 640, 3, (i // 10) % 64, i % 10, 0)
        z[2 * i:2 * i + 2] = pair
        u[2 * i], u[2 * i + 1] = L.uniform(words[0], words[1]), L.uniform(words[2], words[3])
    assert (u > 0).all() and (u < 1).all() and np.isfinite(z).all()
    mean, var = z.mean(), z.var()
    skew, kurt = ((z - mean) ** 3).mean() / var ** 1.5, ((z - mean) ** 4).mean() / var ** 2 - 3.0
    se = np.sqrt(np.array([1.0, 2.0, 6.0, 24.0]) / N)          # standard errors of the four under N(0, 1)
    got = np.array([mean, var - 1.0, skew, kurt])
    print("moments", got.tolist(), "in standard errors", (got / se).tolist())
    assert (np.abs(got) <= 4.0 * se).all(), (got / se).tolist()
    ks = np.abs(np.sort(u) - (np.arange(N) + 0.5) / N).max()
    assert ks <= 1.95 / np.sqrt(N), ks                           # the uniforms: Kolmogorov's 0.1 % point
    special = pytest.importorskip("scipy.special")
    want = special.ndtri(u)
    err = np.abs(z - want) / np.maximum(np.abs(want), 1.0)
    print("PPND16 against scipy.special.ndtri: worst difference", float(err.max()), "relative to max(|z|, 1)")
    # measured on the CPU: 9.8e-16 at worst (AS241 claims about 1 part in 1e16 for the rational functions; q num / den adds three
    # roundings and ndtri has its own); twice that
    assert err.max() <= 2e-15


# ---- one generation's algebra ----

def _views(capi, state, case):
    return capi.cmaes_state_views(state, case["n"], case["lam"])


def _values(case, ev):
    """f [K, lam] from an evaluation's arrays, as the header states it."""
    K, lam, P = case["K"], case["lam"], case["P"]
    v, s = ev["value"].reshape(K, lam, P), ev["status"].reshape(K, lam, P)
    f = np.zeros((K, lam))
    for p in range(P):
        f = f + v[:, :, p]
    return np.where((s != 0).any(axis=2) | ~(f < np.inf), np.inf, f)


def _box(case):
    n = case["n"]
    lo = np.full(n, np.finfo(np.float64).tiny if case["log"] else -np.inf) if case["lo"] is None else case["lo"]
    hi = np.full(n, np.inf) if case["hi"] is None else case["hi"]
    log = lambda a: np.array([math.log(x) for x in a])   # noqa: E731  (libm's, as the library's entry points take it)
    return (log(lo), log(hi), lo, hi) if case["log"] else (lo, hi, lo, hi)


def _check_ask(capi, case, v, trial, runs, gen):
    """The points of generation `gen` in the state views v: the numpy statement's, bit for bit, inside the box, and the trial rows."""
    ulo, uhi, xlo, xhi = _box(case)
    n, lam, P = case["n"], case["lam"], case["P"]
    for c in runs:
        for k in range(lam):
            u, _, _ = L.ask_point(case["seed"], c, gen, k, v["m"][c], v["sigma"][c], v["B"][c], v["D"][c], ulo, uhi)
            assert L.same_bits(v["pop"][c, k], u), (c, k)
    assert (v["pop"] >= ulo).all() and (v["pop"] <= uhi).all() and (v["pop_x"] >= xlo).all() and (v["pop_x"] <= xhi).all()
    want_x = np.exp(v["pop"]) if case["log"] else v["pop"]
    assert np.allclose(v["pop_x"], want_x, rtol=4 * EPS, atol=0)
    rows = np.tile(case["base"], (case["K"] * lam * P, 1))
    rows[:, case["free"]] = np.repeat(v["pop_x"].reshape(-1, n), P, axis=0)
    assert L.same_bits(trial, rows)


@pytest.mark.parametrize("K", L.K_CASES)
@pytest.mark.parametrize("log", [False, True])
@pytest.mark.parametrize("P", L.P_CASES)
@pytest.mark.parametrize("which", [0, 1, 2])
@pytest.mark.parametrize("n", L.N_CASES)
def test_generation_algebra(ion, n, which, P, log, K):
    capi = ion.capi
    lam = L.lam_cases(n)[which]
    case = L.draw(1000 * n + 100 * which + 10 * P + K + int(log), K, n, lam, P, log=log)
    c = L.constants(n, lam)
    snaps = L.run_sequence(case)
    runs = sorted({0, K // 2, K - 1})
    v0 = _views(capi, snaps[0][0], case)
    assert (snaps[0][1] == 0).all() and (snaps[0][2] == [1, 0]).all()
    assert L.same_bits(v0["m"], np.log(case["x0"]) if log else case["x0"])
    _check_ask(capi, case, v0, snaps[0][3], runs, 0)
    worst = {}
    for t in (1, 2, 3):
        b, a = _views(capi, snaps[t - 1][0], case), _views(capi, snaps[t][0], case)
        f = _values(case, case["evals"][t - 1])
        assert L.same_bits(a["f"], f)                                                   # protocol sums, failures and NaNs: exact
        assert (snaps[t][1] == 0).all() and (snaps[t][2] == [t + 1, t * lam]).all()
        for r in runs:
            rk = L.ranks(f[r])
            assert L.same_bits(a["w"][r], np.where(rk < c["mu"], c["w"][np.minimum(rk, c["mu"] - 1)], 0.0))    # ranking with ties and infs: exact
            assert a["nfinite"][r] == np.isfinite(f[r]).sum()
            want = L.tell(dict(m=b["m"][r], sigma=b["sigma"][r], pc=b["pc"][r], ps=b["ps"][r], C=b["C"][r]), b["pop"][r], f[r], c, t)
            # Rounding bound: every quantity is a sum of at most lam + n products of stored numbers, each formed with a handful of
            # roundings, so it differs from any other summation order by at most 8 (lam + n) eps times the sum of the terms' magnitudes
            # (bounded here by the quantities' scale); p_sigma goes through C^-1/2, whose two forms (Jacobi's B D^-1 B^T, eigh's) differ by
            # eps times the condition of C on top.
            tol = 8 * (lam + n) * EPS
            y = np.abs(b["pop"][r] - b["m"][r][None]).max() / b["sigma"][r]
            cond = a["cond"][r] if t > 1 else 1.0
            cond_b = b["cond"][r] ** 2 if t > 1 else 1.0
            checks = {"m": (a["m"][r], want["m"], np.abs(b["m"][r]).max() + b["sigma"][r] * y),
                      "ps": (a["ps"][r], want["ps"], (np.abs(b["ps"][r]).max() + 3.0 * y * np.sqrt(cond_b)) * cond_b),
                      "pc": (a["pc"][r], want["pc"], np.abs(b["pc"][r]).max() + 3.0 * y),
                      "C": (a["C"][r], want["C"], np.abs(b["C"][r]).max() + 9.0 * y * y)}
            for name, (got, ref, scale) in checks.items():
                err = np.abs(got - ref).max() / (tol * scale)
                worst[name] = max(worst.get(name, 0.0), err)
                assert err <= 1.0, (name, t, r, err)
            assert abs(a["sigma"][r] - want["sigma"]) <= tol * (1.0 + np.abs(a["ps"][r]).max()) * want["sigma"] * max(cond_b, 1.0)
            assert a["hsig"][r] == want["hsig"] and L.same_bits(a["m_old"][r], b["m"][r]) and a["sigma_old"][r] == b["sigma"][r]
            assert np.array_equal(a["C"][r], a["C"][r].T)
            # Jacobi's backward error: a rotation perturbs the matrix by a few eps of its norm, an entry sees 2 (n - 1) rotations a
            # sweep, at most IONODE_CMAES_JACOBI_SWEEPS sweeps: 4 eps x 2 n x sweeps, in the Frobenius norm
            jac = 8 * n * capi.CMAES_JACOBI_SWEEPS * EPS
            B, D = a["B"][r], a["D"][r]
            e1 = np.linalg.norm((B * D ** 2) @ B.T - a["C"][r]) / np.linalg.norm(a["C"][r])
            e2 = np.linalg.norm(B.T @ B - np.eye(n))
            worst["BD2Bt"], worst["BtB"] = max(worst.get("BD2Bt", 0.0), e1 / jac), max(worst.get("BtB", 0.0), e2 / jac)
            assert e1 <= jac and e2 <= jac and (D > 0).all(), (e1, e2, jac)
            assert a["cond"][r] == D.max() / D.min()
            kb = int(np.argmin(f[r]))                                                   # (the first of equal minima)
            if f[r][kb] < b["best_f"][r]:
                assert a["best_f"][r] == f[r][kb] and L.same_bits(a["best_x"][r], b["pop_x"][r, kb])
            else:
                assert a["best_f"][r] == b["best_f"][r] and L.same_bits(a["best_x"][r], b["best_x"][r])
        _check_ask(capi, case, a, snaps[t][3], runs, t)
    print("worst error over bound:", {k: float("%.3g" % x) for k, x in worst.items()})


def _with(case, **fields):
    d = L.mods()[0].IonodeCmaesDesc.from_buffer_copy(case["desc"])
    for k, val in fields.items():
        setattr(d, k, val)
    return dict(case, desc=d)


def test_every_flag_is_reachable_and_a_stopped_run_is_frozen(ion):
    capi = ion.capi
    case = L.draw(11, 5, 4, 8, 3, log=True)
    rows = np.tile(case["base"], (5 * 8 * 3, 1))

    def frozen(snaps, t, who):
        """from call t on nothing of the flagged runs moves, and their trial rows repeat their best point"""
        for a, b in zip(snaps[t][:3], snaps[t + 1][:3]):
            assert L.same_bits(a[who], b[who])
        best = _views(capi, snaps[t + 1][0], case)["best_x"]
        want = rows.copy()
        want[:, case["free"]] = np.repeat(best, 8 * 3, axis=0)
        got = snaps[t + 1][3].reshape(5, 8 * 3, -1)
        assert L.same_bits(got[who], want.reshape(5, 8 * 3, -1)[who]) and L.same_bits(snaps[t][3].reshape(5, 24, -1)[who], got[who])

    every = np.arange(5)
    s = L.run_sequence(_with(case, max_iter=1))
    assert (s[0][1] == 0).all() and (s[1][1] == capi.CMAES_MAXITER).all() and (s[1][2] == [1, 8]).all()
    frozen(s, 1, every)
    s = L.run_sequence(_with(case, unchanged_iters=1, unchanged_threshold=1e300))
    assert (s[1][1] == 0).all() and (s[2][1] == capi.CMAES_UNCHANGED).all() and (s[2][2] == [2, 16]).all()
    frozen(s, 2, every)
    s = L.run_sequence(_with(case, unchanged_iters=2, unchanged_threshold=0.1))     # the values halve every generation: never unchanged
    assert (s[3][1] == 0).all() and (_views(capi, s[3][0], case)["unchanged"] == 0).all()
    s = L.run_sequence(_with(case, tolx=1e300))
    assert (s[1][1] == capi.CMAES_TOLX).all()
    frozen(s, 1, every)
    s = L.run_sequence(case, scale=np.array([1.0, 1e8, 1.0, 1.0]))
    assert (s[1][1] == capi.CMAES_CONDITION).all() and (_views(capi, s[1][0], case)["cond"] > capi.CMAES_CONDITION_LIMIT).all()
    frozen(s, 1, every)
    ev = [dict(value=e["value"].copy(), status=e["status"].copy()) for e in case["evals"]]
    st = ev[0]["status"].reshape(5, 8, 3)
    st[2, :, 1] = 2                       # run 2: nothing finite
    st[3, [0, 4, 6], 0] = 1               # run 3: with its failure of the draw and its NaN five of eight are out: three finite, mu = 4
    s = L.run_sequence(case, evals=ev)
    assert s[1][1].tolist() == [0, 0, capi.CMAES_NONFINITE, capi.CMAES_NONFINITE, 0]
    v0, v1 = _views(capi, s[0][0], case), _views(capi, s[1][0], case)
    assert np.isinf(v1["best_f"][2]) and np.isfinite(v1["best_f"][3]) and v1["nfinite"][2:4].tolist() == [0.0, 3.0]
    for name in ("m", "sigma", "pc", "ps", "C", "B", "D"):
        assert L.same_bits(v0[name][2:4], v1[name][2:4]), name
    frozen(s, 1, np.array([2, 3]))
    assert (s[3][1][[0, 1, 4]] == 0).all() and (s[3][2][[0, 1, 4]] == [4, 24]).all()


@pytest.mark.parametrize("n,lam,P", [(4, 8, 3), (12, 11, 1), (1, 2, 3), (12, 64, 1)])
def test_a_run_does_not_depend_on_its_company(ion, n, lam, P):
    """Alone (its index carried by run_base), inside K = 67, and through an active list (another slot order, a subset): the same bits."""
    capi = ion.capi
    case = L.draw(23 + n, 67, n, lam, P, log=True)
    whole = L.run_sequence(case)
    active = [66, 5, 0, 31, 64, 2, 17]
    listed = L.run_sequence(case, active=active)
    per = lam * P
    init = L.start(case)[0].numpy()
    for k in range(4):
        for c in range(67):   # runs outside the list keep their initial state
            if c not in active:
                assert L.same_bits(listed[k][0][c], init[c]) and listed[k][1][c] == 0 and (listed[k][2][c] == 0).all()
        for s, c in enumerate(active):
            assert L.same_bits(listed[k][0][c], whole[k][0][c]) and listed[k][1][c] == whole[k][1][c] and L.same_bits(listed[k][2][c], whole[k][2][c])
            assert L.same_bits(listed[k][3][s * per:(s + 1) * per], whole[k][3][c * per:(c + 1) * per])
    for c in (0, 5, 66):
        rows = slice(c * per, (c + 1) * per)
        d = capi.IonodeCmaesDesc.from_buffer_copy(case["desc"])
        d.n_run, d.n_active, d.run_base = 1, 1, c
        alone = dict(case, K=1, x0=case["x0"][c:c + 1], desc=d, evals=[{k: v[rows] for k, v in ev.items()} for ev in case["evals"]])
        single = L.run_sequence(alone)
        for k in range(4):
            assert L.same_bits(single[k][0][0], whole[k][0][c]) and single[k][1][0] == whole[k][1][c] and L.same_bits(single[k][3], whole[k][3][rows])


@pytest.mark.parametrize("log", [False, True])
def test_box_handling_redraws_then_clips(ion, log):
    """Starts on the box's upper corner with a step size of a third of the box's width: most first draws leave the box, redraws bring some back,
    the rest are clipped after IONODE_CMAES_RESAMPLES redraws -- as the numpy statement does it, bit for bit -- and no point leaves the box."""
    capi = ion.capi
    case = L.draw(31, 5, 4, 8, 1, log=log, bounds=True)
    case["x0"][:] = case["hi"]
    sigma0 = 0.6
    snaps = L.run_sequence(case, sigma0=sigma0)
    ulo, uhi, xlo, xhi = _box(case)
    attempts, clipped = [], []
    for t, gen in ((0, 0), (1, 1)):
        v = _views(capi, snaps[t][0], case)
        _check_ask(capi, case, v, snaps[t][3], range(5), gen)
        for c in range(5):
            for k in range(8):
                _, att, cl = L.ask_point(case["seed"], c, gen, k, v["m"][c], v["sigma"][c], v["B"][c], v["D"][c], ulo, uhi)
                attempts.append(att)
                clipped.append(cl)
    attempts, clipped = np.array(attempts), np.array(clipped)
    print("attempts beyond the first", np.bincount(attempts, minlength=9).tolist(), "clipped", int(clipped.sum()), "of", clipped.size)
    assert ((attempts > 0) & ~clipped).any() and clipped.any() and (attempts == 0).any()
    v = _views(capi, snaps[0][0], case)
    on_edge = (v["pop"] == ulo) | (v["pop"] == uhi)
    assert on_edge.any(axis=2).sum() >= clipped[:40].sum() > 0


# ---- convergence through the host step on analytic objectives ----

# Generations the numpy statement (cmaes_cases.reference_run: the same generator and formulas, numpy.linalg.eigh) needs from the same
# starts and seeds (seed 3, runs 0 .. 3) to bring the best value to 1e-10 of the start's, measured on the CPU; the budget of the host step
# is twice the largest, because another eigen-solver's rounding changes the path.  The host step itself needed (measured): sphere
# 83 / 87 / 77 / 87, ellipsoid 659 / 665 / 669 / 687, Rosenbrock 164 / 165 / 158 / 241.
CONVERGENCE = {
    # name: (objective, n, log parameters, start value of every coordinate, the numpy statement's generations per run)
    "sphere": (L.sphere, 4, False, 3.0, (89, 79, 94, 82)),
    "ellipsoid": (L.ellipsoid, 12, False, 3.0, (704, 654, 709, 560)),
    "rosenbrock": (L.rosenbrock, 4, True, 0.3, (167, 176, 432, 177)),
}


@pytest.mark.parametrize("name", sorted(CONVERGENCE))
def test_convergence_on_analytic_objectives(ion, name):
    capi = ion.capi
    _, cm = L.mods()
    fn, n, log, start, reference = CONVERGENCE[name]
    budget = 2 * max(reference)
    npar = 12 if n > 8 else 8
    model = capi.MODEL_MARKOV6 if npar == 12 else capi.MODEL_HH2
    free = list(range(n))
    x0 = np.full((4, n), start)
    f0 = fn(x0[0])
    lam = capi.cmaes_default_lambda(n)
    first = {}

    def watch(it, state, flag, iters):
        best = capi.cmaes_state_views(state, n, lam)["best_f"].numpy()
        for k in range(4):
            if best[k] <= 1e-10 * f0:
                first.setdefault(k, it)          # step `it` told generation it - 1: `it` generations told

    x, val, flag, iters = cm.minimise(model, x0, np.zeros((2, 10)), np.zeros((2, 5)), np.arange(5.0), base_params=np.ones(npar), free=free,
                                      log_parameters=log, solver=L.analytic_solver(fn, free, 2), max_iter=budget, unchanged_iters=10 ** 6,
                                      unchanged_threshold=0.0, tolx=0.0, seed=3, device="cpu", state_dtype=torch.float64, callback=watch,
                                      y0=(0.0, 1.0) if npar == 8 else (0.0,) * 6, compact_every=None)
    print(name, "generations to 1e-10 of the start's value:", [first.get(k) for k in range(4)], "numpy statement:", reference, "budget", budget)
    assert sorted(first) == [0, 1, 2, 3] and max(first.values()) <= budget
    assert (val.numpy() <= 1e-10 * f0).all() and np.allclose([fn(r) for r in x.numpy()], val.numpy(), rtol=1e-12, atol=0)


def test_the_numpy_statement_needs_what_the_budgets_say():
    """The recorded generation counts are the numpy statement's own (the cheap two of the three are re-measured here)."""
    for name in ("sphere", "rosenbrock"):
        fn, n, log, start, reference = CONVERGENCE[name]
        u0 = np.full(n, np.log(start) if log else start)
        f0 = fn(np.full(n, start))
        got = tuple(L.reference_run((lambda u: fn(np.exp(u))) if log else fn, u0, seed=3, run=k, target=1e-10 * f0, max_gen=1000)[0] for k in range(4))
        assert got == reference, (name, got)
