"""No GPU: the Levenberg-Marquardt step through its host mirror ionode_lm_step_host -- the per-candidate routine the kernel runs,
compiled for the host.  Header / binding / library agreement, every refusal, and the step's algebra on seeded cases (tests/lm_cases.py)
against a numpy statement of it."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import lm_cases as L

ROOT = os.path.join(os.path.dirname(__file__), "..")
ENTRIES = ("ionode_lm_step", "ionode_lm_step_host")
ERR_ARG = -1
NAMES = ["d", "active", "sse", "jtr", "jtj", "status", "state", "flag", "iters", "trial"]


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
    body = hdr[hdr.index("typedef struct ionode_lm_desc {"):hdr.index("} ionode_lm_desc;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in re.findall(r"(?:int32_t|double)\s+([^;]+);", body):
        names += [re.sub(r"\[.*?\]", "", n).strip() for n in decl.split(",")]
    assert names == [f[0] for f in capi.IonodeLmDesc._fields_]
    const = dict(re.findall(r"#define IONODE_LM_(\w+) (\S+)", hdr))
    for k, v in const.items():
        assert float.fromhex(v) if "p" in v else int(v) == getattr(capi, "LM_" + k), k
    assert float.fromhex(const["FLOOR_REL"]) == capi.LM_FLOOR_REL and float.fromhex(const["FLOOR_ABS"]) == capi.LM_FLOOR_ABS > 0.0
    assert set(capi.LM_FLAG_TEXT) == set(range(7)) and capi.lm_state_doubles(4) == 4 + 24 + 16


def _call(capi, case, *, entry="ionode_lm_step_host", null=(), **fields):
    """A complete call on the case's first evaluation with host arrays; `null` names the pointers to leave out, `fields` overwrite
    descriptor fields (a (index, value) pair writes one array element)."""
    d = capi.IonodeLmDesc.from_buffer_copy(case["desc"])
    for k, v in fields.items():
        if isinstance(v, tuple):
            getattr(d, k)[v[0]] = v[1]
        else:
            setattr(d, k, v)
    state, flag, iters, trial = L.start(case)
    t = L.tensors(case["evals"][0])
    a = dict(active=None, sse=t["sse"], jtr=t["jtr"], jtj=t["jtj"], status=t["status"], state=state, flag=flag, iters=iters, trial=trial)
    ptrs = [None if (n in null or a[n] is None) else C.c_void_p(a[n].data_ptr()) for n in NAMES[1:]]
    tail = (None,) if entry == "ionode_lm_step" else ()
    rc = getattr(capi.lib(), entry)(None if "d" in null else C.byref(d), *ptrs, *tail)
    return rc, capi.lib().ionode_grad_last_error().decode(), (state, flag, iters, trial)


def test_refusals_come_before_anything_is_touched(ion):
    capi = ion.capi
    case = L.draw(0, 3, 4, 2, log=True)
    entries = ("ionode_lm_step_host",) if torch.cuda.is_available() else ENTRIES   # (with a device a call that slipped through would launch on host addresses)
    for entry in entries:
        rc, msg, _ = _call(capi, case, entry=entry, null=("d",))
        assert rc == ERR_ARG and entry in msg and "null descriptor" in msg
        for name in NAMES[2:]:
            rc, msg, _ = _call(capi, case, entry=entry, null=(name,))
            assert rc == ERR_ARG and entry in msg and "required buffer is NULL" in msg, (name, rc, msg)
        for nf in (0, 13, -1):
            rc, msg, _ = _call(capi, case, entry=entry, n_free=nf)
            assert rc == ERR_ARG and "n_free" in msg
        for bad in (-1, 8):
            rc, msg, _ = _call(capi, case, entry=entry, free_idx=(1, bad))
            assert rc == ERR_ARG and "free index" in msg
        rc, msg, _ = _call(capi, case, entry=entry, lo=(2, 3.0), hi=(2, 2.0))
        assert rc == ERR_ARG and "lo > hi" in msg
        for lo in (0.0, -1.0):
            rc, msg, _ = _call(capi, case, entry=entry, lo=(0, lo))
            assert rc == ERR_ARG and "positive bounds" in msg
        rc, msg, _ = _call(capi, case, entry=entry, n_params=9)
        assert rc == ERR_ARG and "n_params" in msg
        for f in ("n_cand", "n_active", "n_prot", "max_iter"):
            rc, msg, _ = _call(capi, case, entry=entry, **{f: 0})
            assert rc == ERR_ARG and "must be positive" in msg
    rc, msg, _ = _call(capi, case, log_parameters=0, lo=(0, -1.0))   # a negative bound is fine without the logarithm
    assert rc == 0
    rc, msg, (state, flag, iters, trial) = _call(capi, case, n_free=0)
    before = L.start(case)
    assert rc == ERR_ARG and all(L.same_bits(a.numpy(), b.numpy()) for a, b in zip((state, flag, iters, trial), before))


def _views(capi, state, nf):
    return capi.lm_state_views(state, nf)


@pytest.mark.parametrize("C_", L.C_CASES)
@pytest.mark.parametrize("log", [False, True])
@pytest.mark.parametrize("P", L.P_CASES)
@pytest.mark.parametrize("nf", L.NF_CASES)
def test_step_algebra(ion, nf, P, log, C_):
    capi = ion.capi
    case = L.draw(100 * nf + 10 * P + C_ + int(log), C_, nf, P, log=log)
    lam0, free, x0 = 1e-3, case["free"], case["x0"]
    (s1, fl1, it1, tr1), (s2, fl2, it2, tr2) = L.run_sequence(case, lam_init=lam0)
    v = _views(capi, s1, nf)
    # call 1: the evaluation of the starts is accepted as it is; the reduction over protocols, bit for bit
    f, g, H = L.reduce_reference(case, case["evals"][0], x0)
    assert L.same_bits(v["f"], f) and L.same_bits(v["g"], g) and L.same_bits(v["H"], H)
    assert np.array_equal(v["H"], v["H"].transpose(0, 2, 1))
    assert (fl1 == 0).all() and (it1 == 1).all() and (v["lam"] == lam0).all() and (v["nu"] == 2.0).all()
    assert L.same_bits(v["x"], x0) and L.same_bits(v["u"], np.log(x0) if log else x0)
    # the damped system: Cholesky's backward-error bound, in the infinity norm
    D = L.damping_diagonal(capi, H)
    for c in range(C_):
        A = H[c] + v["lam"][c] * np.diag(D[c])
        r = A @ v["delta"][c] + g[c]
        bound = 64 * nf * L.EPS * (np.abs(A).sum(1).max() * np.abs(v["delta"][c]).max() + np.abs(g[c]).max())
        assert np.abs(r).max() <= bound, (c, np.abs(r).max(), bound)
    # the trial point (no box here: with the logarithm the smallest normal number stands for no lower bound), its rows of the trial
    # tensor, the predicted reduction
    raw = v["u"] + v["delta"]
    inside = raw > np.log(np.finfo(np.float64).tiny) + 1e-9 if log else np.ones_like(raw, dtype=bool)
    assert inside.any() and L.same_bits(v["ut"][inside], raw[inside])
    assert np.allclose(v["ut"][~inside], np.log(np.finfo(np.float64).tiny), rtol=4 * L.EPS, atol=0)
    want_xt = np.exp(v["ut"]) if log else v["ut"]
    assert np.allclose(v["xt"][inside], want_xt[inside], rtol=4 * L.EPS, atol=0)
    rows = np.tile(case["base"], (C_ * P, 1))
    rows[:, free] = np.repeat(v["xt"], P, axis=0)
    assert L.same_bits(tr1, rows)
    d = v["ut"] - v["u"]
    pred = -(np.einsum("cj,cj->c", g, d) + 0.5 * np.einsum("cj,cjl,cl->c", d, H, d))
    scale = np.einsum("cj,cj->c", np.abs(g), np.abs(d)) + np.einsum("cj,cjl,cl->c", np.abs(d), np.abs(H), np.abs(d))
    assert (np.abs(v["pred"] - pred) <= 8 * nf * L.EPS * scale).all() and (v["pred"] > 0).all()
    # call 2: a quarter of the value -- the gain ratio decides, Nielsen's rule moves the damping
    w = _views(capi, s2, nf)
    f2, g2, H2 = L.reduce_reference(case, case["evals"][1], v["xt"])
    rho = (f - f2) / v["pred"]
    acc = (f2 < f) & (rho > case["desc"].rho_accept)
    assert acc.any()
    shrink = np.maximum(1.0 / 3.0, 1.0 - (2.0 * rho - 1.0) * (2.0 * rho - 1.0) * (2.0 * rho - 1.0))
    for c in range(C_):
        if acc[c]:
            assert w["f"][c] == f2[c] and L.same_bits(w["g"][c], g2[c]) and L.same_bits(w["H"][c], H2[c]) and L.same_bits(w["x"][c], v["xt"][c])
            assert L.same_bits(w["u"][c], v["ut"][c]) and w["nu"][c] == 2.0 and tuple(it2[c]) == (2, 2)
        else:
            assert w["f"][c] == f[c] and L.same_bits(w["g"][c], g[c]) and L.same_bits(w["H"][c], H[c]) and L.same_bits(w["x"][c], x0[c])
            assert w["nu"][c] == 4.0 and tuple(it2[c]) == (2, 1)
        if fl2[c] == 0:   # (a retry inside the call would move lam further; it must not be needed on SPD input)
            assert w["lam"][c] == (lam0 * shrink[c] if acc[c] else lam0 * 2.0)


@pytest.mark.parametrize("log", [False, True])
def test_projection_onto_the_box_and_pred_of_the_projected_step(ion, log):
    capi = ion.capi
    case = L.draw(7, 67, 4, 3, log=log, bounds=True)
    case["evals"][0]["jtr"] *= 300.0   # steps long enough to leave the box
    (s1, fl1, _, tr1), _ = L.run_sequence(case, lam_init=1e-6)
    v = _views(capi, s1, 4)
    lo, hi = case["lo"], case["hi"]
    raw = v["u"] + v["delta"]
    ulo, uhi = (np.log(lo), np.log(hi)) if log else (lo, hi)
    out = (raw < ulo - 1e-12) | (raw > uhi + 1e-12)
    assert out.any() and (~out).any()
    assert (v["xt"] >= lo).all() and (v["xt"] <= hi).all()
    assert np.allclose(v["ut"], np.clip(raw, ulo, uhi), rtol=0, atol=4 * L.EPS * np.abs(ulo).max() + 4 * L.EPS)
    assert L.same_bits(v["ut"][~out], raw[~out])
    edge = np.where(raw > uhi, hi, lo) * np.ones_like(raw)
    assert np.allclose(v["xt"][out], edge[out], rtol=8 * L.EPS, atol=0)
    d = v["ut"] - v["u"]
    pred = -(np.einsum("cj,cj->c", v["g"], d) + 0.5 * np.einsum("cj,cjl,cl->c", d, v["H"], d))
    scale = np.einsum("cj,cj->c", np.abs(v["g"]), np.abs(d)) + np.einsum("cj,cjl,cl->c", np.abs(d), np.abs(v["H"]), np.abs(d))
    run = fl1 == 0
    assert run.any() and (np.abs(v["pred"] - pred)[run] <= 32 * L.EPS * scale[run]).all()
    rows = np.tile(case["base"], (67 * 3, 1))
    rows[:, case["free"]] = np.repeat(np.where(run[:, None], v["xt"], v["x"]), 3, axis=0)
    assert L.same_bits(tr1, rows)


def _with(case, **fields):
    d = L.mods()[0].IonodeLmDesc.from_buffer_copy(case["desc"])
    for k, val in fields.items():
        setattr(d, k, val)
    return dict(case, desc=d)


def test_every_flag_is_reachable(ion):
    capi = ion.capi
    case = L.draw(11, 5, 4, 3, log=True)
    worse = [case["evals"][0], dict(case["evals"][1], sse=case["evals"][1]["sse"] * 100.0)]
    assert (L.run_sequence(_with(case, gtol=1e300))[0][1] == capi.LM_GTOL).all()
    assert (L.run_sequence(_with(case, xtol=1e300))[0][1] == capi.LM_XTOL).all()
    first, second = L.run_sequence(_with(case, ftol=1.0))
    assert (first[1] == 0).all() and (second[1] == capi.LM_FTOL).all() and (second[2] == 2).all()
    first, second = L.run_sequence(_with(case, lam_max=1.5e-3), evals=worse)
    assert (first[1] == 0).all() and (second[1] == capi.LM_STALLED).all() and (second[2] == (2, 1)).all()
    assert (L.run_sequence(_with(case, max_iter=1))[0][1] == capi.LM_MAXITER).all()
    bad = dict(case, x0=np.where(np.arange(5)[:, None] == 2, np.nan, case["x0"]))
    ev = dict(case["evals"][0], sse=case["evals"][0]["sse"].copy(), status=case["evals"][0]["status"].copy())
    ev["sse"][2 * 3 + 1], ev["status"][2 * 3 + 1] = np.inf, 2
    (state, flag, iters, trial), _ = L.run_sequence(bad, evals=[ev, case["evals"][1]])
    assert flag.tolist() == [0, 0, capi.LM_NONFINITE, 0, 0] and np.isinf(state[2, capi.LM_STATE_F]) and tuple(iters[2]) == (1, 0)
    nang = dict(case["evals"][0], jtr=np.where(np.arange(15)[:, None] == 4, np.nan, case["evals"][0]["jtr"]))   # a finite value with a NaN gradient
    assert L.run_sequence(case, evals=[nang])[0][1].tolist() == [0, capi.LM_NONFINITE, 0, 0, 0]


def test_a_failed_trajectory_makes_the_trial_infinite_and_rejected(ion):
    capi = ion.capi
    case = L.draw(13, 5, 4, 3, log=True)
    ev = dict(case["evals"][1], status=case["evals"][1]["status"].copy())
    ev["status"][3 * 3 + 2] = 3     # candidate 3's last protocol, its sse left finite: the status alone decides
    (s1, _, _, _), (s2, fl2, it2, tr2) = L.run_sequence(case, evals=[case["evals"][0], ev])
    v, w = _views(capi, s1, 4), _views(capi, s2, 4)
    for name in ("f", "u", "x", "g", "H"):
        assert L.same_bits(v[name][3], w[name][3]), name
    assert w["lam"][3] == v["lam"][3] * 2.0 and w["nu"][3] == 4.0 and tuple(it2[3]) == (2, 1) and fl2[3] == 0
    assert (it2[[0, 1, 2, 4]] == 2).all()


def test_an_indefinite_matrix_takes_the_retry_path_and_stalls(ion):
    capi = ion.capi
    case = L.draw(17, 5, 4, 1, log=False)
    ev = dict(case["evals"][0], jtj=case["evals"][0]["jtj"].copy())
    ev["jtj"][1][np.ix_(case["free"], case["free"])] = -np.eye(4)
    ev["jtj"][2][np.ix_(case["free"], case["free"])] = np.diag([1.0, 1.0, -1e-4, 1.0])   # curable: lam D_j reaches 1e-4 within the retries
    (state, flag, iters, trial), = L.run_sequence(case, evals=[ev], lam_init=1e-3)
    v = _views(capi, state, 4)
    assert flag.tolist() == [0, capi.LM_STALLED, 0, 0, 0]
    assert v["lam"][1] == 1e-3 * 2.0 ** sum(range(1, capi.LM_RETRIES + 1)) and v["nu"][1] == 2.0 ** (capi.LM_RETRIES + 1)
    assert v["lam"][2] > 1e-3 and v["nu"][2] > 2.0 and np.isfinite(v["delta"][2]).all()
    A = v["H"][2] + v["lam"][2] * np.diag(L.damping_diagonal(capi, v["H"])[2])
    assert np.linalg.eigvalsh(A).min() > 0 and np.allclose(A @ v["delta"][2], -v["g"][2], rtol=1e-10, atol=1e-12)
    rows = np.tile(case["base"], (5, 1))
    rows[:, case["free"]] = np.where((flag == 0)[:, None], v["xt"], v["x"])
    assert L.same_bits(trial, rows)


def test_a_stopped_candidate_is_frozen(ion):
    capi = ion.capi
    case = _with(L.draw(19, 5, 8, 3, log=True), max_iter=1)
    first, second = L.run_sequence(case)
    assert (first[1] == capi.LM_MAXITER).all()
    for a, b in zip(first[:3], second[:3]):
        assert L.same_bits(a, b)
    v = _views(capi, second[0], 8)
    rows = np.tile(case["base"], (15, 1))
    rows[:, case["free"]] = np.repeat(v["x"], 3, axis=0)
    assert L.same_bits(second[3], rows)


@pytest.mark.parametrize("nf,P", [(4, 3), (12, 1), (1, 3)])
def test_a_candidate_does_not_depend_on_its_company(ion, nf, P):
    """Alone, inside C = 67, and through an active list (another slot order, a subset): the same bits."""
    case = L.draw(23 + nf, 67, nf, P, log=True)
    whole = L.run_sequence(case)
    active = [66, 5, 0, 31, 64, 2, 17]
    listed = L.run_sequence(case, active=active)
    for k in range(2):
        for c in range(67):   # candidates outside the list keep their initial state
            if c not in active:
                assert L.same_bits(listed[k][0][c], L.start(case)[0].numpy()[c]) and listed[k][1][c] == 0 and (listed[k][2][c] == 0).all()
        for s, c in enumerate(active):
            assert L.same_bits(listed[k][0][c], whole[k][0][c]) and listed[k][1][c] == whole[k][1][c] and L.same_bits(listed[k][2][c], whole[k][2][c])
            assert L.same_bits(listed[k][3][s * P:(s + 1) * P], whole[k][3][c * P:(c + 1) * P])
    fit = L.mods()[1]
    for c in (0, 5, 66):
        rows = slice(c * P, (c + 1) * P)
        d = case["desc"]
        alone = dict(case, C=1, x0=case["x0"][c:c + 1], evals=[{k: v[rows] for k, v in ev.items()} for ev in case["evals"]],
                     desc=fit.lm_desc(1, P, case["npar"], case["free"], case["base"], log_parameters=True, lo=None, hi=None, max_iter=d.max_iter,
                                      gtol=d.gtol, xtol=d.xtol, ftol=d.ftol))
        single = L.run_sequence(alone)
        for k in range(2):
            assert L.same_bits(single[k][0][0], whole[k][0][c]) and single[k][1][0] == whole[k][1][c] and L.same_bits(single[k][3], whole[k][3][rows])


def test_a_variable_on_its_bound_with_the_gradient_pointing_out_is_held(ion):
    """Starts on the box's upper corner: the variables whose gradient is negative there (the step would push them out) get
    delta = 0 exactly, the others solve the reduced damped system; the gradient test does not count the held ones."""
    capi = ion.capi
    case = L.draw(29, 67, 4, 1, log=False, bounds=True)
    case["x0"][:] = case["hi"]
    (state, flag, iters, trial), _ = L.run_sequence(case)
    v = _views(capi, state, 4)
    held = v["g"] < 0
    corner = held.all(1)          # every variable held: the corner is the constrained minimum of the model, the gradient test says so
    assert corner.any() and (~corner).any() and (flag[corner] == capi.LM_GTOL).all() and (flag[~corner] == 0).all()
    held = held & ~corner[:, None]
    assert (v["delta"][held] == 0).all() and (v["ut"][held] == case["hi"][None, :].repeat(67, 0)[held]).all()
    D = L.damping_diagonal(capi, v["H"])
    for c in range(67):
        k = ~held[c]
        if not corner[c]:
            A = (v["H"][c] + v["lam"][c] * np.diag(D[c]))[np.ix_(k, k)]
            r = A @ v["delta"][c][k] + v["g"][c][k]
            assert np.abs(r).max() <= 64 * 4 * L.EPS * (np.abs(A).sum(1).max() * np.abs(v["delta"][c][k]).max() + np.abs(v["g"][c][k]).max())
