"""No GPU: the NN models' tangent sweep below the kernel -- the entry point ionode_tangent_sweep_nn (header, exports, binding, refusals
with host stand-in pointers), the rule for an NN model in sensitivity / objective / fit / mala (refused without weights as before,
served with one weight set), the three drivers with model = NN-d, weights and a stand-in solver on CPU tensors, the chunk order, and
the checker (tests/tangent_nn_check.py): its recorded forward-mode Jacobians against the walk's step algebra written out by hand."""
import ctypes as C
import importlib
import os
import re

import numpy as np
import pytest
import torch

import kat_cases as K
import lm_cases as L
import mala_cases as M
import sse_nn_cases as N
import tangent_nn_check as T

ROOT = os.path.join(os.path.dirname(__file__), "..")
ENTRY, HELPER = "ionode_tangent_sweep_nn", "ionode_tangent_nn_state_doubles"
ERR_ARG, ERR_UNSUPPORTED = -1, -2
GRAD_REL_TOL = 1e-4   # the project's tolerance for every NN derivative against its checker (tests/test_gpu_sse_grad_nn.py)


def _mod(name):
    return importlib.import_module("neural-ode-ion-channels_amd." + name)


def test_header_declares_library_exports_and_capi_binds_the_entry_point(ion):
    capi = ion.capi
    hdr = open(os.path.join(ROOT, "include", "ionode.h")).read()
    assert "#define IONODE_ABI_VERSION 10" in hdr and capi.ABI_VERSION == 10 and capi.lib().ionode_abi_version() == 10
    args = re.search(r"\bint\s+%s\s*\(([^;]*)\);" % ENTRY, hdr).group(1).split(",")
    names = [a.split()[-1].lstrip("*") for a in args]
    assert names == ["d", "it_begin", "it_end", "n_iter"] + list(capi.TANGENT_NN_BUFFERS) + ["stream"]
    restype, argtypes = capi.PROTOTYPES[ENTRY]
    assert restype is C.c_int and len(argtypes) == len(names) and argtypes[1:4] == [C.c_int32] * 3 and set(argtypes[4:]) == {C.c_void_p}
    assert re.search(r"\bsize_t\s+%s\s*\(\s*void\s*\)\s*;" % HELPER, hdr) and capi.PROTOTYPES[HELPER] == (C.c_size_t, [])
    assert ENTRY in capi.EXPORTS and HELPER in capi.EXPORTS and ENTRY not in capi.SWEEP_BUFFERS
    lib = C.CDLL(capi.LIB_PATH)
    assert getattr(lib, ENTRY) is not None and getattr(lib, HELPER) is not None
    # per (trajectory, parameter): S [2], Kd_7 [2], J^T r, a row of J^T J
    assert capi.lib().ionode_tangent_nn_state_doubles() == 8 * (2 + 2 + 1 + 8)
    # the closed-form entry point keeps refusing the NN models; its comment no longer gives the reason that stopped holding
    assert "Jacobian-vector product through the MLP tiles" not in hdr and "ionode_tangent_sweep_nn below" in hdr


class _HostCall:
    """A complete NN-d call with HOST stand-in pointers (nothing is dereferenced by the checks); keywords name defects."""
    BUFFERS = ("grad_image", "params", "prot_v", "t_eval", "n_accepted", "packets", "state")

    def __init__(self, capi):
        self.capi = capi
        self.buf = np.zeros(64)

    def __call__(self, *, model=3, null_desc=False, missing=(), outputs=("di_dp", "jtr", "jtj"), sse_ref=True, ckpt=True, traj_per_image=0,
                 rng=(0, 3, 3), mlp=(5, 10)):
        capi, p = self.capi, self.buf.ctypes.data
        m6 = model == capi.MODEL_MARKOV6
        d = capi.make_desc(model=model, n_state=6 if m6 else 2, n_out=5, n_traj=3, n_prot=1, prot_n=10, n_params=12 if m6 else 8,
                           prot_dt=1.0, rtol=1e-7, atol=1e-9, v_oob=-80.0, obs_g=1.0, obs_e=-86.0, traj_per_image=traj_per_image,
                           mlp_layers=mlp[0] if model >= 2 else 0, mlp_width=mlp[1] if model >= 2 else 0)
        if ckpt:
            d.ckpt, d.ckpt_cap = p, 4
        if sse_ref:
            d.sse_ref = p
        a = {n: (None if n in missing else p) for n in self.BUFFERS}
        o = {n: (p if n in outputs else None) for n in ("di_dp", "jtr", "jtj")}
        rc = capi.lib().ionode_tangent_sweep_nn(None if null_desc else C.byref(d), rng[0], rng[1], rng[2], a["grad_image"], a["params"],
                                                a["prot_v"], None, None, a["t_eval"], a["n_accepted"], a["packets"], a["state"], o["di_dp"],
                                                o["jtr"], o["jtj"], None)
        return rc, capi.lib().ionode_grad_last_error().decode()


@pytest.fixture
def host_call(ion):
    if torch.cuda.is_available():
        pytest.skip("a HIP device is visible: a call that slipped through the checks would launch with host addresses")
    return _HostCall(ion.capi)


def test_refusals_are_decided_before_any_launch(host_call):
    rc, msg = host_call(null_desc=True)
    assert rc == ERR_ARG and "null descriptor" in msg
    for name in _HostCall.BUFFERS:
        rc, msg = host_call(missing=(name,))
        assert rc == ERR_ARG and ENTRY in msg and "required buffer is NULL" in msg, (name, rc, msg)
    rc, msg = host_call(ckpt=False)
    assert rc == ERR_ARG and ENTRY in msg and "ckpt" in msg
    rc, msg = host_call(outputs=())
    assert rc == ERR_ARG and ENTRY in msg and "all NULL" in msg
    for outs in (("jtr",), ("jtj",), ("di_dp", "jtj")):
        rc, msg = host_call(outputs=outs, sse_ref=False)
        assert rc == ERR_ARG and ENTRY in msg and "sse_ref" in msg, (outs, rc, msg)
    for rng in ((-1, 2, 3), (2, 2, 3), (2, 1, 3), (0, 4, 3)):
        rc, msg = host_call(rng=rng)
        assert rc == ERR_ARG and "bad iteration range" in msg, (rng, rc, msg)
    for model in (0, 1):
        rc, msg = host_call(model=model)
        assert rc == ERR_UNSUPPORTED and ENTRY in msg and "ionode_tangent_sweep)" in msg, (model, rc, msg)
    for model in (2, 3):
        rc, msg = host_call(model=model, traj_per_image=16)
        assert rc == ERR_UNSUPPORTED and ENTRY in msg and "traj_per_image" in msg
    for mlp in ((5, 300), (16, 10), (5, 513)):   # a width between two compiled classes, too deep, too wide
        rc, msg = host_call(mlp=mlp)
        assert rc == ERR_UNSUPPORTED and ENTRY in msg and "compiled variants" in msg, (mlp, rc, msg)
    rc, msg = host_call(mlp=(0, 10))
    assert rc == ERR_ARG and "bad MLP shape" in msg


def test_the_trace_alone_passes_the_checks_without_sse_ref(ion):
    """(no launch is made: the range check behind the sse_ref rule refuses the call)"""
    if torch.cuda.is_available():
        pytest.skip("a HIP device is visible")
    rc, msg = _HostCall(ion.capi)(outputs=("di_dp",), sse_ref=False, rng=(3, 3, 3))
    assert rc == ERR_ARG and "bad iteration range" in msg


def test_chunks_are_visited_forward_in_time():
    s = _mod("sensitivity")
    chunk, bounds = s.nn_chunks(12, 2, 1024, 1 << 30, 5)
    assert chunk == 5 and bounds == [(7, 12), (2, 7), (0, 2)]
    assert s.nn_chunks(12, 2, 1024, 1 << 30, 1)[1] == [(k, k + 1) for k in range(11, -1, -1)]
    assert s.nn_chunks(12, 2, 1024, 1 << 30)[1] == [(0, 12)] and s.nn_chunks(600, 2, 1024, 1 << 30)[1] == [(344, 600), (88, 344), (0, 88)]
    chunk, bounds = s.nn_chunks(600, 2, 1024, 2 * 2 * 1024 * 8 * 7)   # a budget of seven iterations of packets per buffer half
    assert chunk == 7 and bounds[0] == (593, 600) and bounds[-1] == (0, 5) and all(a[0] == b[1] for a, b in zip(bounds, bounds[1:]))


# ---- the rule for NN models, everywhere it is applied ----

BASE = np.array([1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0])
W = np.arange(2 * 3 + 3 + 1 * (3 * 3 + 3) + 3 + 1, dtype=np.float32)   # a (1, 3) net's flat state dict
NN = dict(weights=W, mlp_layers=1, mlp_width=3)


def _gn_standin(seen):
    def solver(model, params, prot_v, y0, t_eval, sse_ref, **kw):
        seen.append(dict(kw, model=model, B=params.shape[0]))
        pot = kw["prot_of_traj"].double()
        sse = params.sum(1) * (pot + 1.0)
        jtr = params * (pot[:, None] + 2.0)
        jtj = params[:, :, None] * params[:, None, :] + torch.eye(8, dtype=torch.float64)[None] * (pot[:, None, None] + 1.0)
        return sse, jtr, jtj, torch.zeros(params.shape[0], dtype=torch.int32)
    return solver


def _callers(capi, model, extra):
    """Every function the rule is applied in, as (name, call) with the NN keywords `extra`."""
    obj, fit, mala, s = _mod("objective"), _mod("fit"), _mod("mala"), _mod("sensitivity")
    p8, y2 = torch.ones((3, 8), dtype=torch.float64), torch.zeros((3, 2), dtype=torch.float64)
    pv, te, ref = torch.zeros((1, 10), dtype=torch.float64), torch.arange(5.0, dtype=torch.float64), torch.zeros((1, 5), dtype=torch.float64)
    free = extra.pop("free", (4, 5, 6))
    pop = (np.ones((2, len(free))), np.zeros((1, 20)), np.zeros((1, 7)), np.arange(7.0))
    box = (np.full(len(free), 0.1), np.full(len(free), 10.0))
    common = dict(base_params=BASE, free=free, solver=_gn_standin([]), device="cpu", max_step=0.0, model=model, **extra)
    out = [("population_gauss_newton", lambda: obj.population_gauss_newton(*pop, **common)),
           ("population_fit", lambda: obj.population_fit(*pop, **common)),
           ("population_mala", lambda: obj.population_mala(*pop, bounds=box, sigma=1.0, **common)),
           ("fit.levenberg_marquardt", lambda: fit.levenberg_marquardt(model, *pop, **{k: v for k, v in common.items() if k != "model"})),
           ("mala.sample", lambda: mala.sample(model, *pop, bounds=box, sigma=1.0, **{k: v for k, v in common.items() if k != "model"}))]
    if free == (4, 5, 6):   # (the sensitivity entry points take no `free`)
        out += [("sensitivity.current_s1", lambda: s.current_s1(model, p8, pv, y2, te, **extra)),
                ("sensitivity.gauss_newton", lambda: s.gauss_newton(model, p8, pv, y2, te, ref, **extra))]
    return out


def test_an_nn_model_without_weights_is_refused_as_before(ion):
    capi = ion.capi
    for model in (capi.MODEL_NNF, capi.MODEL_NND):
        for name, call in _callers(capi, model, {}):
            with pytest.raises(capi.IonodeError) as e:
                call()
            assert all(w in str(e.value) for w in ("closed-form", "HH 2-state and 6-state", "population_mcmc", "weights")), (name, str(e.value))


def test_a_weight_population_and_nn_f_columns_below_4_are_refused_by_name(ion):
    capi = ion.capi
    for name, call in _callers(capi, capi.MODEL_NND, dict(weights=np.stack([W, W]), mlp_layers=1, mlp_width=3)):
        with pytest.raises(capi.IonodeError, match=r"weights \[C, n\]"):
            call()
    for free in ((0, 4), (3,), (4, 5, 2)):
        for name, call in _callers(capi, capi.MODEL_NNF, dict(NN, free=free)):
            with pytest.raises(capi.IonodeError, match="NN-f has no p1..p4"):
                call()
    for name, call in _callers(capi, capi.MODEL_HH2, dict(NN)):
        with pytest.raises(capi.IonodeError, match="no MLP"):
            call()
    # with weights the sensitivity entry points get as far as the device check
    s = _mod("sensitivity")
    p8, y2 = torch.ones((3, 8), dtype=torch.float64), torch.zeros((3, 2), dtype=torch.float64)
    with pytest.raises(capi.IonodeError, match="no HIP tensors"):
        s.current_s1(capi.MODEL_NND, p8, torch.zeros((1, 10), dtype=torch.float64), y2, torch.arange(5.0, dtype=torch.float64), **NN)
    for mod, words in ((s, ("NN models", "y0", "Levenberg-Marquardt")), (_mod("fit"), ("NN models", "CMA-ES", "noise model", "y0"))):
        assert all(w in mod.__doc__ for w in words)
    assert all(w in _mod("objective").population_fit.__doc__ for w in ("NN models", "CMA-ES", "noise model", "y0"))


# ---- the drivers with model = NN-d, weights and a stand-in solver: to their stop flags through the host steps ----

def test_population_gauss_newton_hands_the_weights_to_the_evaluation(ion):
    capi, obj = ion.capi, _mod("objective")
    seen = []
    Cn, P, free = 3, 2, (1, 4, 6)
    cand = np.random.default_rng(0).uniform(0.5, 2.0, (Cn, len(free)))
    sse, g, H = obj.population_gauss_newton(cand, np.zeros((P, 20)), np.zeros((P, 7)), np.arange(7.0), base_params=BASE, free=free,
                                            max_step="auto", state_dtype=torch.float64, model=capi.MODEL_NND, solver=_gn_standin(seen),
                                            device="cpu", weights_key="k", **NN)
    kw = seen[0]
    assert kw["model"] == capi.MODEL_NND and kw["B"] == Cn * P and kw["weights"] is W and (kw["mlp_layers"], kw["mlp_width"]) == (1, 3)
    assert kw["weights_key"] == "k" and kw["max_step"] == 0.0   # "auto": no cap for the NN models, as population_cmaes resolves it
    for c in range(Cn):
        p = BASE.copy()
        p[list(free)] = cand[c]
        want_g = 2.0 * sum(p * (k + 2.0) for k in range(P))[list(free)]
        assert np.allclose(g[c].numpy(), want_g, rtol=1e-13, atol=0) and torch.equal(H[c], H[c].T)
    # a closed-form model's evaluation sees no MLP keywords
    seen.clear()
    obj.population_gauss_newton(cand, np.zeros((P, 20)), np.zeros((P, 7)), np.arange(7.0), base_params=BASE, free=free, max_step=1.0,
                                solver=_gn_standin(seen), device="cpu")
    assert "weights" not in seen[0] and "mlp_layers" not in seen[0]


def test_population_fit_runs_an_nn_model_to_its_stop_flags(ion):
    capi, obj = ion.capi, _mod("objective")
    data, x0, seen = L.two_exp_data(sigma=0.1), L.two_exp_starts(4), []
    inner = L.two_exp_solver()

    def solver(model, params, *a, **kw):
        seen.append((model, kw.get("weights"), kw.get("mlp_layers"), kw.get("mlp_width"), kw.get("weights_key"), kw["max_step"]))
        return inner(model, params, *a, **kw)

    kw = dict(base_params=L.BASE8, bounds=(L.TRUE / 3.0, L.TRUE * 3.0), solver=solver, state_dtype=torch.float64, device="cpu", max_iter=100, gtol=1e-10,
              xtol=1e-10, ftol=1e-13)
    x, sse, flag, iters = obj.population_fit(x0, L.SCALES, data, L.T_EVAL, model=capi.MODEL_NND, max_step="auto", weights_key="k", **NN, **kw)
    assert len(seen) >= 2 and all(s[1] is W and s[:1] + s[2:] == (capi.MODEL_NND, 1, 3, "k", 0.0) for s in seen)   # "auto": no cap for the NN models
    assert (flag.numpy() != capi.LM_RUNNING).all() and (flag.numpy() != capi.LM_MAXITER).all() and (flag.numpy() != capi.LM_NONFINITE).all()
    # the NN keywords change nothing in the iteration: the closed-form call on the same stand-in ends at the same bits
    ref = obj.population_fit(x0, L.SCALES, data, L.T_EVAL, max_step=0.0, **kw)
    for a, b in zip((x, sse, flag, iters), ref):
        assert L.same_bits(a.numpy(), b.numpy())


def test_population_mala_runs_an_nn_model_to_its_stop_flags(ion):
    capi, obj = ion.capi, _mod("objective")
    pb = M.gauss_problem(True)
    free, seen = (4, 6, 7), []
    inner = M.gn_solver(pb["resid"], free, 2)

    def solver(model, params, *a, **kw):
        seen.append((model, kw.get("weights"), kw.get("mlp_layers"), kw.get("mlp_width")))
        return inner(model, params, *a, **kw)

    args = (np.zeros((2, 10)), np.zeros((2, 5)), np.arange(5.0))
    kw = dict(base_params=np.full(8, 9.0), free=free, bounds=pb["bounds"], sigma=1.0, max_step=0.0, state_dtype=torch.float64, device="cpu",
              max_iter=20, seed=3)
    for model in (capi.MODEL_NND, capi.MODEL_NNF):   # (NN-f: every free index is at least 4)
        seen.clear()
        smp, rate, flag, iters = obj.population_mala(pb["x0"][:3], *args, solver=solver, model=model, **NN, **kw)
        assert len(seen) == 21 and all(s[0] == model and s[1] is W and s[2:] == (1, 3) for s in seen)
        assert (flag.numpy() == capi.MALA_MAXITER).all() and smp.shape == (3, 21, 4) and np.isfinite(smp.numpy()).all()
    ref = obj.population_mala(pb["x0"][:3], *args, solver=inner, **kw)
    assert M.same_bits(smp.numpy(), ref[0].numpy())


# ---- the checker ----

@pytest.mark.parametrize("f32", [False, True])
@pytest.mark.parametrize("L_,N_,model", T.CASES)
def test_recorded_jacobians_against_the_step_algebra(oracle, L_, N_, model, f32):
    """Every recorded row (forward-mode AD through the replay) against the walk's recurrence written out by hand, which takes the net's
    derivative as the recompute kernel does: from a reverse pass through the fp32 net.  The two differ by the fp32 rounding of that one
    number per stage -- fp32 epsilon, 6e-8, times the handful of operations per layer: 1e-6 = GRAD_REL_TOL / 100 bounds it (measured:
    4e-10 at most in fp64 state); NN-f's recorded columns p1..p4 are zero."""
    c = N.problem(L_, N_, model, f32)
    cols = N.param_cols(model)
    worst = 0.0
    for b, J in T.recorded_jacobians(L_, N_, model, f32).items():
        steps, anchors = T.steps_and_anchors(oracle, c, b)
        assert J.shape == (c.te.size, 8) and not J[0].any() and (np.linalg.norm(J[:, cols], axis=0) > 0).all()
        if model == K.MODEL_NNF:
            assert not J[:, :4].any()
        worst = max(worst, float(T.column_errors(T.manual_jacobian(oracle, c, b, steps, anchors), J, cols).max()))
    print(f"L={L_} N={N_} model {model} {'f32' if f32 else 'f64'}: worst column, step algebra vs recorded AD {worst:.2e}")
    assert worst <= 0.01 * GRAD_REL_TOL


@pytest.mark.slow
def test_the_record_is_what_the_checker_computes(oracle):
    """One recorded trajectory recomputed (NN-f at (1, 200), fp32 state: four passes of dual numbers): the same bits up to the
    rounding of another BLAS, and its reverse-mode counterpart J^T w."""
    torch.set_num_threads(1)
    L_, N_, model, f32 = 1, 200, K.MODEL_NNF, True
    c = N.problem(L_, N_, model, f32)
    b = 18
    i0, J = T.jacobian(oracle, c, b)
    rec = T.recorded_jacobians(L_, N_, model, f32)[b]
    assert T.column_errors(J, rec, N.param_cols(model)).max() <= 0.01 * GRAD_REL_TOL   # (another BLAS may sum the fp32 net's 200-term products in another order)
    steps, anchors = T.steps_and_anchors(oracle, c, b)
    w = np.random.default_rng(5).normal(0.0, 1.0, i0.size)
    p = torch.tensor(c.params[b], dtype=torch.float64, requires_grad=True)
    (T.replay_current(oracle, c, b, p, steps, anchors) * torch.from_numpy(w)).sum().backward()
    rev = p.grad.numpy()
    assert np.linalg.norm(J.T @ w - rev) <= 1e-5 * np.linalg.norm(rev)   # (fp32 net: forward and reverse mode round differently)
