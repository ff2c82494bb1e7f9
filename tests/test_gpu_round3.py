"""-m gpu: round-3 additions -- the review's hygiene items and the advisor's edge cases.

* BASELINE configs[3] at one GPU's full share over ALL THREE protocol families (8192 candidates x (7 Pr3 + 16 Pr4 + 9 Pr5) sweeps),
  through planted / repeated / NaN candidates (size-independent properties) and three candidates against the oracle.
* gradient path: a failing trajectory inside a batch neither grows the checkpoint buffer nor leaks NaN into the gradients of an
  UNMASKED loss; the checkpoint budget raises instead of exhausting memory; an uncapped rate-parameter gradient warns and
  max_step="auto" (grad.stable_step_cap) keeps it finite on a long hold in fp32 state.
* a large population of N <= 16 nets (16 trajectories per candidate) dispatches to a kernel that accepts it.
* the asm evaluation stream of the N = 200 tile: every depth L = 1 .. 6 (odd / even: the barrier behind Linear(N, 1)), ragged tiles.
"""
import importlib
import warnings

import numpy as np
import pytest
import torch

import kat_cases as K

pytestmark = pytest.mark.gpu


def test_config4_share_over_all_three_protocol_families(ion, gpu, oracle):
    """8192 candidates x 32 sweeps (Pr3 activation train-s1.py:69-80, synthetic Pr4, Pr5 deactivation :83-95) = 262 144 solves,
    fused sum of squares.  The data are the GPU's own traces of the true parameters: the planted candidates score exactly 0 in
    every family, repeated candidates repeat, a NaN candidate is inf, three random candidates equal the oracle sweep by sweep."""
    P = ion.protocols
    obj = importlib.import_module("neural-ode-ion-channels_amd.objective")
    fams = {"pr3": np.stack([P.activation_pr3(v) for v in P.PR3_STEPS]),
            "pr4": np.stack([P.pr4_synthetic(k) for k in range(16)]),
            "pr5": np.stack([P.deactivation_pr5(v) for v in P.PR5_STEPS])}
    rng = np.random.default_rng(11)
    C = 8192
    cand = np.array([1.13e-4, 7.45e-2, 3.60e-5, 4.49e-2]) * np.exp(rng.normal(0.0, 0.1, (C, 4)))   # CMA-ES first generation, train-d0.py:325-328
    planted = [0, 4097, C - 1]
    cand[planted] = K.P_NN_D[:4]
    cand[100:200] = cand[300:400]
    cand[77] = np.nan
    total = np.zeros(C)
    for name, pv in fams.items():
        S, Np = pv.shape
        te = np.arange(Np) * 0.1
        data = ion.solve(K.MODEL_HH2, np.tile(K.P_NN_D, (S, 1)), pv, torch.tensor([[0.0, 1.0]]), te, prot_t0=0.0, prot_dt=0.1,
                         current=True).i.cpu().numpy()
        got = obj.population_sum_of_squares(cand, pv, data, te, base_params=K.P_NN_D, prot_t0=0.0, prot_dt=0.1,
                                            max_total_steps=200000).cpu().numpy()
        assert got.shape == (C,) and np.isinf(got[77]) and (got[planted] == 0.0).all(), name
        fin = np.isfinite(got)
        assert fin.sum() >= C - 1 and (got[fin] >= 0).all() and np.array_equal(got[100:200], got[300:400]), name
        for c in (5, 2500, 8000):
            p = K.P_NN_D.copy()
            p[:4] = cand[c]
            o = oracle.solve(K.MODEL_HH2, np.tile(p, (S, 1)), pv, [0.0, 1.0], te, prot_t0=0.0, prot_dt=0.1, state_f32=True,
                             prot_of_traj=np.arange(S, dtype=np.int32), max_total_steps=200000, nthreads=4)
            assert (o["status"] == 0).all()
            sim = np.stack([oracle.current(o["y"][k], oracle.protocol_v(pv[k], te, prot_t0=0.0, prot_dt=0.1)[0], state_f32=True)
                            for k in range(S)])
            want = ((sim - data) ** 2).sum()
            assert abs(got[c] - want) <= 1e-12 * max(want, 1e-300), (name, c)
        total += got
    assert (total[planted] == 0.0).all() and np.isinf(total[77]) and total[np.isfinite(total)].min() == 0.0


def _hh_batch(gpu, B, f32=False, n_prot=2001):
    pv = np.full((1, n_prot), -80.0)
    pv[0, 200:1200] = 20.0
    te = np.arange(0, n_prot - 1, 10.0)
    params = np.tile(K.P_HH, (B, 1)) * np.random.default_rng(3).uniform(0.9, 1.1, (B, 8))
    sdt = torch.float32 if f32 else torch.float64
    return (torch.from_numpy(params).to(gpu), torch.from_numpy(pv).to(gpu),
            torch.tensor([[0.0, 1.0]], dtype=sdt, device=gpu).repeat(B, 1).contiguous(), torch.from_numpy(te).to(gpu))


def test_failed_trajectory_inside_a_gradient_batch(ion, gpu):
    """one trajectory fails (too stiff for the explicit solver: step budget / dt underflow).  Its row must not size the checkpoint buffer, its y is
    NaN-filled, and with an UNMASKED loss the other rows' gradients stay finite while its own are exactly zero."""
    B = 20
    params, pv, y0, te = _hh_batch(gpu, B)
    stiff = params.clone()
    stiff[7, 4:8] *= 3e3                       # the r gate of trajectory 7 becomes far too stiff for an explicit solver
    p = stiff.requires_grad_(True)
    y0 = y0.requires_grad_(True)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        y, status = ion.grad.solve(K.MODEL_HH2, None, p, pv, y0, te, prot_t0=0.0, prot_dt=1.0, max_total_steps=3000, ckpt_cap=256)
    st = status.cpu().numpy()
    assert st[7] != 0 and (np.delete(st, 7) == 0).all()   # (step budget or dt underflow, whichever the stiff gate hits first)
    assert torch.isnan(y[7, -1]).all()
    torch.nan_to_num(y).sum().backward()       # unmasked: the upstream gradient of row 7 is 1 everywhere
    gp, gy0 = p.grad.cpu().numpy(), y0.grad.cpu().numpy()
    assert np.isfinite(gp).all() and np.isfinite(gy0).all()
    assert (gp[7] == 0).all() and (gy0[7] == 0).all() and np.abs(np.delete(gp, 7, 0)).sum() > 0
    # a clean batch of the other 19 gives the same gradients: the failing row did not disturb its tile-mates
    keep = [i for i in range(B) if i != 7]
    p2 = stiff.detach()[keep].clone().requires_grad_(True)
    y2 = y0.detach()[keep].clone().requires_grad_(True)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        yb, sb = ion.grad.solve(K.MODEL_HH2, None, p2, pv, y2, te, prot_t0=0.0, prot_dt=1.0, max_total_steps=3000, ckpt_cap=256)
    yb.sum().backward()
    assert torch.equal(yb, y[keep]) and np.array_equal(p2.grad.cpu().numpy(), gp[keep]) and np.array_equal(y2.grad.cpu().numpy(), gy0[keep])


def test_checkpoint_budget_raises_instead_of_allocating(ion, gpu):
    params, pv, y0, te = _hh_batch(gpu, 4)
    with pytest.raises(ion.capi.IonodeError, match="ckpt_budget_bytes"):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            ion.grad.solve(K.MODEL_HH2, None, params.requires_grad_(True), pv, y0, te, prot_t0=0.0, prot_dt=1.0, ckpt_cap=2,
                           ckpt_budget_bytes=1 << 10)


def test_uncapped_rate_gradient_warns_and_auto_cap_keeps_it_finite(ion, gpu):
    """in fp32 state the exact derivative of accepted-but-unstable steps on a long hold explodes (|dL/dp| up to
    1e36).  The default call warns; max_step='auto' (3 / lambda_max of the rate constants) returns a bounded gradient that
    agrees with an fp64-state solve of the same capped problem."""
    B = 4
    params, _, y0, _ = _hh_batch(gpu, B, f32=True)
    pv = np.full((1, 100001), -80.0)
    pv[0, 5000:15000] = 40.0                   # 10 s protocol: 1 s at +40 mV, then a 8.5 s hold at -80 mV
    pv = torch.from_numpy(pv).to(gpu)
    te = torch.arange(0, 10000.0, 50.0, dtype=torch.float64, device=gpu)
    p = params.clone().requires_grad_(True)
    with pytest.warns(RuntimeWarning, match="UNCAPPED"):
        ion.grad.solve(K.MODEL_HH2, None, p, pv, y0, te, prot_t0=0.0, prot_dt=0.1)
    cap = ion.grad.stable_step_cap(K.MODEL_HH2, params, pv)
    assert 1.0 < cap < 40.0
    grads = {}
    for f32 in (True, False):
        p = params.clone().requires_grad_(True)
        with warnings.catch_warnings():
            warnings.simplefilter("error", RuntimeWarning)   # 'auto' must not warn
            y, status = ion.grad.solve(K.MODEL_HH2, None, p, pv, y0.to(torch.float32 if f32 else torch.float64), te, prot_t0=0.0,
                                       prot_dt=0.1, max_step="auto")
        assert bool((status == 0).all())
        (y.double()[:, :, 0] * y.double()[:, :, 1]).sum().backward()
        grads[f32] = p.grad.cpu().numpy()
        assert np.isfinite(grads[f32]).all() and np.abs(grads[f32]).max() < 1e6
    rel = np.linalg.norm(grads[True] - grads[False]) / np.linalg.norm(grads[False])
    assert rel < 1e-2, rel


def test_large_population_of_tiny_nets_dispatches(ion, gpu, oracle):
    """C x 16 >= 73 728 trajectories with one N = 10 net per candidate (weights [C, n], traj_per_image = 16) used to
    pick the 64-per-wavefront kernel and fail with IONODE_ERR_ARG; it now runs on the 16-per-wavefront kernel."""
    P = ion.protocols
    obj = importlib.import_module("neural-ode-ion-channels_amd.objective")
    pv = np.stack([P.deactivation_pr5(v)[:2001] for v in P.PR5_STEPS])
    S, Np = pv.shape
    te = np.arange(0, Np, 4) * 0.1
    C, L, N = 4700, 1, 10
    rng = np.random.default_rng(2)
    n = 2 * N + N + L * (N * N + N) + N + 1
    w = rng.normal(0, 0.1, (C, n)).astype(np.float32)
    w[1] = w[0]
    data = np.zeros((S, te.size))
    got = obj.population_sum_of_squares(np.zeros((C, 0)), pv, data, te, base_params=K.P_HH, free=(), prot_t0=0.0, prot_dt=0.1,
                                        model=K.MODEL_NNF, weights=w, mlp_layers=L, mlp_width=N, state_dtype=torch.float64).cpu().numpy()
    assert got.shape == (C,) and np.isfinite(got).all() and got[0] == got[1]
    for c in (0, C - 1):
        o = oracle.solve(K.MODEL_NNF, np.tile(K.P_HH, (S, 1)), pv, [0.0, 1.0], te, prot_t0=0.0, prot_dt=0.1, weights=w[c],
                         mlp_layers=L, mlp_width=N, prot_of_traj=np.arange(S, dtype=np.int32))
        sim = np.stack([oracle.current(o["y"][k], oracle.protocol_v(pv[k], te, prot_t0=0.0, prot_dt=0.1)[0]) for k in range(S)])
        want = (sim ** 2).sum()
        assert abs(got[c] - want) <= 1e-10 * want


@pytest.mark.parametrize("L", [1, 2, 3, 4, 6])
@pytest.mark.parametrize("f32", [False, True])
@pytest.mark.parametrize("tile", [4, 8])
def test_asm_stream_every_depth(ion, gpu, oracle, L, f32, tile):
    """The N = 200 tile's evaluation is one asm statement looping over the hidden layers (tools/gen_mlp_asm.py): odd and even depths
    (weight-ring wrap to layer 0, the barrier behind Linear(N, 1) for even L), ragged tiles, NN-f and NN-d -- for the 16-trajectory
    tile (tile_waves = 4) and the 32-trajectory tile with two column sets per weight fragment (tile_waves = 8: B = 53 is one full
    tile and one whose second column set holds 5 trajectories)."""
    N, B = 200, (21 if tile == 4 else 53)
    rng = np.random.default_rng(100 + L)
    n = 2 * N + N + L * (N * N + N) + N + 1
    w = (rng.normal(0, 0.08, n)).astype(np.float32)
    pv = np.stack([K.activation(v)[1][:1501] for v in (-20, 40)])
    te = np.arange(0, 1500, 3.0)
    params = np.tile(K.P_HH, (B, 1)) * rng.uniform(0.9, 1.1, (B, 8))
    pot = (np.arange(B) % 2).astype(np.int32)
    for model in (K.MODEL_NNF, K.MODEL_NND):
        g = ion.solve(model, params, pv, torch.tensor([[0.0, 1.0]], dtype=torch.float32 if f32 else torch.float64), te,
                      weights=w, mlp_layers=L, mlp_width=N, prot_t0=0.0, prot_dt=1.0, prot_of_traj=pot, current=True, tile_waves=tile)
        # (TAIL slot: bit 2 = two column sets, bit 3 = the lean variant, which this call -- uniform grids, no step log -- qualifies for)
        assert any(("13, 13, %d>" % t) in g.kernel for t in ((4, 12) if tile == 8 else (0, 8))), g.kernel
        o = oracle.solve(model, params, pv, [0.0, 1.0], te, weights=w, mlp_layers=L, mlp_width=N, prot_t0=0.0, prot_dt=1.0,
                         prot_of_traj=pot, state_f32=f32, nthreads=8)
        assert np.array_equal(g.status.cpu().numpy(), o["status"]) and np.array_equal(g.stats.cpu().numpy(), o["stats"])
        assert np.array_equal(g.y.double().cpu().numpy(), o["y"], equal_nan=True)
        cur = np.stack([oracle.current(o["y"][b], oracle.protocol_v(pv[pot[b]], te, prot_t0=0.0, prot_dt=1.0)[0], state_f32=f32) for b in range(B)])
        assert np.array_equal(g.i.cpu().numpy(), cur)


@pytest.mark.parametrize("f32", [False, True])
def test_six_state_model_at_large_batches(ion, gpu, oracle, f32):
    """The 6-state kernel (one wavefront per SIMD, packed dense output) over three residency rounds: 24 random trajectories of a
    200 000-trajectory batch against the oracle bit for bit, plain emission and table epilogue; repeated inputs repeat their bits."""
    B = 200000
    rng = np.random.default_rng(B + f32)
    pv = np.stack([K.activation(v)[1][:1201] for v in (-40, 0, 40)])
    half = np.tile(K.P_M6, (B // 2, 1)) * rng.uniform(0.8, 1.25, (B // 2, 12))
    params = np.concatenate([half, half])
    pot = np.tile((np.arange(B // 2) % 3).astype(np.int32), 2)
    y0 = torch.tensor([[0.0, 1.0, 0.0, 0.0, 0.0, 0.0]], dtype=torch.float32 if f32 else torch.float64)
    pick = rng.choice(B // 2, 24, replace=False)
    te = np.arange(0, 1201, 5) * 1.0
    ref = rng.normal(0, 0.3, (3, te.size))
    for name, kw in (("plain", {}), ("table", dict(current=True, sse_ref=ref, obs_open_state_only=True))):
        sol = ion.solve(K.MODEL_MARKOV6, params, pv, y0, te, prot_t0=0.0, prot_dt=1.0, prot_of_traj=pot, **kw)
        # plain = states only on an exact grid: the lean variant (TAIL slot 1) where the dispatcher prefers it, else the general one
        assert any(", 1, 0, 0, 0, %d>" % t in sol.kernel for t in ({"plain": (0, 1), "table": (2,)}[name])) and ("float" if f32 else "double") in sol.kernel, sol.kernel
        o = oracle.solve(K.MODEL_MARKOV6, params[pick], pv, [0.0, 1.0, 0.0, 0.0, 0.0, 0.0], te, prot_t0=0.0, prot_dt=1.0,
                         prot_of_traj=pot[pick], nthreads=8, state_f32=f32)
        assert np.array_equal(sol.y[pick].double().cpu().numpy(), o["y"]) and np.array_equal(sol.stats[pick].cpu().numpy(), o["stats"])
        assert torch.equal(sol.y[: B // 2], sol.y[B // 2:]) and bool((sol.status == 0).all())


def test_odeint_adjoint_is_the_stabilised_sweep(ion, gpu):
    """`from torchdiffeq import odeint_adjoint` (train-s1.py:29-32).  Forward values: odeint's bits, with or without a gradient request
    (round 5: torchdiffeq's adjoint returns odeint's forward exactly, so the cap is opt-in).  With adjoint_options={"max_step": "auto"}
    the step sequence is capped at 3 / lambda_max, so the rate-parameter gradient of a long hold stays bounded in fp32 state and no warning is
    raised; as the tolerance tightens the capped discrete gradient converges (to the continuous adjoint's value): rtol 1e-7 against
    rtol 1e-10 agree to 1e-4 relative, and both agree with central finite differences of the forward solve."""
    import ref_style_modules as M
    from torchdiffeq import odeint, odeint_adjoint
    tp = np.arange(0.0, 6000.1, 0.5)
    vp = np.full(tp.size, -80.0)
    vp[(tp >= 200) & (tp < 1200)] = 30.0                          # 1 s step, then a 4.8 s hold at -80 mV
    te = torch.arange(0.0, 6000.0, 25.0)

    def make(dtype, p7=None):
        f = M.HodgkinHuxley(K.P_HH)
        f.set_fixed_form_voltage_protocol(tp, vp)
        f.p7 = torch.tensor(float(K.P_HH[6]) if p7 is None else p7, dtype=torch.float64, requires_grad=True)
        return f, torch.tensor([[0.0, 1.0]], dtype=dtype)

    f, y0 = make(torch.float32)
    with torch.no_grad():
        plain = odeint(f, y0, te)
        assert torch.equal(odeint_adjoint(f, y0, te), plain)
    with pytest.warns(RuntimeWarning, match="UNCAPPED"):          # default: reference-exact forward, the uncapped derivative warns
        yg = odeint_adjoint(f, y0, te)
    assert yg.requires_grad and torch.equal(yg.detach(), plain)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        assert torch.equal(odeint(f, y0, te).detach(), plain)
    grads = {}
    for dtype, rtol in ((torch.float32, 1e-7), (torch.float64, 1e-7), (torch.float64, 1e-10)):
        f, y0 = make(dtype)
        with warnings.catch_warnings():
            warnings.simplefilter("error", RuntimeWarning)
            y = odeint_adjoint(f, y0, te.to(dtype), rtol=rtol, atol=rtol * 1e-2, adjoint_options={"max_step": "auto"})
        (y[:, 0, 0] * y[:, 0, 1]).double().sum().backward()
        grads[(dtype, rtol)] = float(f.p7.grad)
        assert np.isfinite(grads[(dtype, rtol)])
    ref = grads[(torch.float64, 1e-10)]
    assert abs(grads[(torch.float64, 1e-7)] - ref) <= 1e-4 * abs(ref), grads
    assert abs(grads[(torch.float32, 1e-7)] - ref) <= 2e-2 * abs(ref), grads
    # central finite differences of the (capped, tight) forward solve
    h = 1e-4 * float(K.P_HH[6])
    vals = []
    for dp in (+h, -h):
        f, y0 = make(torch.float64, float(K.P_HH[6]) + dp)
        with torch.no_grad():
            y = odeint(f, y0, te.double(), rtol=1e-11, atol=1e-13, options={"max_step": "auto"})
        vals.append(float((y[:, 0, 0] * y[:, 0, 1]).sum()))
    fd = (vals[0] - vals[1]) / (2 * h)
    assert abs(fd - ref) <= 1e-4 * abs(ref), (fd, ref)


@pytest.mark.parametrize("case", ["hh_states", "hh_objective", "hh_current", "m6_states", "m6_objective", "s00_tile", "s00_tile32", "tiny64", "tiny16", "s09"])
def test_launch_order_is_a_schedule_not_a_permutation_of_the_results(ion, gpu, case):
    """ionode_desc.launch_order (ABI 6): launch slot s integrates trajectory order[s]; inputs and outputs stay at the trajectory's
    own index.  Every kernel family, ragged last tile / wavefront: a random order returns the bits of index order -- states, current,
    fused objective, status, statistics."""
    capi = ion.capi
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(len(case))
    pvs = np.stack([K.activation(v)[1][:1501] for v in (-40, -10, 20, 40)])
    te = torch.arange(0, 1500, 2.5, dtype=torch.float64, device=dev)
    kw = dict(prot_t0=0.0, prot_dt=1.0)
    if case.startswith("hh"):
        model, p0, y0, B = capi.MODEL_HH2, K.P_HH, [0.0, 1.0], 3 * 64 + 37
    elif case.startswith("m6"):
        model, p0, y0, B = capi.MODEL_MARKOV6, K.P_M6, [0.0, 1.0, 0, 0, 0, 0], 2 * 64 + 5
    else:
        model, p0, y0 = capi.MODEL_NNF, K.P_HH, [0.0, 1.0]
        L, N, B = {"s00_tile": (5, 200, 16 * 5 + 3), "s00_tile32": (2, 200, 32 * 3 + 7), "tiny64": (5, 10, 64 * 2 + 9),
                   "tiny16": (5, 10, 16 * 4 + 2), "s09": (5, 100, 16 * 3 + 1)}[case]
        w = np.random.default_rng(3).normal(0, 0.1, 2 * N + N + L * (N * N + N) + N + 1).astype(np.float32)
        kw.update(mlp_packed=torch.from_numpy(capi.mlp_pack(w, L, N)).to(dev), mlp_layers=L, mlp_width=N,
                  tile_waves={"s00_tile": 4, "s00_tile32": 8, "tiny64": 64, "tiny16": 1, "s09": 0}[case])
    if case.endswith("objective"):
        kw.update(sse_ref=torch.from_numpy(rng.normal(0, 0.3, (4, te.numel()))).to(dev), states=False)
    if case.endswith("current") or case.startswith("s00") or case == "s09":
        kw.update(current=True)
    if case.startswith("hh") or case.startswith("m6"):
        kw.update(tile_waves=64)
    params = torch.from_numpy(p0[None, :] * rng.uniform(0.8, 1.25, (B, p0.size))).to(dev)
    pv = torch.from_numpy(pvs).to(dev)
    y0t = torch.tensor([y0], dtype=torch.float64, device=dev).repeat(B, 1).contiguous()
    pot = torch.from_numpy(rng.integers(0, 4, B).astype(np.int32)).to(dev)
    base = capi.dopri5(model, params, pv, y0t, te, prot_of_traj=pot, launch_order=None, **kw)
    order = torch.from_numpy(rng.permutation(B).astype(np.int32)).to(dev)
    perm = capi.dopri5(model, params, pv, y0t, te, prot_of_traj=pot, launch_order=order, **kw)
    auto = capi.dopri5(model, params, pv, y0t, te, prot_of_traj=pot, launch_order=capi._protocol_major(pot), **kw)
    assert perm["kernel"] == base["kernel"]
    for other in (perm, auto):
        for k in ("y", "i", "sse", "status", "stats"):
            if base.get(k) is not None:
                assert torch.equal(base[k], other[k]), (case, k)
    assert bool((base["status"] == 0).all())


def test_solve_launch_order_keeps_the_callers_order(ion, gpu):
    """batched.solve(launch_order=perm): the schedule of solve(order=perm) without the gather -- every field of the Solution is in
    the caller's order and equals the plain launch bit for bit; cost-sorted order from the previous solve's own counters."""
    B, Nt = 80, 6001
    pv = ion.protocols.sinewave(ion.protocols.sinewave_scales(0, B), n_samples=Nt, dt=0.1, xp=torch, device=gpu)
    params = np.tile(K.P_HH, (B, 1))
    te = np.arange(0, Nt, 10) * 0.1
    kw = dict(weights=K.load_weights("s1"), mlp_layers=5, mlp_width=200, prot_t0=0.0, prot_dt=0.1, current=True)
    y0 = torch.tensor([[0.0, 1.0]], dtype=torch.float64)
    plain = ion.solve(K.MODEL_NNF, params, pv, y0, te, **kw)
    srt = ion.solve(K.MODEL_NNF, params, pv, y0, te, launch_order=ion.schedule.lpt_order(plain.stats[:, 2]), **kw)
    assert srt.order is None
    for name in ("y", "i", "status", "stats"):
        assert torch.equal(getattr(plain, name), getattr(srt, name)), name
    with pytest.raises(ion.IonodeError):
        ion.solve(K.MODEL_NNF, params, pv, y0, te, launch_order=np.zeros(B, dtype=np.int64), **kw)
    with pytest.raises(ion.IonodeError):
        ion.solve(K.MODEL_NNF, params, pv, y0, te, launch_order=np.arange(B), order=np.arange(B), **kw)


def test_rccl_path_runs_under_the_drivers_launcher_with_one_rank(ion, gpu):
    """The driver launches N > 1 as `python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 ... bench.py
    --gpus N`, backend nccl (= RCCL).  A 1-GPU box cannot hold two RCCL ranks, but it can run that exact launch with one rank and the
    process group forced on: RCCL initialises, the timing / loss / status all-reduces of the N > 1 path execute on the device, and
    the line reports the backend and world size torch.distributed saw."""
    import json
    import os
    import socket
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(root, "bench.py"), "--gpus", "1", "--force-dist", "--batch", "64", "--nt", "5001",
           "--steps", "2", "--warmup", "1", "--full", "--no-cpu-baseline", "--no-extra-legs"]
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env["HSA_ENABLE_IPC_MODE_LEGACY"] = "0"
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    res = json.loads(lines[0])
    assert res["config"]["dist_backend"] == "nccl" and res["config"]["dist_world_size"] == 1
    assert res["n_gpus"] == 1 and res["config"]["trajectories_ok"] == 64 and res["value"] > 0
    # the self-explaining multi-rank fields ride on this line too (all-gather + 16-byte all-reduce through RCCL, sharded objective leg)
    assert len(res["config"]["per_rank_ms"]) == 1 and res["config"]["allreduce_16B_us"] > 0
    assert "error" not in res["config"]["objective_sharded"], res["config"]["objective_sharded"]


@pytest.mark.parametrize("model_name", ["s1", "d2"])
def test_two_phase_sweep_equals_the_one_phase_sweep(ion, gpu, model_name):
    """grad.solve(two_phase=...).  A stage's vector-Jacobian product is linear in its seed, a scalar per trajectory: the two-phase
    sweep computes the unit-seed products of every (tile, step) ahead on the whole chip (ionode_dopri5_backward_recompute), walks
    the steps with the adjoint algebra alone (ionode_dopri5_backward_sweep) and scales the records by the seeds in the reduction
    (ionode_grad_reduce_unit).  The seed then multiplies at the end of the fp32 product instead of at its start: dL/dW, dL/dp,
    dL/dy0 equal the one-phase sweep's to fp32 rounding (1e-5 relative, against the checker's 1e-4) -- with one chunk, with a record
    budget small enough for several chunks (double-buffered records and packets, phase A one chunk ahead; chunking itself is
    bit-invariant for dL/dp and dL/dy0), ragged last tile, fp32 and fp64 state."""
    grad = importlib.import_module("neural-ode-ion-channels_amd.grad")
    capi = ion.capi
    B, Nt = 37, 4001
    P = ion.protocols
    pv = P.sinewave(P.sinewave_scales(0, B), n_samples=Nt, xp=torch, device=gpu)
    model = capi.MODEL_NNF if model_name == "s1" else capi.MODEL_NND
    p0 = K.MODELS[model_name][4]
    te = torch.arange(0, Nt, 4, dtype=torch.float64, device=gpu) * 0.1

    def rel(a, b):
        a, b = a.double(), b.double()
        return float((a - b).norm() / b.norm())

    for sdt in (torch.float32, torch.float64):
        got = {}
        small = 3 * 6 * 40 * int(capi.lib().ionode_grad_record_floats(5, 200)) * 4     # ~20 iterations per chunk and buffer
        for tag, kw in (("one", dict(two_phase=False)), ("two", dict(two_phase=True)),
                        ("one_chunked", dict(two_phase=False, record_budget_bytes=small)),
                        ("two_chunked", dict(two_phase=True, record_budget_bytes=small))):
            w = torch.from_numpy(K.load_weights(model_name).copy()).to(gpu).requires_grad_(True)
            params = torch.from_numpy(np.tile(p0, (B, 1)) * np.random.default_rng(5).uniform(0.9, 1.1, (B, 8))).to(gpu).requires_grad_(True)
            y0 = torch.tensor([[0.0, 1.0]], dtype=sdt, device=gpu).repeat(B, 1).requires_grad_(True)
            with warnings.catch_warnings():
                warnings.simplefilter("ignore", RuntimeWarning)
                y, status = grad.solve(model, w, params, pv, y0, te, mlp_layers=5, mlp_width=200, prot_t0=0.0, prot_dt=0.1, **kw)
            assert bool((status == 0).all())
            (y[..., 0] * y[..., 1]).double().sum().backward()
            got[tag] = (w.grad.clone(), params.grad.clone(), y0.grad.clone())
        for ref, tag in (("one", "two"), ("one_chunked", "two_chunked")):
            for a, b in zip(got[tag], got[ref]):
                assert rel(a, b) < 1e-5, (tag, sdt, rel(a, b))
        # chunking changes the slab partition of the weight-gradient reduction, not dL/dp and dL/dy0 -- in either form
        for one in ("one", "two"):
            assert torch.equal(got[one][1], got[one + "_chunked"][1]) and torch.equal(got[one][2], got[one + "_chunked"][2])
            assert rel(got[one][0], got[one + "_chunked"][0]) < 1e-5
