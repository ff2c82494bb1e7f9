"""-m gpu: the fused objective's second kind, objective="sae" -- per trajectory sum_k |i_k - ref[protocol][k]|, n_out times the
reference's prediction loss torch.mean(torch.abs(pred_yo - data)) -- in every forward kernel that carries the fused sum of squares,
against the sum over the stored current trace.  Tolerance: the project's own for a fused sum against the trace sum, rtol 1e-12,
atol 0 (tests/test_gpu_round2.py): a sum of non-negative terms like the squares, so no worse conditioned.  Shapes of that file: the
smallest at which every emission path runs (1-sample steps, steps of more than 64 samples, ragged last tile)."""
import ctypes as C

import numpy as np
import pytest
import torch

import kat_cases as K
from test_oracle_kats import _kat_loss

pytestmark = pytest.mark.gpu
RTOL = 1e-12


def _rand_weights(L, N, seed):
    rng = np.random.default_rng(seed)
    return rng.normal(0, 0.1, 2 * N + N + L * (N * N + N) + N + 1).astype(np.float32)


def _t(x, gpu, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(x)).to(gpu)
    return t if dtype is None else t.to(dtype).contiguous()


def _three_ways(ion, gpu, model, params, pv, y0, te, pot, ref, f32, bad, **kw):
    """One batch three times: plain (states only), traces + fused sum, fused sum alone.  Checks both sums against the stored current
    trace, inf for failed trajectories (`bad` among them), states bit-identical to the plain solve.  Returns (traces run, lean run)."""
    capi = ion.capi
    sdt = torch.float32 if f32 else torch.float64
    args = (model, _t(params, gpu), _t(pv, gpu), _t(y0, gpu, sdt), _t(te, gpu))
    common = dict(prot_t0=0.0, prot_dt=1.0, prot_of_traj=_t(pot, gpu), **kw)
    ref_t = _t(ref, gpu)
    plain = capi.dopri5(*args, **{k: v for k, v in common.items() if k != "v_at_outputs"})
    full = capi.dopri5(*args, current=True, sse_ref=ref_t, objective="sae", **common)
    lean = capi.dopri5(*args, states=False, sse_ref=ref_t, objective="sae", **common)
    torch.cuda.synchronize()
    assert lean["y"] is None and lean["i"] is None and lean["sse"] is None and full["sse"] is None
    status = full["status"].cpu().numpy()
    ok = status == 0
    assert not ok[bad] and ok.sum() >= len(ok) // 2
    want = np.abs(full["i"].cpu().numpy() - ref[pot]).sum(1)
    for r in (full, lean):
        got = r["sae"].cpu().numpy()
        assert np.array_equal(r["status"].cpu().numpy(), status)
        assert np.isinf(got[~ok]).all() and (got[~ok] > 0).all()
        print("sae rel. deviation from the trace sum:", np.abs(got[ok] / want[ok] - 1).max(), r["kernel"])
        np.testing.assert_allclose(got[ok], want[ok], rtol=RTOL, atol=0)
    assert torch.equal(full["y"].view(torch.uint8), plain["y"].view(torch.uint8))
    assert torch.equal(full["stats"], plain["stats"]) and torch.equal(lean["stats"], plain["stats"])
    return full, lean


# ---- 1. closed-form kernels: table and general variant ----

@pytest.mark.parametrize("table", [True, False])
@pytest.mark.parametrize("model,f32", [(K.MODEL_HH2, True), (K.MODEL_HH2, False), (K.MODEL_MARKOV6, True), (K.MODEL_MARKOV6, False)])
def test_closed_form_kernels(ion, gpu, model, f32, table):
    rng = np.random.default_rng(17)
    B = 37
    pv = np.stack([K.activation(v)[1] for v in (-20, 20, 60)])
    te = K.activation(0)[2][:3001]
    pot = (np.arange(B) % 3).astype(np.int32)
    ref = rng.normal(0, 0.5, (3, te.size))
    if model == K.MODEL_MARKOV6:
        params, y0, kw = np.tile(K.P_M6, (B, 1)) * rng.uniform(0.8, 1.2, (B, 12)), [0, 1.0, 0, 0, 0, 0], dict(obs_open_state_only=True)
    else:
        params, y0, kw = np.tile(K.P_HH, (B, 1)) * rng.uniform(0.8, 1.2, (B, 8)), [0.0, 1.0], {}
    y0b = np.tile(y0, (B, 1)).astype(np.float64)
    y0b[4, 1] = np.nan
    full, lean = _three_ways(ion, gpu, model, params, pv, y0b, te, pot, ref, f32, 4, obs_g=1.3, obs_e=-88.0,
                             v_at_outputs="auto" if table else None, **kw)
    for r in (full, lean):
        assert (r["v_at_outputs"] is not None) == table
        assert (", 1, 16, 0, 0, %d>" % (2 if table else 0)) in r["kernel"] and ("float" if f32 else "double") in r["kernel"], r["kernel"]


# ---- 2. N <= 16 nets, 16 and 64 per wavefront ----

@pytest.mark.parametrize("model,L,N,f32", [(K.MODEL_NNF, 5, 10, False), (K.MODEL_NND, 3, 16, True)])
def test_tiny_nets_in_both_geometries(ion, gpu, model, L, N, f32):
    rng = np.random.default_rng(7 * L + N)
    B = 150
    w = rng.normal(0, 0.3, 2 * N + N + L * (N * N + N) + N + 1).astype(np.float32)
    pv = np.stack([K.atau(30)[1], K.atau(300)[1], K.activation(20)[1][: K.atau(30)[1].size]])
    te = K.atau(30)[2][:1201]
    params = np.tile(K.P_NN_D if model == K.MODEL_NND else K.P_HH, (B, 1)) * rng.uniform(0.85, 1.2, (B, 8))
    y0 = np.tile(K.NN_Y0, (B, 1)).astype(np.float64)
    y0[77, 0] = np.nan
    pot = rng.integers(0, 3, B).astype(np.int32)
    ref = rng.normal(0, 0.2, (3, te.size))
    packed = _t(ion.capi.mlp_pack(w, L, N), gpu)
    sums = {}
    for tw in (64, 1):
        full, lean = _three_ways(ion, gpu, model, params, pv, y0, te, pot, ref, f32, 77, mlp_packed=packed, mlp_layers=L, mlp_width=N,
                                 tile_waves=tw, max_total_steps=20000)
        assert (", 1, 64, 1, %d, 0>" % (10 if N == 10 else 1) if tw == 64 else ", 1, 1, 1, 1, 0>") in lean["kernel"], lean["kernel"]
        sums[tw] = lean["sae"].cpu().numpy()
    ok = np.isfinite(sums[1])
    np.testing.assert_allclose(sums[64][ok], sums[1][ok], rtol=2 * RTOL, atol=0)   # (both within RTOL of one trace sum)


# ---- 3. MLP tiles ----

TILES = [  # weights, model, L, N, tile_waves, f32, B, what the kernel name holds
    ("s1", K.MODEL_NNF, 5, 200, 4, False, 37, ", 4, 4, 13, 13, "),
    ("d2", K.MODEL_NND, 5, 200, 4, True, 37, ", 4, 4, 13, 13, "),
    ("s1", K.MODEL_NNF, 5, 200, 8, False, 37, ", 4, 4, 13, 13, "),
    ("d2", K.MODEL_NND, 5, 200, 2, False, 37, ", 4, 4, 13, 13, "),
    ("s1", K.MODEL_NNF, 5, 200, 16, False, 3, ", 4, 4, 13, 13, "),
    (None, K.MODEL_NNF, 2, 100, 4, True, 37, ", 4, 4, 7, 7, "),
    (None, K.MODEL_NND, 1, 500, 4, False, 37, ", 4, 8, 32, 4, "),
    (None, K.MODEL_NNF, 3, 48, 4, False, 37, ", 4, 1, 0, 1, "),
]
TILE_BITS = {4: 0, 8: 4, 2: 16, 16: 32}    # KernelForm's TAIL bits of the N = 200 tiles (8: lean, on a verified uniform output grid)


@pytest.mark.parametrize("name,model,L,N,tw,f32,B,form", TILES)
def test_mlp_tiles(ion, gpu, name, model, L, N, tw, f32, B, form):
    rng = np.random.default_rng(100 * L + N + tw)
    w = K.load_weights(name) if name else _rand_weights(L, N, 7 * L + N)
    pv = np.stack([K.activation(v)[1] for v in (-20, 20, 60)])
    te = K.activation(0)[2][:1201]
    pot = (np.arange(B) % 3).astype(np.int32)
    ref = rng.normal(0, 0.5, (3, te.size))
    params = np.tile(K.P_NN_D if model == K.MODEL_NND else K.P_HH, (B, 1)) * rng.uniform(0.8, 1.2, (B, 8))
    y0 = np.tile(K.NN_Y0, (B, 1)).astype(np.float64)
    bad = 1 if B == 3 else 4
    y0[bad, 1] = np.nan
    full, lean = _three_ways(ion, gpu, model, params, pv, y0, te, pot, ref, f32, bad, mlp_packed=_t(ion.capi.mlp_pack(w, L, N), gpu),
                             mlp_layers=L, mlp_width=N, tile_waves=tw, obs_g=1.3, obs_e=-88.0, max_total_steps=20000)
    for r in (full, lean):
        assert form in r["kernel"] and ("float" if f32 else "double") in r["kernel"] and r["composed"] is None, r["kernel"]
        if N == 200:
            tail = int(r["kernel"].split(",")[-1].split(">")[0])
            assert (tail & ~8) == TILE_BITS[tw], r["kernel"]
            # the lean 16-tile (TAIL 8: it shrinks and defers, and fills the register file) is compiled for the squares alone: absolute
            # residuals run the 16-tile's general variant, every other tile its lean one
            assert tail == (0 if tw == 4 else TILE_BITS[tw] | 8), r["kernel"]


# ---- 4. several weight sets in one launch ----

def test_several_weight_sets(ion, gpu):
    rng = np.random.default_rng(41)
    nset, per, L, N = 3, 16, 5, 200
    B = nset * per - 5      # the last set's tile is ragged
    ws = np.stack([_rand_weights(L, N, 7 * k + N) for k in range(nset)])
    pv = np.stack([K.atau(30)[1], K.atau(300)[1], K.activation(20)[1][: K.atau(30)[1].size]])
    te = K.atau(30)[2][:901]
    params = np.tile(K.P_HH, (B, 1)) * rng.uniform(0.9, 1.1, (B, 8))
    pot = rng.integers(0, 3, B).astype(np.int32)
    ref = rng.normal(0, 0.3, (3, te.size))
    kw = dict(prot_t0=0.0, prot_dt=1.0, max_total_steps=20000, mlp_layers=L, mlp_width=N, sse_ref=ref, states=False, objective="sae",
              tile_waves=4)
    y0 = torch.tensor([K.NN_Y0], dtype=torch.float64)
    sol = ion.solve(K.MODEL_NNF, params, pv, y0, te, weights=ws, traj_per_image=per, prot_of_traj=pot, **kw)
    assert sol.sse is None and sol.y is None and bool((sol.status == 0).all())
    for k in range(nset):
        lo, hi = k * per, min(B, (k + 1) * per)
        one = ion.solve(K.MODEL_NNF, params[lo:hi], pv, y0, te, weights=ws[k], prot_of_traj=pot[lo:hi], **kw)
        assert one.kernel == sol.kernel
        assert torch.equal(sol.sae[lo:hi], one.sae) and bool(torch.isfinite(one.sae).all()) and bool((one.sae > 0).all()), k
    assert not torch.equal(sol.sae[:per - 5], sol.sae[2 * per:])     # (the sets differ: the right image went to the right tile)


# ---- 5. squares through the new entry point; launch order ----

def _cases_5(ion, gpu):
    rng = np.random.default_rng(23)
    B, P = 53, 5
    pv = np.stack([K.activation(v)[1] for v in (-40, -20, 0, 20, 40)])
    te = K.activation(0)[2][:1201]
    y0 = np.tile([0.0, 1.0], (B, 1)) + rng.uniform(0, 0.05, (B, 2)) * [1, -1]
    y0[9, 0] = np.nan
    common = dict(prot_t0=0.0, prot_dt=1.0, prot_of_traj=_t(rng.integers(0, P, B).astype(np.int32), gpu),
                  sse_ref=_t(rng.normal(0, 1, (P, te.size)), gpu), current=True)
    params = _t(np.tile(K.P_HH, (B, 1)) * rng.uniform(0.8, 1.25, (B, 8)), gpu)
    perm = _t(rng.permutation(B).astype(np.int32), gpu)
    return {
        "hh2": ((K.MODEL_HH2, params, _t(pv, gpu), _t(y0, gpu), _t(te, gpu)), common, perm),
        "n200": ((K.MODEL_NNF, params, _t(pv, gpu), _t(y0, gpu), _t(te, gpu)),
                 dict(common, mlp_packed=_t(ion.capi.mlp_pack(K.load_weights("s1"), 5, 200), gpu), mlp_layers=5, mlp_width=200, tile_waves=4), perm),
    }


@pytest.mark.parametrize("which", ["hh2", "n200"])
def test_squares_through_the_new_entry_point_are_the_composed_launch(ion, gpu, which):
    capi = ion.capi
    args, kw, _ = _cases_5(ion, gpu)[which]
    r = capi.dopri5(*args, objective="sse", **kw)
    torch.cuda.synchronize()
    assert r["sae"] is None and r["sse"] is not None
    # the same descriptor, fresh outputs, through ionode_dopri5_composed directly
    d = type(r["desc"]).from_buffer_copy(r["desc"])
    out = {k: torch.full_like(r[k], -7) for k in ("y", "i", "status", "stats", "sse")}
    d.sse_out = out["sse"].data_ptr()
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    rc = capi.lib().ionode_dopri5_composed(C.byref(d), p(kw.get("mlp_packed")), p(args[1]), p(args[2]), None, p(kw["prot_of_traj"]), p(args[3]),
                                           p(args[4]), p(out["y"]), p(out["i"]), p(out["status"]), p(out["stats"]),
                                           C.c_void_p(torch.cuda.current_stream(gpu).cuda_stream), None, 0, 0)
    assert rc == 0, capi.last_error()
    torch.cuda.synchronize()
    assert capi.lib().ionode_last_kernel_name().decode() == r["kernel"]
    assert bool(torch.isinf(r["sse"][9])) and int(torch.isfinite(r["sse"]).sum()) == r["sse"].numel() - 1
    for k in out:
        assert torch.equal(out[k].view(torch.uint8), r[k].view(torch.uint8)), k


@pytest.mark.parametrize("which", ["hh2", "n200"])
def test_launch_order_does_not_change_sae(ion, gpu, which):
    args, kw, perm = _cases_5(ion, gpu)[which]
    base = ion.capi.dopri5(*args, objective="sae", launch_order=None, **kw)
    moved = ion.capi.dopri5(*args, objective="sae", launch_order=perm, **kw)
    torch.cuda.synchronize()
    assert moved["kernel"] == base["kernel"] and bool(torch.isinf(base["sae"][9]))
    for k in ("sae", "y", "i", "status", "stats"):
        assert torch.equal(base[k].view(torch.uint8), moved[k].view(torch.uint8)), k


# ---- 6. every sample once: the trace of the same solve as the reference ----

@pytest.mark.parametrize("which", ["hh2 table", "n200 16-tile"])
def test_every_sample_enters_once(ion, gpu, which):
    """P = B, one protocol and one reference row per trajectory, the reference being the stored current of the same solve: a sample
    that were skipped, or counted twice, or taken from a neighbour's row would leave its |i| behind.  The fused and the stored current
    are one expression, so 0.0 is what is expected; the bound asked for is 1e-12 of sum |i|."""
    capi = ion.capi
    rng = np.random.default_rng(3)
    B = 20
    pv = np.stack([K.activation(v)[1] for v in np.linspace(-50, 60, B)])
    te = K.activation(0)[2][:1201]
    args = (K.MODEL_HH2 if which == "hh2 table" else K.MODEL_NNF, _t(np.tile(K.P_HH, (B, 1)) * rng.uniform(0.8, 1.2, (B, 8)), gpu), _t(pv, gpu),
            _t(np.tile([0.0, 1.0], (B, 1)), gpu), _t(te, gpu))
    kw = dict(prot_t0=0.0, prot_dt=1.0, prot_of_traj=torch.arange(B, dtype=torch.int32, device=gpu), obs_g=1.3, obs_e=-88.0)
    if which == "hh2 table":
        first = capi.dopri5(*args, current=True, v_at_outputs=None, **kw)
        kw["v_at_outputs"] = capi.protocol_at_outputs(first["desc"], args[2], None, args[4])
    else:
        kw.update(mlp_packed=_t(capi.mlp_pack(K.load_weights("s1"), 5, 200), gpu), mlp_layers=5, mlp_width=200, tile_waves=4)
        first = capi.dopri5(*args, current=True, **kw)
    r = capi.dopri5(*args, states=False, sse_ref=first["i"], objective="sae", **kw)
    torch.cuda.synchronize()
    assert (", 1, 16, 0, 0, 2>" if which == "hh2 table" else ", 4, 4, 13, 13, ") in r["kernel"], r["kernel"]
    assert bool((r["status"] == 0).all())
    mass = first["i"].abs().sum(1)
    print(which, "largest sae / sum |i|:", float((r["sae"] / mass).max()), "largest sae:", float(r["sae"].max()))
    assert bool((mass > 0).all()) and bool((r["sae"] >= 0).all())
    assert bool((r["sae"] <= 1e-12 * mass).all())


# ---- 7. the reference's logged losses, on the device ----

CONVERGED_BRANCH_MAY_TAKE = {("deact", "-70.0"), ("deact", "-50.0")}     # kat_cases.py names them; no others


@pytest.mark.parametrize("sec,key,case", K.all_cases(), ids=[f"{s} {k}" for s, k, _ in K.all_cases()])
def test_logged_s1_prediction_losses_from_one_fused_call(ion, gpu, oracle, sec, key, case):
    """train-s1.py --pred: loss = torch.mean(torch.abs(pred_yo - data)).  The ground-truth model's current trace is the data; the
    NN-f solve returns sae, and loss = sae / Nt -- no trace of the prediction is written."""
    capi = ion.capi
    tm, tp, ty0, nm, npar = K.MODELS["s1"]
    pt, pv, te = case
    dev = lambda x, dt=torch.float64: _t(np.atleast_2d(np.asarray(x, dtype=np.float64)), gpu, dt)
    pt_t, te_t = _t(pt, gpu), _t(te, gpu)
    truth = capi.dopri5(tm, dev(tp), dev(pv), dev(ty0, torch.float32), te_t, prot_t=pt_t, current=True)
    r = capi.dopri5(nm, dev(npar), dev(pv), dev(K.NN_Y0, torch.float32), te_t, prot_t=pt_t, sse_ref=truth["i"], objective="sae", states=False,
                    mlp_packed=_t(capi.mlp_pack(K.load_weights("s1"), K.MLP_L, K.MLP_N), gpu), mlp_layers=K.MLP_L, mlp_width=K.MLP_N)
    torch.cuda.synchronize()
    assert int(truth["status"][0]) == 0 and int(r["status"][0]) == 0 and r["y"] is None and r["i"] is None
    loss = float(r["sae"][0]) / te.size
    logged = K.expected(K.load_kats(), "s1", sec, key)
    took = []

    def converged():
        took.append(1)
        return _kat_loss(oracle, "s1", case, False, 1e-10, 1e-12)
    want = _kat_loss(oracle, "s1", case)
    print(f"s1 {sec} {key}: device {loss:.9f} oracle {want:.9f} logged {logged:.6f}")
    assert K.kat_within_tolerance(loss, logged, converged), f"s1 {sec} {key}: {loss:.6f} vs logged {logged:.6f}"
    assert not took or (sec, key) in CONVERGED_BRANCH_MAY_TAKE, (sec, key)
    assert abs(loss - want) <= RTOL * want, (loss, want)
