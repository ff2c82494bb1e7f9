"""-m gpu: the fused sum-of-squares objective gradient of the NN models (grad.sum_of_squares with weights_flat: the G_c kernel
ionode_dopri5_backward_sse_gc, the recompute and walk kernels without grad_y).  Checked against the fused forward of batched.solve
(values), against the materialised route grad.solve -> torch current -> sum of squares -> autograd, and against autograd through the
torch replay of the oracle's accepted steps (tests/grad_check.py).  Problems and references: tests/sse_nn_cases.py.

Tolerances (the project's own): GRAD_REL_TOL against the checker and in fp32 state (tests/test_gpu_grad.py); 1e-5 between the fused
and the materialised route in fp64 state -- the two differ only by where fp32 roundings of the vector-Jacobian products fall (the
seeds and d net / d x1 pass through fp32: grad.solve's two-phase against one-phase bound); 2e-5 for dL/dW under another split-K
order (test_config5_share_at_full_size_gradient_is_additive)."""
import numpy as np
import pytest
import torch

import kat_cases as K
import sse_cases as S
import sse_nn_cases as N

pytestmark = pytest.mark.gpu
GRAD_REL_TOL = 1e-4
ROUTE_TOL = 1e-5
SPLIT_K_TOL = 2e-5
NAN = N.NAN_ROW


def _against_materialised(ion, gpu, c, got, tag):
    m = N.materialised(ion, gpu, c)
    assert np.array_equal(m.st, got.st)
    cols = N.param_cols(c.model)
    e = {"dL/dp": N.rel(got.gp[:, cols], m.gp[:, cols]), "dL/dy0": N.rel(got.gy0, m.gy0), "dL/dW": N.rel(got.gw, m.gw)}
    print(tag, "rel-L2 vs materialised", {k: f"{v:.2e}" for k, v in e.items()})
    assert max(e.values()) <= (GRAD_REL_TOL if c.f32 else ROUTE_TOL), e


@pytest.mark.parametrize("f32", [False, True])
@pytest.mark.parametrize("L,N_,model", [(2, 10, K.MODEL_NNF), (3, 100, K.MODEL_NND), (1, 200, K.MODEL_NNF), (1, 500, K.MODEL_NND)])
def test_values_and_gradients_against_the_materialised_route(ion, gpu, L, N_, model, f32):
    """One case per compiled width, both state dtypes, an explicit protocol time grid and a uniform one; with 19 trajectories on two
    protocols the G_c kernel reads V(t_k) from the [P, Nt] table (the checker test's seven-row run has none: protocol_v per sample).
    Values equal the fused forward of batched.solve; a NaN y0 fails alone; dL/dp, dL/dy0 and dL/dW equal the materialised route's."""
    for explicit in (True, False):
        c = N.problem(L, N_, model, f32, explicit=explicit)
        tag = f"L={L} N={N_} model {model} {'f32' if f32 else 'f64'} {'explicit' if explicit else 'uniform'}:"
        got = N.fused(ion, gpu, c)
        ok = np.arange(c.B) != NAN
        assert got.st[NAN] != 0 and (got.st[ok] == 0).all()
        assert np.isinf(got.sse[NAN]) and np.all(got.gp[NAN] == 0) and np.all(got.gy0[NAN] == 0)
        assert np.isfinite(got.gw).all() and np.abs(got.gw).max() > 0
        if model == K.MODEL_NNF:
            assert np.abs(got.gp[:, :4]).max() == 0.0
        want = N.fused_forward(ion, gpu, c).sse.cpu().numpy()
        assert np.isinf(want[NAN])
        assert np.all(np.abs(got.sse[ok] - want[ok]) <= 1e-12 * np.abs(want[ok])), np.max(np.abs(got.sse[ok] / want[ok] - 1))
        # the failing trajectory leaves the others unchanged
        fixed = N.problem(L, N_, model, f32, explicit=explicit)
        fixed.y0[NAN, 0] = 0.1
        got2 = N.fused(ion, gpu, fixed)
        assert (got2.st == 0).all()
        assert np.array_equal(got2.sse[ok], got.sse[ok]) and np.array_equal(got2.gp[ok], got.gp[ok]) and np.array_equal(got2.gy0[ok], got.gy0[ok])
        _against_materialised(ion, gpu, c, got, tag)


@pytest.mark.parametrize("f32", [False, True])
@pytest.mark.parametrize("L,N_,model", [(2, 10, K.MODEL_NND), (1, 200, K.MODEL_NNF)])
def test_gradients_against_the_checker(ion, gpu, oracle, L, N_, model, f32):
    """Every third healthy trajectory: autograd through the torch replay of the oracle's accepted steps, the sum of squares formed in
    torch fp64.  dL/dW: the fused route once more on the checked rows (seven of them: no voltage table, protocol_v per sample)."""
    torch.set_num_threads(8)
    c = N.problem(L, N_, model, f32)
    got = N.fused(ion, gpu, c)
    worst, ew = N.check_against_checker(ion, gpu, oracle, c, got, GRAD_REL_TOL)
    print(f"L={L} N={N_} model {model} {'f32' if f32 else 'f64'}: worst rel-L2 vs checker dL/dp, dL/dy0 {worst:.2e}, dL/dW {ew:.2e}")


DENSE = np.arange(0.0, 140.0, 0.05)   # 2800 samples over 140 ms of a step protocol: tens of samples per accepted step, none in the smallest


def _dense(f32=False):
    return N.problem(2, 10, K.MODEL_NNF, f32, te=DENSE)


@pytest.fixture(scope="module")
def dense_default(ion, gpu):
    c = _dense()
    return c, N.fused(ion, gpu, c)


def test_grid_that_reaches_the_corners_of_the_gc_kernel(ion, gpu, oracle, dense_default):
    """Steps with more than 64 samples (the kernel's second pass), with exactly one and with none, asserted on the oracle's accepted
    steps; against the materialised route and the checker."""
    c, got = dense_default
    counts = []
    for b in range(c.B):
        if b != NAN:
            counts += [n for _, n in S.samples_per_step(c.te, N.accepted_steps_of(oracle, c, b))]
    counts = np.array(counts)
    assert (counts > 64).any() and (counts == 1).any() and (counts == 0).any(), np.bincount(counts)
    assert got.st[NAN] != 0 and (np.delete(got.st, NAN) == 0).all()
    _against_materialised(ion, gpu, c, got, "dense grid:")
    worst, ew = N.check_against_checker(ion, gpu, oracle, c, got, GRAD_REL_TOL)
    print(f"dense grid: worst rel-L2 vs checker dL/dp, dL/dy0 {worst:.2e}, dL/dW {ew:.2e}")


def test_grid_that_ends_with_the_protocol(ion, gpu, oracle):
    """The last output time is the (uniform) protocol's end, t = 399: the last accepted step overshoots it (stage voltages beyond the
    protocol) and, as every trajectory's last step, has its y1 recomputed.  Against the materialised route and the checker."""
    e = N.problem(2, 10, K.MODEL_NNF, False, te=np.arange(0.0, 399.25, 0.5), explicit=False)
    assert e.te[-1] == 399.0
    t0, dt = N.accepted_steps_of(oracle, e, 0)[-1]
    assert t0 + dt > 399.0                                    # the last accepted step overshoots the protocol's end
    got_e = N.fused(ion, gpu, e)
    _against_materialised(ion, gpu, e, got_e, "grid to the protocol's end:")
    worst, ew = N.check_against_checker(ion, gpu, oracle, e, got_e, GRAD_REL_TOL)
    print(f"grid to the protocol's end: worst rel-L2 vs checker dL/dp, dL/dy0 {worst:.2e}, dL/dW {ew:.2e}")


def test_chunked_backward(ion, gpu, dense_default):
    """The dense-grid problem with the default record budget (one chunk) and with one that cuts the sweep into at least three chunks on
    two buffers: G_c and the sample-0 term per chunk, phase A one chunk ahead.  The sweep itself is chunk-invariant (bit-identical sse,
    dL/dp, dL/dy0); dL/dW moves by the split-K order only.  Two runs of the same call are bit-identical in everything."""
    c, one = dense_default
    pre = N.fused_forward(ion, gpu, c)
    st = pre.status.cpu().numpy()
    n_iter = int(pre.stats[:, 0].cpu().numpy()[st == 0].max()) + 1
    lib = ion.capi.lib()
    tiles, recf, pkd = (c.B + 15) // 16, int(lib.ionode_grad_record_floats(c.L, c.N)), int(lib.ionode_grad_packet_doubles())
    budget = 2 * (tiles * 6 * recf * 4) * ((n_iter + 3) // 4)   # a quarter of the iterations per buffer
    chunk, n_buf, bounds = ion.grad.plan_backward_chunks(n_iter, tiles, recf, pkd, budget, True, True)
    assert len(bounds) >= 3 and n_buf == 2 and bounds[-1][1] == n_iter
    assert len(ion.grad.plan_backward_chunks(n_iter, tiles, recf, pkd, ion.grad.DEFAULT_RECORD_BUDGET, True, True)[2]) == 1
    cut = N.fused(ion, gpu, c, record_budget_bytes=budget)
    assert np.array_equal(cut.sse, one.sse) and np.array_equal(cut.st, one.st)
    assert np.array_equal(cut.gp, one.gp) and np.array_equal(cut.gy0, one.gy0)
    assert N.rel(cut.gw, one.gw) <= SPLIT_K_TOL
    for ref, kw in ((one, {}), (cut, dict(record_budget_bytes=budget))):
        again = N.fused(ion, gpu, c, **kw)
        assert np.array_equal(again.sse, ref.sse) and np.array_equal(again.gp, ref.gp) and np.array_equal(again.gy0, ref.gy0)
        assert np.array_equal(again.gw, ref.gw)


def test_memory_does_not_grow_with_the_output_grid(ion, gpu):
    """NN-f (2 x 10) fp64, 256 x 100 001 samples on the sine-wave protocols: forward + backward peak below the checkpoints + the record
    budget + 64 MiB (one [B, Nt, 2] fp64 array alone is 410 MB: any materialised trace or grad_y fails the bound)."""
    B, Nt, L, N_ = 256, 100001, 2, 10
    budget = 128 << 20
    rng = np.random.default_rng(2)
    pv = ion.protocols.sinewave(ion.protocols.sinewave_scales(0, 4), n_samples=Nt, dt=0.1, xp=torch, device=gpu)
    pot = (torch.arange(B, device=gpu) % 4).to(torch.int32)
    te = torch.arange(Nt, dtype=torch.float64, device=gpu) * 0.1
    params = torch.from_numpy(np.tile(K.P_HH, (B, 1)) * rng.uniform(0.9, 1.1, (B, 8))).to(gpu)
    y0 = torch.tensor([[0.0, 1.0]], dtype=torch.float64, device=gpu).repeat(B, 1)
    ref = torch.from_numpy(rng.normal(0.0, 1.0, (4, Nt))).to(gpu)
    w = N.rand_weights(L, N_, 11 * L + N_)
    cap = ion.grad.stable_step_cap(K.MODEL_NNF, params, pv)
    pre = ion.batched.solve(K.MODEL_NNF, params, pv, y0, te, weights=w, mlp_layers=L, mlp_width=N_, prot_t0=0.0, prot_dt=0.1,
                            prot_of_traj=pot, sse_ref=ref, states=False, max_step=cap)
    most = int(pre.stats[:, 0].max())
    del pre
    ckpt_bytes = B * most * (4 + 8 * 2) * 8
    wt = torch.from_numpy(w.copy()).to(gpu).requires_grad_(True)
    p = params.clone().requires_grad_(True)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(gpu)
    base = torch.cuda.memory_allocated(gpu)
    sse, st = ion.grad.sum_of_squares(K.MODEL_NNF, p, pv, y0, te, ref, prot_t0=0.0, prot_dt=0.1, prot_of_traj=pot, max_step="auto",
                                      ckpt_cap=most, weights_flat=wt, mlp_layers=L, mlp_width=N_, record_budget_bytes=budget)
    sse.sum().backward()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated(gpu) - base
    print(f"{most} accepted steps: checkpoints {ckpt_bytes / 2**20:.0f} MiB, peak {peak / 2**20:.0f} MiB")
    assert bool((st == 0).all()) and bool(torch.isfinite(p.grad).all()) and bool(torch.isfinite(wt.grad).all())
    assert float(wt.grad.abs().max()) > 0
    assert peak < ckpt_bytes + budget + (64 << 20), (peak, ckpt_bytes)
