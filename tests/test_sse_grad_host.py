"""CPU tests of the fused sum-of-squares gradient's host side: the C entry point's argument checks (they return before any
launch) and the sharded evaluateS1 objective under gloo with a stand-in solver."""
import ctypes as C
import importlib
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import kat_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _desc(capi, model, **kw):
    m6 = model == capi.MODEL_MARKOV6
    base = dict(model=model, n_state=6 if m6 else 2, n_out=10, n_traj=20, n_prot=1, prot_n=10, n_params=12 if m6 else 8,
                prot_dt=1.0, rtol=1e-7, atol=1e-9, obs_g=1.0, obs_e=-86.0)
    if model in (capi.MODEL_NNF, capi.MODEL_NND):
        base.update(n_state=2, mlp_layers=1, mlp_width=10)
    base.update(kw)
    return capi.make_desc(**base)


def test_backward_sse_rejects_bad_arguments_before_any_launch(ion):
    capi = ion.capi
    lib = capi.lib()
    assert capi.ABI_VERSION == 10 and lib.ionode_abi_version() == 10
    buf = np.zeros(4096, dtype=np.float64)   # stand-in addresses: every call below returns before anything is dereferenced
    ptr = C.c_void_p(buf.ctypes.data)

    def call(d, grad_sse=ptr):
        return lib.ionode_dopri5_backward_sse(C.byref(d), 0, 1, 1, ptr, ptr, None, None, ptr, ptr, grad_sse, ptr, ptr, ptr, None)

    for model in (capi.MODEL_HH2, capi.MODEL_MARKOV6):
        full = dict(ckpt=buf.ctypes.data, ckpt_cap=4, sse_ref=buf.ctypes.data)
        assert call(_desc(capi, model, **{**full, "sse_ref": None})) == -1            # IONODE_ERR_ARG
        assert call(_desc(capi, model, **full), grad_sse=None) == -1
        assert call(_desc(capi, model, **{**full, "ckpt": None})) == -1
        assert call(_desc(capi, model, **{**full, "traj_per_image": 16})) == -2       # IONODE_ERR_UNSUPPORTED
        d = _desc(capi, model, **full)
        assert lib.ionode_dopri5_backward_sse(C.byref(d), 3, 2, 4, ptr, ptr, None, None, ptr, ptr, ptr, ptr, ptr, ptr, None) == -1
    for model in (capi.MODEL_NNF, capi.MODEL_NND):
        assert call(_desc(capi, model, ckpt=buf.ctypes.data, ckpt_cap=4, sse_ref=buf.ctypes.data)) == -2
    assert "closed-form" in lib.ionode_grad_last_error().decode()


def test_sum_of_squares_rejects_nn_models_and_cpu_tensors(ion):
    with pytest.raises(ion.IonodeError, match="closed-form"):
        ion.grad.sum_of_squares(ion.capi.MODEL_NNF, torch.zeros((1, 8), dtype=torch.float64), torch.zeros((1, 10)),
                                torch.zeros((1, 2)), torch.arange(10.0), torch.zeros((1, 10)))
    with pytest.raises(ion.IonodeError, match="no HIP tensors"):
        ion.grad.sum_of_squares(ion.capi.MODEL_HH2, torch.zeros((1, 8), dtype=torch.float64), torch.zeros((1, 10)),
                                torch.zeros((1, 2)), torch.arange(10.0), torch.zeros((1, 10)), max_step=1.0)


# ---- gloo world size 2: population_sum_of_squares_s1 with a stand-in solver ----

FREE = (0, 1, 2, 3)


def _population():
    rng = np.random.default_rng(11)
    C = 7   # odd: uneven shards
    cand = K.P_HH[None, :4] * rng.uniform(0.8, 1.25, (C, 4))
    cand[6] *= 3.0          # the fastest gate sits in rank 1's shard: a per-shard cap would differ on rank 0
    cand[3, 1] = np.nan     # a failing candidate
    pv = np.stack([K.activation(v)[1][:200] for v in (-40, 0, 40)])
    te = np.arange(50, dtype=np.float64)
    data = rng.normal(0, 1.0, (3, te.size))
    return cand, pv, te, data


class StandIn:
    """Differentiable stand-in with grad.sum_of_squares' signature: sse_b = sum_k (p_b . phi_k(protocol) - data)^2, status 2 where
    the parameters are not finite.  Records the step cap it was called with."""

    def __init__(self):
        self.caps = []

    def __call__(self, model, params, prot_v, y0, t_eval, sse_ref, *, prot_t0, prot_dt, prot_of_traj, obs_g, obs_e,
                 obs_open_state_only, max_total_steps, max_step):
        self.caps.append(float(max_step))
        pot = prot_of_traj.long()
        phi = torch.stack([torch.cos(0.01 * (i + 1) * t_eval) for i in range(params.shape[1])], 1)    # [Nt, npar]
        pred = (params[:, None, :] * phi[None] * prot_v[pot, :1, None].abs()).sum(-1) * 1e-3 + y0[:, :1].double()
        val = ((pred - sse_ref[pot]) ** 2).sum(1)
        ok = torch.isfinite(params).all(1)
        return torch.where(ok, val, torch.full_like(val, float("inf"))), torch.where(ok, 0, 2).to(torch.int32)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _run(ion):
    cand, pv, te, data = _population()
    solver = StandIn()
    sse, g = ion.objective.population_sum_of_squares_s1(cand, pv, data, te, base_params=K.P_HH, free=FREE, solver=solver,
                                                        state_dtype=torch.float64)
    return sse.numpy(), g.numpy(), solver.caps


def _worker(rank, world, port, q):
    for p in (ROOT, os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port))
    ion = importlib.import_module("neural-ode-ion-channels_amd")
    importlib.import_module("neural-ode-ion-channels_amd.objective")
    d = ion.distributed.init_process_group()
    assert d.get_backend() == "gloo" and d.get_world_size() == world
    q.put((rank, _run(ion)))
    d.barrier()
    d.destroy_process_group()


@pytest.mark.timeout(300)
def test_two_rank_s1_objective_equals_single_process(ion):
    importlib.import_module("neural-ode-ion-channels_amd.objective")
    want_sse, want_g, want_caps = _run(ion)
    cand, pv, _, _ = _population()
    # the auto cap: grad.stable_step_cap over the whole (finite) population, not over a shard
    params = np.tile(K.P_HH, (cand.shape[0], 1))
    params[:, list(FREE)] = cand
    fin = np.isfinite(params).all(1)
    cap = ion.grad.stable_step_cap(ion.capi.MODEL_HH2, torch.from_numpy(params[fin]), torch.from_numpy(pv))
    shard0 = ion.grad.stable_step_cap(ion.capi.MODEL_HH2, torch.from_numpy(params[:4][fin[:4]]), torch.from_numpy(pv))
    assert cap > 0 and shard0 != cap and want_caps == [cap]
    assert np.isinf(want_sse[3]) and np.all(want_g[3] == 0) and np.isfinite(np.delete(want_sse, 3)).all()
    assert np.all(np.delete(want_g, 3, axis=0) != 0)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = dict(q.get(timeout=240) for _ in range(2))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for r in (0, 1):
        sse, g, caps = got[r]
        assert np.array_equal(sse, want_sse) and np.array_equal(g, want_g)
        assert caps == [cap]
