"""CPU tests of the NN models' fused sum-of-squares gradient, host side: the three C entry points exist and check their arguments
before any launch, and grad.sum_of_squares routes the models and their weights as documented."""
import ctypes as C

import numpy as np
import pytest
import torch

ARG, UNSUPPORTED = -1, -2   # IONODE_ERR_ARG, IONODE_ERR_UNSUPPORTED


def _desc(capi, model, **kw):
    m6 = model == capi.MODEL_MARKOV6
    base = dict(model=model, n_state=6 if m6 else 2, n_out=10, n_traj=20, n_prot=1, prot_n=10, n_params=12 if m6 else 8,
                prot_dt=1.0, rtol=1e-7, atol=1e-9, obs_g=1.0, obs_e=-86.0)
    if model in (capi.MODEL_NNF, capi.MODEL_NND):
        base.update(mlp_layers=1, mlp_width=10)
    base.update(kw)
    return capi.make_desc(**base)


def test_entry_points_reject_bad_arguments_before_any_launch(ion):
    capi = ion.capi
    lib = capi.lib()
    assert capi.ABI_VERSION == 10 and lib.ionode_abi_version() == 10   # additions only
    for name in ("ionode_dopri5_backward_sse_gc", "ionode_dopri5_backward_recompute_sse", "ionode_dopri5_backward_sweep_sse"):
        assert name in capi.EXPORTS and getattr(lib, name)
    buf = np.zeros(4096, dtype=np.float64)   # stand-in addresses: every call below returns before anything is dereferenced
    ptr = C.c_void_p(buf.ctypes.data)
    full = dict(ckpt=buf.ctypes.data, ckpt_cap=4, sse_ref=buf.ctypes.data)

    def gc(d, rng=(0, 1, 1), grad_sse=ptr, packets=ptr, s0=ptr):
        return lib.ionode_dopri5_backward_sse_gc(C.byref(d), *rng, ptr, None, None, ptr, ptr, grad_sse, packets, s0, None)

    def recompute(d, rng=(0, 1, 1), packets=ptr):
        return lib.ionode_dopri5_backward_recompute_sse(C.byref(d), *rng, ptr, ptr, ptr, None, None, ptr, ptr, None, packets, None)

    def sweep(d, rng=(0, 1, 1), s0=ptr):
        return lib.ionode_dopri5_backward_sweep_sse(C.byref(d), *rng, ptr, ptr, ptr, None, None, ptr, ptr, s0, ptr, None, ptr, ptr, ptr, None)

    for model in (capi.MODEL_NNF, capi.MODEL_NND):
        for call in (gc, recompute, sweep):
            assert call(_desc(capi, model, **{**full, "sse_ref": None})) == ARG
            assert call(_desc(capi, model, **{**full, "ckpt": None})) == ARG
            assert call(_desc(capi, model, **{**full, "ckpt_cap": 0})) == ARG
            for rng in ((3, 2, 4), (-1, 1, 1), (0, 2, 1), (1, 1, 1)):
                assert call(_desc(capi, model, **full), rng=rng) == ARG
            assert call(_desc(capi, model, **{**full, "traj_per_image": 16})) == UNSUPPORTED
            assert call(_desc(capi, model, **{**full, "mlp_width": 300})) == UNSUPPORTED      # a width the sweep does not serve
            assert call(_desc(capi, model, **{**full, "mlp_layers": 16})) == UNSUPPORTED      # more than 15 hidden layers
        assert gc(_desc(capi, model, **full), grad_sse=None) == ARG
        assert gc(_desc(capi, model, **full), packets=None) == ARG
        assert gc(_desc(capi, model, **full), s0=None) == ARG
        assert recompute(_desc(capi, model, **full), packets=None) == ARG
        assert sweep(_desc(capi, model, **full), s0=None) == ARG
    for model in (capi.MODEL_HH2, capi.MODEL_MARKOV6):
        for call in (gc, recompute, sweep):
            assert call(_desc(capi, model, **full)) == UNSUPPORTED
            assert "ionode_dopri5_backward_sse" in lib.ionode_grad_last_error().decode()   # names the entry point that serves them


def _args():
    return (torch.zeros((1, 8), dtype=torch.float64), torch.zeros((1, 10)), torch.zeros((1, 2)), torch.arange(10.0), torch.zeros((1, 10)))


def test_sum_of_squares_routes_models_and_weights(ion):
    capi = ion.capi
    w = torch.zeros(2 * 10 + 10 + 2 * (10 * 10 + 10) + 10 + 1)
    # an NN model with weights goes on to the device check (before the feature: "closed-form models only")
    with pytest.raises(ion.IonodeError, match="no HIP tensors"):
        ion.grad.sum_of_squares(capi.MODEL_NNF, *_args(), weights_flat=w, mlp_layers=2, mlp_width=10)
    with pytest.raises(ion.IonodeError, match="closed-form"):
        ion.grad.sum_of_squares(capi.MODEL_NND, *_args())
    for model in (capi.MODEL_HH2, capi.MODEL_MARKOV6):
        with pytest.raises(ion.IonodeError, match="no MLP"):
            ion.grad.sum_of_squares(model, *_args(), weights_flat=w, mlp_layers=2, mlp_width=10)
    # two-phase only: the refusal names the alternative
    with pytest.raises(ion.IonodeError, match="grad.solve"):
        ion.grad.sum_of_squares(capi.MODEL_NNF, *_args(), weights_flat=w, mlp_layers=2, mlp_width=10, two_phase=False)


def test_one_phase_environment_is_refused(ion, monkeypatch):
    monkeypatch.setenv("IONODE_GRAD_ONE_PHASE", "1")
    w = torch.zeros(2 * 10 + 10 + 2 * (10 * 10 + 10) + 10 + 1)
    with pytest.raises(ion.IonodeError, match="grad.solve"):
        ion.grad.sum_of_squares(ion.capi.MODEL_NNF, *_args(), weights_flat=w, mlp_layers=2, mlp_width=10)
