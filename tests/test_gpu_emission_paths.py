"""-m gpu: the observation current through every forward emission path, in one place.

The dense-output evaluation and the observation model are defined once (csrc/ionode_interp.hpp) and called from four emission loops
of the solve kernel -- the cooperative scan, the owner loop, the work-list passes of the lane-wise kernels, the MLP tiles' batched
emission -- and from the deferred expansion.  Each case below runs a solve with the fused current on and a non-default conductance /
reversal potential (so the g != 1 branch runs), in both state dtypes, and compares bit for bit: states against oracle.solve, currents
against oracle.current over oracle.protocol_v.  Shapes are the smallest that reach the path.

What the cases reach: "scan" the cooperative scan; "owner-loaded-times" the owner loop (lane-wise kernels) and the tiles' batched
emission with output times loaded from t_eval; "uniform-exact-grid" (states stored, current on, 70 trajectories on one protocol, so
the closed-form models run their table variant) the work-list passes with the current for the 6-state model, the owner loop with
arithmetic times and the table's voltages for the 2-state model -- its work-list current needs a solve that stores no states, which
this file does not run -- and the tiles' emission / deferred expansion for NN-f."""
import numpy as np
import pytest

import kat_cases as K
from gpu_util import run_gpu

pytestmark = pytest.mark.gpu

G_OBS, E_OBS = 0.133898199260611944 * 1.2, float(np.float32(-88.4 - 5))  # train-r1.py:43-47
PROT = dict(prot_t0=0.0, prot_dt=1.0)
M6_Y0 = [0, 1.0, 0, 0, 0, 0]


def _irregular():
    te = np.sort(np.random.default_rng(1).uniform(0, 2999, 400))
    te[0] = 0.0
    return te


UNIFORM_DT = 5.0
UNIFORM = np.arange(601) * UNIFORM_DT


def _batch(p, B, spread):
    return p[None, :] * np.random.default_rng(B).uniform(1.0 - spread, 1.0 + spread, (B, p.shape[0]))


# name -> (model, params, y0, open_state_only, weights name, output samples of the grid it takes (None: all), extra run_gpu arguments)
MODELS = {
    "hh2-tpw16": (K.MODEL_HH2, _batch(K.P_HH, 70, 0.2), [0.0, 1.0], False, None, None, dict(tile_waves=16)),
    "hh2-tpw64": (K.MODEL_HH2, _batch(K.P_HH, 70, 0.2), [0.0, 1.0], False, None, None, dict(tile_waves=64)),
    "m6-tpw64": (K.MODEL_MARKOV6, _batch(K.P_M6, 70, 0.1), M6_Y0, True, None, None, dict(tile_waves=64)),
    "nnf-b5": (K.MODEL_NNF, np.tile(K.P_HH, (5, 1)), K.NN_Y0, False, "s1", 301, {}),      # small tile
    "nnf-b18": (K.MODEL_NNF, _batch(K.P_HH, 18, 0.1), K.NN_Y0, False, "s1", None, {}),    # 16-tile plus a ragged one
    "hh2": (K.MODEL_HH2, _batch(K.P_HH, 70, 0.2), [0.0, 1.0], False, None, None, {}),
    "m6": (K.MODEL_MARKOV6, _batch(K.P_M6, 70, 0.1), M6_Y0, True, None, None, {}),
}
IRREGULAR_MODELS = ["hh2-tpw16", "hh2-tpw64", "m6-tpw64", "nnf-b5", "nnf-b18"]
# path -> (output grid, run_gpu's grid arguments as a function of the grid, models)
PATHS = {
    "scan": (_irregular(), lambda te: dict(t_eval_hint=None), IRREGULAR_MODELS),
    # the hint "auto" is given only for a grid whose every time lies within half a spacing of its place; this one does not qualify, the
    # library passes no hint and these cases run the very path of "scan" again ...
    "auto-hint": (_irregular(), lambda te: dict(t_eval_hint="auto"), IRREGULAR_MODELS),
    # ... and the end points' spacing given outright is a guess the kernel verifies and walks from: the owner loop with loaded output times
    "owner-loaded-times": (_irregular(), lambda te: dict(t_eval_hint=(0.0, float(te[-1]) / (len(te) - 1))), IRREGULAR_MODELS),
    "uniform-exact-grid": (UNIFORM, lambda te: dict(t_eval_hint=(0.0, UNIFORM_DT), t_eval_exact=True), ["hh2", "m6", "nnf-b18"]),
}
CASES = [(path, m) for path, (_, _, models) in PATHS.items() for m in models]

_want = {}   # (grid, model parameters, dtype) -> the oracle's states and currents: computed once, shared by the paths, never written to


def _oracle(oracle, path, name, f32):
    model, params, y0, open_only, wname, nt, _ = MODELS[name]
    te = PATHS[path][0][:nt]
    key = (te.tobytes(), model, params.tobytes(), f32)
    if key not in _want:
        pv = K.activation(20)[1]
        kw = dict(PROT)
        if wname:
            kw.update(weights=K.load_weights(wname), mlp_layers=5, mlp_width=200, nthreads=min(len(params), 16))
        o = oracle.solve(model, params, pv, y0, te, state_f32=f32, **kw)
        v, _ = oracle.protocol_v(pv, te, **PROT)
        i = oracle.current(o["y"], v, g=G_OBS, e_rev=E_OBS, open_state_only=open_only, state_f32=f32)
        for a in (o["y"], i):
            a.setflags(write=False)
        _want[key] = (o, i)
    return _want[key]


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("path,name", CASES, ids=[f"{p}-{m}" for p, m in CASES])
def test_current_on_every_emission_path(ion, gpu, oracle, path, name, f32):
    model, params, y0, open_only, wname, nt, extra = MODELS[name]
    te_full, grid_kw, _ = PATHS[path]
    te = te_full[:nt]
    kw = dict(PROT, current=True, obs_g=G_OBS, obs_e=E_OBS, obs_open_state_only=open_only, **grid_kw(te), **extra)
    if wname:
        kw.update(weights=K.load_weights(wname), L=5, N=200)
    g = run_gpu(ion, gpu, model, params, K.activation(20)[1], y0, te, f32=f32, **kw)
    o, want_i = _oracle(oracle, path, name, f32)
    assert (g["status"] == 0).all() and np.array_equal(g["status"], o["status"])
    assert np.array_equal(g["y"], o["y"])
    assert np.array_equal(g["i"], want_i)
