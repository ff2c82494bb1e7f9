"""-m gpu: the rate paths of csrc/ionode_rhs.hpp OUTSIDE the physical range, every kernel family against the oracle bit for bit.

tests/rate_edge_cases.py pushes single exponents to where exp() returns subnormals, zero, inf or NaN.  The oracle integrates some of
those rows to status 0 and fails others -- at once, or late -- and every kernel must return its status, step counters, states (NaN
patterns included) and current trace.  Each case names the kernel it must have run on, so the list reaches every exp variant of
rhs() and closed_rates(): det_exp_inrange / det_exp_ldexp on both sides of the wave-uniform ballot (closed-form kernels and the
N <= 16 one-trajectory-per-lane net, with physical rows in a wavefront of their own), det_exp_s (the 16- and 32-trajectory tiles,
the run-time-width net, N = 100, N = 500) and det_exp_ldexp (one- and 4-trajectory tiles, the shrink net, the deep stack)."""
import numpy as np
import pytest

import kat_cases as K
import rate_edge_cases as R
from gpu_util import run_gpu

pytestmark = pytest.mark.gpu

OBS = dict(obs_g=0.7, obs_e=-86.0)
_solved = {}


def _oracle(oracle, model, f32, net, picks):
    key = (model, f32, net, tuple(picks))
    if key not in _solved:        # cases that differ in the tile only share a solve; nobody writes into it
        _solved[key] = R.oracle_solve(oracle, model, f32, net, picks)
    return _solved[key]


def _gpu(ion, gpu, model, f32, net, params, pot, y0, tile_waves, **kw):
    w = R.weights(net)
    mlp = dict(weights=w["weights"], L=w["mlp_layers"], N=w["mlp_width"]) if w else {}
    g = run_gpu(ion, gpu, model, params, R.protocols(), y0, R.T_EVAL, f32=f32, prot_t0=0.0, prot_dt=1.0, prot_of_traj=pot,
                tile_waves=tile_waves, launch_order=None, **mlp, **kw)
    g["kernel"] = ion.capi.lib().ionode_last_kernel_name().decode()
    return g


def _same(g, o):
    assert np.array_equal(g["status"], o["status"]), (g["status"], o["status"])
    assert np.array_equal(g["stats"], o["stats"]), np.nonzero((g["stats"] != o["stats"]).any(axis=1))[0]
    assert np.array_equal(g["y"], o["y"], equal_nan=True), np.nonzero([not np.array_equal(a, b, equal_nan=True) for a, b in zip(g["y"], o["y"])])[0]


@pytest.mark.parametrize("case", R.GPU_CASES, ids=[c[0] for c in R.GPU_CASES])
def test_out_of_range_rates_match_the_oracle(ion, gpu, oracle, case):
    name, model, f32, net, picks, tile_waves, frag, frag_lean, at_once = case
    params, pot, oor, row, y0, o = _oracle(oracle, model, f32, net, picks)
    R.not_vacuous(o["status"], o["stats"], oor, row, at_once=at_once)
    open_only = model == K.MODEL_MARKOV6

    g = _gpu(ion, gpu, model, f32, net, params, pot, y0, tile_waves, current=True, obs_open_state_only=open_only, **OBS)
    assert frag in g["kernel"], g["kernel"]
    _same(g, o)
    # the fused current trace: g * gate * (V - E) from the oracle's states and protocol lookup, on the rows that integrate
    pv = R.protocols()
    ok = np.nonzero(o["status"] == 0)[0]
    for b in ok:
        v, _ = oracle.protocol_v(pv[pot[b]], R.T_EVAL, prot_t0=0.0, prot_dt=1.0)
        want = oracle.current(o["y"][b], v, g=OBS["obs_g"], e_rev=OBS["obs_e"], state_f32=f32, open_state_only=open_only)
        assert np.array_equal(g["i"][b], want), b
    if frag_lean is not None:     # the lane-wise kernels' lean variant (states only) is a kernel of its own
        gl = _gpu(ion, gpu, model, f32, net, params, pot, y0, tile_waves)
        assert frag_lean in gl["kernel"], gl["kernel"]
        _same(gl, o)

    # path independence: the rows whose arguments are all in range and that integrate, solved alone -- a batch in which every wavefront
    # takes det_exp_inrange and no trajectory fails -- return the bits they had beside out-of-range and failing rows
    alone = np.nonzero(~oor & (o["status"] == 0))[0]
    assert alone.size >= 2 and not R.out_of_range(model, params[alone], pv[pot[alone]]).any()
    ga = _gpu(ion, gpu, model, f32, net, params[alone], pot[alone], y0, tile_waves, current=True, obs_open_state_only=open_only, **OBS)
    assert frag in ga["kernel"], ga["kernel"]
    assert (ga["status"] == 0).all() and np.array_equal(ga["stats"], g["stats"][alone])
    assert np.array_equal(ga["y"], g["y"][alone]) and np.array_equal(ga["i"], g["i"][alone])
