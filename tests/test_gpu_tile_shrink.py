"""-m gpu, round 6: the lean N = 200 16-tile finishes its tiles on the 4-trajectory net once <= 4 of their trajectories are live
(MlpShrink4, ionode_mlp_tile4.hpp).  Only the net changes: every case returns the oracle's bits, and the same bits with the switch turned
off (IONODE_TILE_SHRINK=0, read per plan -- a fresh child process runs every case that way)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import kat_cases as K  # noqa: E402
from gpu_util import run_gpu  # noqa: E402

pytestmark = pytest.mark.gpu

# (name, model, f32, B, NaN y0 slot, max_total_steps): tiles of 16 with heterogeneous protocols and parameters, so that their
# trajectories stop at different attempts; B = 35 leaves a last tile of 3 valid slots (<= 4 from the start)
CASES = [
    ("nnf_f64", K.MODEL_NNF, False, 48, None, 0),
    ("nnf_f32", K.MODEL_NNF, True, 48, None, 0),
    ("nnd_f64", K.MODEL_NND, False, 48, None, 0),
    ("nnd_f32", K.MODEL_NND, True, 48, None, 0),
    ("ragged", K.MODEL_NNF, False, 35, None, 0),
    ("nan_and_cut", K.MODEL_NNF, False, 48, 5, 230),
]


def _inputs(model, f32, B, nan_slot, cut):
    rng = np.random.default_rng(600 + B + 7 * f32 + model)
    w = K.load_weights("d2" if model == K.MODEL_NND else "s1")
    base = K.P_NN_D if model == K.MODEL_NND else K.P_HH
    params = np.tile(base, (B, 1)) * rng.uniform(0.8, 1.2, (B, 8))
    pv = np.stack([K.activation(v)[1] for v in (-20, 20, 40)])
    te = K.activation(0)[2][:2001]
    pot = rng.integers(0, 3, B).astype(np.int32)
    y0 = np.tile(K.NN_Y0, (B, 1)).astype(np.float64)
    if nan_slot is not None:
        y0[nan_slot, 1] = np.nan   # a failing trajectory inside a tile
    kw = dict(prot_t0=0.0, prot_dt=1.0, prot_of_traj=pot)
    if cut:
        kw["max_total_steps"] = cut   # some trajectories of the same tiles run into the attempt bound
    return w, params, pv, y0, te, kw


def _run(ion, dev, case):
    _, model, f32, B, nan_slot, cut = case
    w, params, pv, y0, te, kw = _inputs(model, f32, B, nan_slot, cut)
    g = run_gpu(ion, dev, model, params, pv, y0, te, weights=w, L=5, N=200, f32=f32, current=True, tile_waves=4, **kw)
    g["kernel"] = ion.capi.lib().ionode_last_kernel_name().decode()
    return g


@pytest.fixture(scope="module")
def gate_off(tmp_path_factory, gpu):
    """Every case solved with the switch off, in a fresh child process (the override is read when a launch is planned)."""
    out = str(tmp_path_factory.mktemp("shrink_off") / "off.npz")
    env = dict(os.environ, IONODE_TILE_SHRINK="0")
    subprocess.run([sys.executable, os.path.abspath(__file__), out], env=env, check=True, timeout=900)
    return dict(np.load(out))


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_shrunk_tile_is_bit_identical(ion, gpu, oracle, gate_off, case):
    name, model, f32, B, nan_slot, cut = case
    w, params, pv, y0, te, kw = _inputs(model, f32, B, nan_slot, cut)
    o = oracle.solve(model, params, pv, y0, te, weights=w, mlp_layers=5, mlp_width=200, state_f32=f32, nthreads=4,
                     max_total_steps=cut, **{k: v for k, v in kw.items() if k != "max_total_steps"})
    g = _run(ion, gpu, case)
    assert ", 4, 4, 13, 13, 8>" in g["kernel"], g["kernel"]
    att = o["stats"][:, 0] + o["stats"][:, 1]
    assert len(np.unique(att)) > B // 2   # the tiles' trajectories stop at different attempts: their tails run shrunk
    if nan_slot is not None:
        assert (o["status"] != 0).sum() >= 2 and (o["status"] == 0).any(), o["status"]
    assert np.array_equal(g["status"], o["status"]) and np.array_equal(g["stats"], o["stats"])
    assert np.array_equal(g["y"], o["y"], equal_nan=True)
    for key in ("y", "i", "status", "stats"):
        assert np.array_equal(g[key], gate_off[f"{name}_{key}"], equal_nan=True), key


def test_shrunk_attempts_occur_in_the_stamps_build(ion, gpu):
    """The diagnostic build (-DIONODE_STAMPS) counts every tile's attempts on the 4-trajectory net in the step log
    (tools/tile_shrink_stamps.py): with the switch on, tiles finish on it; with it off, none does."""
    subprocess.run(["bash", os.path.join(ROOT, "tools", "build_variant.sh"), "shrink_stamps", "-DIONODE_STAMPS"], cwd=ROOT, check=True,
                   timeout=900, stdout=subprocess.DEVNULL)
    lib = os.path.join(ROOT, "neural-ode-ion-channels_amd", "variants", "shrink_stamps", "libionode.so")
    res = {}
    for gate in ("1", "0"):
        env = dict(os.environ, IONODE_LIB=lib, IONODE_TILE_SHRINK=gate)
        p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "tile_shrink_stamps.py"), "--batch", "512"],
                           env=env, check=True, timeout=600, capture_output=True, text=True)
        res[gate] = json.loads(p.stdout.strip().splitlines()[-1])
    on, off = res["1"], res["0"]
    assert ", 4, 4, 13, 13, 8>" in on["kernel"], on
    assert on["tiles_shrunk"] >= on["tiles"] // 2 and on["shrunk_attempts"]["sum"] > 0, on
    assert off["tiles_shrunk"] == 0 and off["shrunk_attempts"]["sum"] == 0, off


if __name__ == "__main__":   # child of the gate_off fixture: solve every case, save the outputs
    import importlib

    import torch
    _ion = importlib.import_module("neural-ode-ion-channels_amd")
    _dev = torch.device("cuda:0")
    _out = {}
    for _c in CASES:
        _g = _run(_ion, _dev, _c)
        assert ", 4, 4, 13, 13, 8>" in _g["kernel"], _g["kernel"]
        for _k in ("y", "i", "status", "stats"):
            _out[f"{_c[0]}_{_k}"] = _g[_k]
    np.savez(sys.argv[1], **_out)
