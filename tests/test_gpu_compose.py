"""-m gpu: the shrink-aware tile composition of the lean N = 200 16-tile (csrc/ionode_compose.hpp, capi.dopri5(cost_hint=...)).
The composition only decides which trajectories share a tile: the device kernel's order equals the host mirror's, and every output
is bit for bit that of launch_order=None (and the oracle's), wherever the cost comes from -- explicit costs, the pilot, the stats of
an earlier call, a stats tensor full of garbage -- with the current trace, the deferred dense output and the solve kernel's tail on.
Inputs: test_gpu_tile_shrink.py's heterogeneous tiles (short protocols, per-trajectory parameters), forced onto the 16-tile."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import kat_cases as K  # noqa: E402
import test_gpu_tile_shrink as TS  # noqa: E402

pytestmark = pytest.mark.gpu

KERNEL = ", 4, 4, 13, 13, 8>"
KEYS = ("y", "i", "status", "stats")
# (name, model, f32, B): one tile, a ragged last tile of 8, four tiles; both state dtypes; one NN-d case
CASES = [
    ("nnf_f64_16", K.MODEL_NNF, False, 16),
    ("nnf_f64_40", K.MODEL_NNF, False, 40),
    ("nnf_f64_64", K.MODEL_NNF, False, 64),
    ("nnf_f32_40", K.MODEL_NNF, True, 40),
    ("nnd_f64_40", K.MODEL_NND, False, 40),
]


class _Case:
    """Device-resident inputs of one case and its launch_order=None solve, made once."""

    def __init__(self, ion, dev, case):
        import torch
        _, self.model, self.f32, self.B = case
        self.capi, self.dev = ion.capi, dev
        w, params, pv, y0, te, kw = TS._inputs(self.model, self.f32, self.B, None, 0)
        self.host = dict(w=w, params=params, pv=pv, y0=y0, te=te, pot=kw["prot_of_traj"])
        sdt = torch.float32 if self.f32 else torch.float64
        self.args = (self.model, torch.from_numpy(params).to(dev), torch.from_numpy(pv).to(dev),
                     torch.from_numpy(y0).to(dev).to(sdt).contiguous(), torch.from_numpy(te).to(dev))
        self.kw = dict(mlp_packed=torch.from_numpy(self.capi.mlp_pack(w, 5, 200)).to(dev), mlp_layers=5, mlp_width=200, prot_t0=0.0,
                       prot_dt=1.0, prot_of_traj=torch.from_numpy(kw["prot_of_traj"]).to(dev), current=True, tile_waves=4)
        self.base = self.numpy(self.solve(launch_order=None))

    def solve(self, **kw):
        import torch
        r = self.capi.dopri5(*self.args, **self.kw, **kw)
        torch.cuda.synchronize()
        assert KERNEL in r["kernel"], r["kernel"]
        return r

    @staticmethod
    def numpy(r):
        return {k: r[k].double().cpu().numpy() if k == "y" else r[k].cpu().numpy() for k in KEYS}

    def check(self, r, source, cost=None):
        """r was composed from `source`; its order is a permutation (the host mirror's for a known cost); its outputs are the base's."""
        assert r["composed"] == source, (r["composed"], source)
        order = r["launch_order"].cpu().numpy()
        assert order.dtype == np.int32 and np.array_equal(np.sort(order), np.arange(self.B))
        if cost is not None:
            assert np.array_equal(order, self.capi.compose_order_host(cost))
        g = self.numpy(r)
        for k in KEYS:
            assert np.array_equal(g[k], self.base[k], equal_nan=True), (source, k)


_CASES = {}


def _case(ion, dev, case):
    if case[0] not in _CASES:
        _CASES[case[0]] = _Case(ion, dev, case)
    return _CASES[case[0]]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_composed_launch_is_bit_identical(ion, gpu, oracle, case):
    import torch
    c = _case(ion, gpu, case)
    capi, B = c.capi, c.B
    assert (c.base["status"] == 0).all() and len(np.unique(c.base["stats"][:, 2])) > B // 2   # heterogeneous tiles
    h = c.host
    o = oracle.solve(c.model, h["params"], h["pv"], h["y0"], h["te"], weights=h["w"], mlp_layers=5, mlp_width=200, state_f32=c.f32,
                     nthreads=4, prot_t0=0.0, prot_dt=1.0, prot_of_traj=h["pot"])
    assert np.array_equal(c.base["stats"], o["stats"]) and np.array_equal(c.base["y"], o["y"], equal_nan=True)
    # the plans: this launch qualifies, defers its dense output, and (from two tiles on) expands early tiles in the solve kernel
    r0 = c.solve(cost_hint=None)
    assert r0["composed"] is None and r0["launch_order"] is None
    assert capi.compose_plan(r0["desc"], True) == {"compose": True, "source": "auto"}
    assert capi.dense_defer_plan(r0["desc"], True)["capacity"] > 0
    assert capi.dense_tail_plan(r0["desc"], True)["tail_rank"] == (B + 15) // 16 * 5 // 8
    # explicit costs: the solve's own RHS evaluations, fp64
    nfe = c.base["stats"][:, 2].astype(np.float64)
    r = c.solve(cost_hint=torch.from_numpy(nfe).to(gpu))
    c.check(r, "explicit", nfe)
    tiles = (B + 15) // 16
    assert 0 <= capi.compose_tail_plan(r["desc"], True, r["composed"])["tail_rank"] <= tiles
    assert B <= 16 or not np.array_equal(r["launch_order"].cpu().numpy(), np.arange(B))   # a real re-composition
    # the pilot
    c.check(c.solve(cost_hint="pilot"), "pilot")
    # a reused `out`: the earlier call's stats are the cost, read in place ahead of the solve that overwrites them
    out = {k: r[k] for k in KEYS}
    c.check(c.solve(cost_hint="hint", out=out), "hint", nfe)
    assert out["stats"].data_ptr() == r["stats"].data_ptr()
    # ... and a stats tensor filled with garbage
    rng = np.random.default_rng(77 + B)
    junk = rng.integers(-2**62, 2**62, (B, 4), dtype=np.int64)
    junk[rng.integers(0, B, 5), 2] = 3   # ties
    c.check(c.solve(cost_hint="hint", out={"stats": torch.from_numpy(junk.copy()).to(gpu)}), "hint", junk[:, 2].astype(np.float64))
    # "auto" leaves a forced tile shape alone
    assert c.solve()["composed"] is None


@pytest.mark.parametrize("B", [1, 16, 17, 40, 64, 4096, 8192])
def test_device_order_equals_the_host_mirror(ion, gpu, B):
    import torch
    capi = ion.capi
    rng = np.random.default_rng(B)
    cost = rng.uniform(0, 1e4, B)
    cost[rng.integers(0, B, max(1, B // 8))] = np.nan
    cost[rng.integers(0, B, max(1, B // 8))] = -1.0
    cost[rng.integers(0, B, max(1, B // 8))] = np.inf
    cost[rng.integers(0, B, max(1, B // 4))] = 5.0   # ties
    got = capi.compose_order(torch.from_numpy(cost).to(gpu)).cpu().numpy()
    assert np.array_equal(got, capi.compose_order_host(cost))
    # a stats tensor's column, read in place (int64, stride 4)
    stats = rng.integers(0, 30000, (B, 4), dtype=np.int64)
    st = torch.from_numpy(stats).to(gpu)
    got = capi.compose_order(st[:, 2]).cpu().numpy()
    assert np.array_equal(got, capi.compose_order_host(stats[:, 2].astype(np.float64)))
    # equal costs: index order
    assert np.array_equal(capi.compose_order(torch.full((B,), 3.0, dtype=torch.float64, device=gpu)).cpu().numpy(), np.arange(B))


def test_planner_says_no(ion, gpu, monkeypatch):
    import torch
    capi = ion.capi
    cus = torch.cuda.get_device_properties(gpu).multi_processor_count

    def desc(**kw):
        d = dict(model=capi.MODEL_NNF, state_f32=0, n_state=2, n_out=2001, n_traj=40, n_prot=3, prot_n=2001, mlp_layers=5, mlp_width=200,
                 n_params=8, prot_t0=0.0, prot_dt=1.0, v_oob=-80.0, rtol=1e-7, atol=1e-9, obs_g=1.0, obs_e=-86.0, tile_waves=4,
                 t_eval_t0_hint=0.0, t_eval_dt_hint=1.0, t_eval_exact=1)
        d.update(kw)
        return capi.make_desc(**d)

    yes = lambda **kw: capi.compose_plan(desc(**kw), True)["compose"]
    assert yes() and yes(model=capi.MODEL_NND, state_f32=1)
    assert yes(n_traj=16 * cus) and not yes(n_traj=16 * cus + 1)                    # more tiles than compute units
    assert yes(n_traj=1025, tile_waves=0) and not yes(n_traj=1024, tile_waves=0)    # 1024 trajectories: the 4-trajectory tile's kernel
    assert not yes(traj_per_image=16, mlp_image_stride=int(capi.lib().ionode_mlp_packed_floats(5, 200)))
    own = torch.arange(40, dtype=torch.int32, device=gpu)
    assert not yes(launch_order=own.data_ptr())                                     # a caller's own order
    assert not yes(t_eval_exact=0) and not yes(mlp_width=100)                       # not the lean N = 200 tile
    for sw, want in (("0", (False, "off")), ("pilot", (True, "pilot")), ("hint", (True, "hint")), ("", (True, "auto"))):
        monkeypatch.setenv("IONODE_COMPOSE", sw)                                    # read per plan
        p = capi.compose_plan(desc(), True)
        assert (p["compose"], p["source"]) == want, (sw, p)
    monkeypatch.setenv("IONODE_TILE_SHRINK", "0")
    assert not yes()
