"""The cases of the posterior predictive bands, shared by tests/test_predictive_host.py (CPU: the host mirrors) and
tests/test_gpu_predictive.py (-m gpu: the kernels against the mirrors, bit for bit): seeded synthetic traces with failed rows and awkward
values, their numpy references, and the sequence "accumulate in chunks, then the quantiles" on either device.
"""
import importlib
from types import SimpleNamespace

import numpy as np
import torch

import cmaes_cases as L

U = 2.0 ** -53
Q = (0.0, 0.025, 0.5, 0.975, 1.0)
# draws -> slots of the column store: never a power of two (a store may be larger than what is accumulated; unwritten slots sort last)
S_CAP = {1: 3, 2: 3, 5: 5, 33: 33, 100: 100}
SHAPES = [(S, Nt, P) for S in (1, 2, 5, 33, 100) for Nt in (1, 37, 130) for P in (1, 3)]
TAG_ATTEMPT = 0x7072   # capi.PREDICTIVE_TAG / 65536: the generator's fourth word in cmaes_cases.draw_words' terms


def mods():
    ion = importlib.import_module("neural-ode-ion-channels_amd")
    return ion.capi, importlib.import_module("neural-ode-ion-channels_amd.predictive")


def failures(S, Nt, P):
    """bool [S, P]: which rows fail.  Three patterns: "edges" -- the first, a middle and the last draw (what S allows: S = 2 the first
    only, S = 1 none); "all"; "one" -- every draw but S // 2.  Protocol p carries pattern p % 3; P = 1 takes one, by Nt."""
    edges, everything, one = np.zeros(S, bool), np.ones(S, bool), np.ones(S, bool)
    if S >= 5:
        edges[[0, S // 2, S - 1]] = True
    elif S >= 2:
        edges[0] = True
    one[S // 2] = False
    pats = [edges, everything, one]
    if P == 1:
        return pats[{1: 1, 37: 2}.get(Nt, 0)][:, None]
    return np.stack([pats[p % 3] for p in range(P)], axis=1)


def make(S, Nt, P, seed=None):
    """A case: trace [S * P, Nt] fp64 (row = draw * P + protocol) of N(1, 1) values with +0.0, -0.0, repeated values and denormals
    planted, status int32 [S * P] (2 where failures() says so), and per-draw noise levels."""
    # (k % 2 alternates within k % 3 == 1: k = 1, 7, 13 .. odd -> 5e-324; k = 4, 10 .. even -> -3e-310)
    rng = np.random.default_rng(1000 * S + 10 * Nt + P if seed is None else seed)
    x = 1.0 + rng.normal(size=(S, P, Nt))
    fail = failures(S, Nt, P)
    # The awkward values, by column: k % 3 == 0 takes +0.0 / -0.0 in pairs of draws at random places, k % 3 == 2 the repeated value
    # 0.75 likewise, and k % 3 == 1 ONE denormal (5e-324 or -3e-310, by k) at a surviving draw.  One, because the issue's bounds are
    # relative ones -- u times a magnitude -- and hold where no result underflows: between two denormal neighbours (or a zero and a
    # denormal) an interpolated quantile is rounded to a multiple of 5e-324, far above u times its size.
    for k in range(Nt):
        if k % 3 == 1:
            for p in range(P):
                s = S // 2 if not fail[S // 2, p] else (S // 2 + 1) % S
                x[s, p, k] = 5e-324 if k % 2 else -3e-310
            continue
        n = max(1, (S * P) // 6)
        s, p = rng.integers(0, S, n), rng.integers(0, P, n)
        x[s, p, k], x[(s + 1) % S, p, k] = (0.0, -0.0) if k % 3 == 0 else (0.75, 0.75)
    # what a failed solve leaves in its trace is not the accumulation's business: make it loud
    x[fail] = np.where(rng.random((int(fail.sum()), Nt)) < 0.5, np.nan, 1e300)
    return SimpleNamespace(S=S, Nt=Nt, P=P, s_cap=S_CAP.get(S, S), trace=np.ascontiguousarray(x.reshape(S * P, Nt)),
                           status=np.where(fail, 2, 0).astype(np.int32).reshape(S * P), fail=fail,
                           sigma=np.ascontiguousarray(0.05 + 0.2 * rng.random(S)))


def run(case, device="cpu", chunk=None, noise=False, sigma=None, seed=0, q=Q, store=True, draw_offset=0):
    """Accumulate the case in chunks of `chunk` draws (None: all at once), then the quantiles.  Returns a dict of numpy arrays: mean, m2,
    min, max, count, cols, quant."""
    _, pr = mods()
    dev = torch.device(device)
    st = pr.new_state(case.P, case.Nt, case.s_cap, dev, store=store)
    sig = torch.from_numpy(sigma).to(dev) if isinstance(sigma, np.ndarray) else sigma
    step = case.S if chunk is None else chunk
    for lo in range(0, case.S, step):
        hi = min(case.S, lo + step)
        pr.accumulate(st, torch.from_numpy(case.trace[lo * case.P:hi * case.P]).to(dev), torch.from_numpy(case.status[lo * case.P:hi * case.P]).to(dev),
                      draw_base=lo, sigma=sig, noise=noise, seed=seed, draw_offset=draw_offset)
    out = {k: st[k].cpu().numpy() for k in ("mean", "m2", "min", "max", "count")}
    out["cols"] = st["cols"].cpu().numpy() if store else None
    out["quant"] = pr.quantile_pass(st, q).cpu().numpy() if store and q else None
    return out


def same_bits(a, b):
    """dict against dict, every array bit for bit (NaNs and the sign of zeros included)."""
    assert a.keys() == b.keys()
    for k in a:
        if (a[k] is None) != (b[k] is None):
            return False
        if a[k] is not None and not L.same_bits(a[k], b[k]):
            return False
    return True


def survivors(case, p, values=None):
    """[m, Nt]: protocol p's values of the draws that did not fail, in draw order."""
    x = (case.trace if values is None else values).reshape(case.S, case.P, case.Nt)
    return x[~case.fail[:, p], p]


def key_sort(x):
    """Sort along axis 0 in the kernels' total order (the sign-flip keys: -0 before +0), returning doubles."""
    b = np.ascontiguousarray(x).view(np.uint64)
    key = np.where(b >> np.uint64(63), ~b, b | np.uint64(1 << 63))
    key = np.sort(key, axis=0)
    back = np.where(key >> np.uint64(63), key & np.uint64((1 << 63) - 1), ~key)
    return back.view(np.float64)


def quantile_statement(xs, q):
    """The header's formula on sorted values xs [m, ...] in numpy fp64, operation for operation: (value, x_lo, x_hi)."""
    m = xs.shape[0]
    h = q * float(m - 1)
    lo = int(np.floor(h))
    g = h - np.floor(h)
    hi = min(lo + 1, m - 1)
    with np.errstate(invalid="ignore"):
        return xs[lo] + g * (xs[hi] - xs[lo]), xs[lo], xs[hi]


def normal(seed, draw, p, k):
    """The noise deviate of (seed, draw, p, k) from the numpy statement of the generator (tests/cmaes_cases.py)."""
    w = L.draw_words(seed, draw, p, k, 0, TAG_ATTEMPT)
    return L.ppnd16(L.uniform(w[0], w[1]))


def current_solver(oracle, calls=None):
    """The CPU oracle behind batched.solve's signature for current=True, states=False: cmaes_cases.oracle_solver's solve, returning the
    current traces .i [B, Nt] and .status instead of a fused sum."""
    def solver(model, params, prot_v, y0, t_eval, **kw):
        assert kw["current"] is True and kw["states"] is False and not kw["sse_ref"].any()
        p, te, pv, pot = params.numpy(), t_eval.numpy(), prot_v.numpy(), kw["prot_of_traj"].numpy()
        assert y0.shape[0] == p.shape[0] == pot.shape[0]
        if calls is not None:
            calls.append(p.shape[0])
        r = oracle.solve(model, p, pv, [0.0, 1.0], te, prot_t0=kw["prot_t0"], prot_dt=kw["prot_dt"], prot_of_traj=pot, state_f32=False,
                         rtol=kw["rtol"], atol=kw["atol"], max_step=kw["max_step"])
        volt = [oracle.protocol_v(pv[k], te, prot_t0=kw["prot_t0"], prot_dt=kw["prot_dt"])[0] for k in range(pv.shape[0])]
        i = np.stack([oracle.current(r["y"][b], volt[pot[b]], state_f32=False) for b in range(p.shape[0])])
        return SimpleNamespace(i=torch.from_numpy(i), status=torch.from_numpy(r["status"].astype(np.int32)))
    return solver
