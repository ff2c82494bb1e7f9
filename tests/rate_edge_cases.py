"""Rate parameters and protocols OUTSIDE the physical range, shared by tests/test_rate_edge_cases.py (CPU, oracle only) and
tests/test_gpu_rate_edges.py (-m gpu).

Every other test draws rate parameters near P_HH / P_M6 and voltages in [-120, 60] mV, so every exponent argument p * v the
kernels have seen lies in about [-15, 15].  The rows below push single exponents to where exp() underflows into the subnormal
range (-720, -733.8), returns zero (-745.2, -765, -900, -8e301, -inf), overflows (+720 ... +inf) or is NaN -- on a protocol
and its negation, so that each row meets both signs.  What a row then DOES (integrates to status 0 with rates that are
subnormal or zero, fails at its second evaluation, fails late) is decided by the oracle, never written down here;
not_vacuous() states what a batch must contain for a comparison with it to mean something.
"""
import numpy as np

import kat_cases as K

N_SAMPLES = 600                       # protocol samples on a 1 ms grid, prot_t0 = 0
IN_RANGE = 708.0                      # |p * v| up to here takes the kernels' in-range exp (csrc/ionode_rhs.hpp)


def protocol_neg():
    v = np.full(N_SAMPLES, -80.0)
    v[100:250] = -100.0
    v[250:400] = -20.0
    v[400:500] = -103.5
    v[500:] = -60.0
    return v


def protocols():
    """[2, 600]: `neg` and its negation `pos`."""
    neg = protocol_neg()
    return np.stack([neg, -neg])


NEG, POS = 0, 1
T_EVAL = np.arange(0.0, 599.0, 2.0)   # 0, 2, .., 598: all four plateaus (the oracle takes about a second on it at N = 200 and N = 500)

# (index, value) changes of a physical row; indices are zero-based, the exponents are the odd ones
ROW_CHANGES = (
    (),                        # 0 physical
    ((5, 7.2),),               # 1
    ((1, 7.2),),               # 2
    ((5, 9.0),),               # 3
    ((7, 7.2),),               # 4
    ((3, 7.2),),               # 5
    ((5, 7.09),),              # 6
    ((4, np.nan),),            # 7
    ((5, 7.4),),               # 8
    ((5, 7.2), (1, 7.3)),      # 9
    (),                        # 10 physical
    (),                        # 11 physical
    ((4, 1e-310), (5, 7.09)),  # 12 a subnormal prefactor: the rate is moderate (8e-3 / ms at +100 mV, where exp() is 8e307) until the
                               #    +103.5 mV plateau overflows exp() -- a LATE failure in every model and state dtype (rows 4 and 5
                               #    fail late in some of them only: the 6-state model in fp32 state integrates both)
    # arguments far beyond the int range of exp's exponent k = rint(x / ln 2) -- and infinite ones: there the reduced argument is
    # garbage and only the range cases give 0 / inf.  Up to about |x| = 2^52 the in-range operation sequence itself still lands on
    # 0 or inf (ldexp saturates, both thresholds sit exactly where the scaling rounds to 0 / overflows), so rows 1 .. 9 alone cannot
    # tell det_exp_inrange from det_exp_ldexp, or a dropped select from a kept one
    ((5, 1e300),),             # 13 x = -/+ 8e301 and beyond
    ((7, 1e308),),             # 14 -p7 * v = +/- inf
)
# the order in which tiled() deals the rows out: the first 8 to 10 already hold every kind, for the cases with small batches
TILE_ORDER = (0, 13, 1, 14, 2, 3, 4, 5, 12, 6, 7, 8, 9, 10, 11)
N_ROWS = len(ROW_CHANGES)
PHYSICAL = (0, 10, 11)


def base_params(model):
    return K.P_M6 if model == K.MODEL_MARKOV6 else (K.P_NN_D if model == K.MODEL_NND else K.P_HH)


def exponent_indices(model):
    """The exponents the model's right-hand side reads (NN-f: p4 .. p7 only)."""
    if model == K.MODEL_MARKOV6:
        return (1, 3, 5, 7, 9, 11)
    return (5, 7) if model == K.MODEL_NNF else (1, 3, 5, 7)


def rows(model):
    """[N_ROWS, n_params]: the table's rows on the model's physical parameters."""
    p = np.tile(base_params(model), (N_ROWS, 1))
    for r, changes in enumerate(ROW_CHANGES):
        for i, val in changes:
            p[r, i] = val
    return p


def out_of_range(model, params, prot_v, v_oob=-80.0):
    """bool [B]: the row forms an exponent argument with |p * v| > 708 (or NaN) at some voltage of its protocol or at the hold
    voltage.  prot_v [B, Np]: each row's own protocol."""
    params = np.atleast_2d(params)
    idx = list(exponent_indices(model))
    vmax = np.maximum(np.abs(prot_v).max(axis=1), abs(v_oob))
    with np.errstate(over="ignore"):      # (an infinite argument is out of range)
        x = np.abs(params[:, idx]) * vmax[:, None]
    return ~(x <= IN_RANGE).all(axis=1)


def batch(model, picks):
    """picks: sequence of (row, protocol).  Returns (params [B, n_params], prot_of_traj int32 [B], out_of_range bool [B],
    row int [B])."""
    picks = list(picks)
    table = rows(model)
    r = np.array([p[0] for p in picks], dtype=np.int64)
    pot = np.array([p[1] for p in picks], dtype=np.int32)
    params = table[r].copy()
    oor = out_of_range(model, params, protocols()[pot])
    return params, pot, oor, r


def tiled(B, prots=(NEG, POS)):
    """The rows in TILE_ORDER, each on every protocol of `prots` before the next row (row 0 on neg, row 0 on pos, row 13 on neg, ...),
    repeated to B."""
    cycle = [(r, p) for r in TILE_ORDER for p in prots]
    return [cycle[i % len(cycle)] for i in range(B)]


def mixed_then_physical(n_mixed, n_physical):
    """For the one-trajectory-per-lane kernels: n_mixed rows that mix physical and out-of-range rows of both protocols (the first
    wavefronts), then physical rows only (a wavefront of its own when n_mixed is a multiple of the wavefront's trajectories) -- one
    launch takes both sides of the wave-uniform ballot."""
    return tiled(n_mixed) + [(PHYSICAL[i % 3], (NEG, POS)[i % 2]) for i in range(n_physical)]


# the lean N = 200 16-tile hands its region to the 4-trajectory net once <= 4 trajectories are live: 12 rows that (on NN-d) fail at their
# second evaluation around 4 that integrate, two of them with out-of-range arguments -- the hand-over happens at once
FAIL_AT_ONCE_12_OF_16 = [(1, POS), (2, POS), (0, NEG), (3, POS), (6, POS), (7, POS), (1, NEG), (8, POS), (9, POS), (4, NEG), (0, POS),
                         (5, NEG), (7, NEG), (13, NEG), (1, POS), (3, POS)]


def not_vacuous(status, stats, oor, row, at_once=False):
    """What a batch must contain (decided by the oracle's status and counters) so that comparing a kernel with it exercises the range
    cases: rates that underflow or vanish on trajectories that still integrate, immediate failures, a LATE failure (a tile that has
    carried the trajectory for a while), and untouched physical rows.  Returns the four counts; asserts the conditions.  at_once: the
    one batch built for another purpose (12 of 16 fail at their second evaluation, 4 integrate)."""
    status, nfe = np.asarray(status), np.asarray(stats)[:, 2]
    ok_oor = int(np.sum(oor & (status == 0)))
    failed = int(np.sum(status != 0))
    late = int(np.sum((status != 0) & (nfe > 100)))
    phys = np.isin(row, PHYSICAL)
    if at_once:     # FAIL_AT_ONCE_12_OF_16
        assert int(np.sum((status != 0) & (nfe == 2))) == 12 and int(np.sum(status == 0)) == 4 and ok_oor >= 2 and (status[phys] == 0).all()
        return ok_oor, failed, late, int(phys.sum())
    assert ok_oor >= 4, f"only {ok_oor} rows with an out-of-range argument end with status 0"
    assert failed >= 2, f"only {failed} rows fail"
    assert late >= 1, "no row fails after its 100th evaluation"
    assert phys.any() and (status[phys] == 0).all(), "a physical row failed"
    return ok_oor, failed, late, int(phys.sum())


# ---- the cases of tests/test_gpu_rate_edges.py; tests/test_rate_edge_cases.py checks not_vacuous() for each on the oracle alone ----
def weights(net):
    """net: None, ("golden", name, L, N) or ("random", seed, L, N) -- N(0, 0.1^2) as tests/test_gpu_edge.py draws them."""
    if net is None:
        return {}
    kind, key, L, N = net
    if kind == "golden":
        w = K.load_weights(key)
    else:
        w = np.random.default_rng(key).normal(0, 0.1, 2 * N + N + L * (N * N + N) + N + 1).astype(np.float32)
    return dict(weights=w, mlp_layers=L, mlp_width=N)


S1, S2 = ("golden", "s1", 5, 200), ("golden", "s2", 5, 200)
MIX64, MIX16 = mixed_then_physical(64, 6), mixed_then_physical(32, 16)   # B = 70 at 64 per wavefront; B = 48 at 16 per wavefront

# (id, model, fp32 state, net, picks, tile_waves, fragment of the kernel's name with current=True, fragment without, at_once)
GPU_CASES = []
for _m, _name in ((K.MODEL_HH2, "hh2"), (K.MODEL_MARKOV6, "m6")):
    for _f32 in (False, True):
        _s = "float" if _f32 else "double"
        GPU_CASES += [(f"{_name}-{_s}-64", _m, _f32, None, MIX64, 64, f"<{_m}, {_s}, 1, 0, 0, 0, ", f"<{_m}, {_s}, 1, 0, 0, 0, 1>", False),
                      (f"{_name}-{_s}-16", _m, _f32, None, MIX16, 16, f"<{_m}, {_s}, 1, 16, 0, 0, ", f"<{_m}, {_s}, 1, 16, 0, 0, 1>", False)]
for _m, _name in ((K.MODEL_NNF, "nnf"), (K.MODEL_NND, "nnd")):
    _n10 = ("random", 10, 5, 10)
    GPU_CASES += [
        # N <= 16: one trajectory per lane (the ballot between det_exp_inrange and det_exp_ldexp), and the 16-per-wavefront tile
        (f"{_name}-n10-lane64", _m, False, _n10, MIX64, 64, ", 1, 64, 1, 10, 0>", ", 1, 64, 1, 10, 1>", False),
        (f"{_name}-n10-lane64-float", _m, True, _n10, MIX64, 64, ", 1, 64, 1, 10, 0>", ", 1, 64, 1, 10, 1>", False),
        (f"{_name}-n10-tile", _m, False, _n10, tiled(18), 0, ", 1, 1, 1, 1, ", None, False),
    ]
GPU_CASES += [
    # the other widths: the N = 100 16-tile (det_exp_s), the run-time-width net, N = 500
    ("nnd-n100", K.MODEL_NND, False, ("random", 100, 2, 100), tiled(30), 0, ", 4, 4, 7, 7, ", None, False),
    ("nnf-n100-float", K.MODEL_NNF, True, ("random", 100, 2, 100), tiled(30), 0, ", 4, 4, 7, 7, ", None, False),
    ("nnd-n64-gen", K.MODEL_NND, False, ("random", 64, 2, 64), tiled(30), 0, ", 4, 1, 0, 1, ", None, False),
    ("nnd-n500", K.MODEL_NND, False, ("random", 500, 1, 500), tiled(17), 0, ", 4, 8, 32, 4, ", None, False),
    # N = 200: one trajectory, 4, 16 and 32 trajectories per tile
    ("nnd-n200-one", K.MODEL_NND, False, S2, tiled(30), 16, ", 4, 4, 13, 13, 40>", None, False),
    ("nnf-n200-one", K.MODEL_NNF, False, S1, tiled(30), 16, ", 4, 4, 13, 13, 40>", None, False),
    ("nnd-n200-four", K.MODEL_NND, False, S2, tiled(30), 2, ", 4, 4, 13, 13, 24>", None, False),
    ("nnd-n200-sixteen-at-once", K.MODEL_NND, False, S2, FAIL_AT_ONCE_12_OF_16, 4, ", 4, 4, 13, 13, 8>", None, True),
    ("nnd-n200-sixteen", K.MODEL_NND, False, S2, tiled(20), 4, ", 4, 4, 13, 13, 8>", None, False),
    ("nnd-n200-sixteen-float", K.MODEL_NND, True, S2, tiled(30), 4, ", 4, 4, 13, 13, 8>", None, False),
    ("nnf-n200-sixteen", K.MODEL_NNF, False, S1, tiled(30), 4, ", 4, 4, 13, 13, 8>", None, False),
    ("nnd-n200-thirtytwo", K.MODEL_NND, False, S2, tiled(40), 8, ", 4, 4, 13, 13, 12>", None, False),
    ("nnd-n200-deep", K.MODEL_NND, False, ("random", 210, 10, 200), tiled(30), 16, ", 4, 4, 13, 13, 104>", None, False),
]


def oracle_solve(oracle, model, f32, net, picks, nthreads=4):
    """The oracle on the rows `picks` (shared by the CPU and the GPU test).  Returns (params, prot_of_traj, oor, row, y0, result)."""
    params, pot, oor, row = batch(model, picks)
    y0 = [0.0, 1.0, 0.0, 0.0, 0.0, 0.0] if model == K.MODEL_MARKOV6 else [0.0, 1.0]
    o = oracle.solve(model, params, protocols(), y0, T_EVAL, prot_t0=0.0, prot_dt=1.0, prot_of_traj=pot, state_f32=f32, nthreads=nthreads,
                     **weights(net))
    return params, pot, oor, row, y0, o
