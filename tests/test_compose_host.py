"""The shrink-aware tile composition (csrc/ionode_compose.hpp) through libionode.so's host mirror of the rule
(ionode_compose_order_host; the device kernel applies the same compose_slot() to the same total order -- tests/test_gpu_compose.py
compares the two).  No GPU.

The rule: sort by cost descending, ties by index, a non-finite or negative cost counting as 0; tile k takes sorted entries
4 k .. 4 k + 3 as its slots 0 .. 3 and its other 12 slots from the light end, lightest first; only the last tile is ragged; equal
costs everywhere leave index order.

`Every full tile holds exactly four of the top 4 NT` as the issue words it cannot hold when the last tile has fewer than 4 slots
(B = 17: tile 0 is full and must hold 16 of the 17 entries, so at least 7 of the top 8).  The count that the rule fixes is
nH = 4 (NT - 1) + min(4, slots of the last tile), which IS 4 NT whenever the last tile has at least 4 slots; the test asserts
exactly four of the top nH for every B, and therefore exactly four of the top 4 NT wherever that is possible.
"""
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "headline_attempts.npy")
E4_OVER_E16 = 24.3 / 34.08   # DESIGN.md 5.2 stamps: cycles of one evaluation on the 4-trajectory net / on the 16-tile


def numpy_rule(cost):
    """The rule restated."""
    c = np.asarray(cost, dtype=np.float64)
    c = np.where(np.isfinite(c) & (c >= 0), c, 0.0)
    B, NT = len(c), (len(c) + 15) // 16
    if (c == c[0]).all():
        return np.arange(B, dtype=np.int32)
    s = np.lexsort((np.arange(B), -c))                       # descending cost, ties by index
    nH = 4 * (NT - 1) + min(4, B - 16 * (NT - 1))
    heavy, light = s[:nH], s[nH:][::-1]                      # light: lightest first
    order = np.full(B, -1, dtype=np.int32)
    for k in range(NT):
        lo = heavy[4 * k:4 * k + 4]
        li = light[12 * k:12 * k + 12]
        order[16 * k:16 * k + len(lo)] = lo
        order[16 * k + 4:16 * k + 4 + len(li)] = li
    return order


def _costs(B, kind, rng):
    if kind == "random":
        return rng.uniform(0, 1e4, B)
    if kind == "ties":
        return rng.integers(0, 4, B).astype(np.float64)
    if kind == "equal":
        return np.full(B, 7.0)
    if kind == "garbage":
        c = rng.uniform(-10, 1e4, B)
        c[rng.integers(0, B, max(1, B // 5))] = np.nan
        c[rng.integers(0, B, max(1, B // 7))] = np.inf
        c[rng.integers(0, B, max(1, B // 7))] = -np.inf
        return c
    if kind == "all_nan":
        return np.full(B, np.nan)
    raise KeyError(kind)


KINDS = ("random", "ties", "equal", "garbage", "all_nan")


@pytest.mark.parametrize("kind", KINDS)
def test_order_is_a_permutation_with_four_heavies_per_tile_and_matches_the_rule(ion, kind):
    capi = ion.capi
    for B in list(range(1, 71)) + [255, 256, 4095, 4096, 8192]:
        rng = np.random.default_rng(1000 * KINDS.index(kind) + B)
        cost = _costs(B, kind, rng)
        order = capi.compose_order_host(cost)
        assert order.dtype == np.int32 and order.shape == (B,)
        assert np.array_equal(np.sort(order), np.arange(B)), (kind, B)        # a permutation: every slot < B, so only the last tile is ragged
        assert np.array_equal(order, numpy_rule(cost)), (kind, B)
        c = np.where(np.isfinite(cost) & (cost >= 0), cost, 0.0)
        if (c == c[0]).all():
            assert np.array_equal(order, np.arange(B))                         # nothing to compose: index order
            continue
        NT = (B + 15) // 16
        last = B - 16 * (NT - 1)
        nH = 4 * (NT - 1) + min(4, last)
        assert nH == 4 * NT or last < 4
        top = set(np.lexsort((np.arange(B), -c))[:nH].tolist())
        for k in range(NT - 1 if last < 16 else NT):                           # every full tile
            tile = order[16 * k:16 * k + 16]
            assert len(tile) == 16 and sum(int(t) in top for t in tile) == 4, (kind, B, k)
            assert all(int(t) in top for t in tile[:4])
        assert sum(int(t) in top for t in order[16 * (NT - 1):]) == min(4, last)


def test_tile_zero_gets_the_heaviest_and_the_lightest(ion):
    cost = np.arange(64, dtype=np.float64)            # trajectory b costs b
    order = ion.capi.compose_order_host(cost)
    assert order[:4].tolist() == [63, 62, 61, 60] and order[4:16].tolist() == list(range(12))
    assert order[16:20].tolist() == [59, 58, 57, 56] and order[20:32].tolist() == list(range(12, 24))
    assert order[48:52].tolist() == [51, 50, 49, 48] and order[52:64].tolist() == list(range(36, 48))


def tile_times(attempts, order):
    """The model of DESIGN.md 5.2 in units of 6 e16: a tile runs its fifth-largest attempt count on the 16-tile and the rest of its
    largest on the 4-trajectory net."""
    out = []
    for s in range(0, len(order), 16):
        a = np.sort(attempts[order[s:s + 16]])[::-1].astype(np.float64)
        a5 = a[4] if len(a) > 4 else 0.0
        out.append(a5 + (a[0] - a5) * E4_OVER_E16)
    return np.array(out)


def test_replay_on_the_headline_attempt_counts(ion):
    """tests/golden/headline_attempts.npy (make_headline_attempts.py: the oracle's accepted / rejected counts of bench.py's own 4096
    trajectories): composed with the exact counts as cost, the slowest tile under the model is at most 0.97 of index order's."""
    ar = np.load(FIXTURE)
    assert ar.dtype == np.int32 and ar.shape == (4096, 2)
    attempts = ar.sum(axis=1)
    index = tile_times(attempts, np.arange(4096))
    order = ion.capi.compose_order_host(attempts)
    composed = tile_times(attempts, order)
    ratio = composed.max() / index.max()
    print(f"index-order max {index.max():.1f}, composed max {composed.max():.1f} (units of 6 e16 attempts), ratio {ratio:.4f}")
    assert ratio <= 0.97, ratio
    # the bound the composition aims at: the heaviest trajectory alone on the 4-trajectory net, plus its 12 light companions' share
    assert composed.max() >= attempts.max() * E4_OVER_E16
