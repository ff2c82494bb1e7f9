"""-m gpu: the device primitives of csrc/ionode_math.hpp (and compose_cost of csrc/ionode_compose.hpp) one by one, through the
test-only probe library (tests/csrc/ionode_probe.hip), at the inputs no solve on physical parameters reaches: exp arguments up to
and beyond both range edges (subnormal results, the overflow edge, NaN, inf), the fifth root over the whole double range, the
corrected divisions against IEEE division bit for bit -- the fp32 one for all 2^32 inputs -- and the cross-lane / inline-asm
helpers.  References: the oracle's C copies (bits), numpy's IEEE arithmetic (bits), mpmath / decimal at 60 digits (accuracy)."""
import ctypes
import math

import numpy as np
import pytest

from gpu_util import probe, probe_div_constf_sweep

pytestmark = pytest.mark.gpu

EXP_HI = 709.782712893384          # above: +inf
EXP_LO = -745.1332191019412        # below: +0
DBL_MAX = np.finfo(np.float64).max
TINY = 2.0 ** -1074


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.uint64 if x.dtype == np.float64 else np.uint32)


def _same_bits(got, want):
    """bit equality of two float arrays; returns the number of differing elements"""
    return int(np.sum(_bits(got) != _bits(want)))


def _same_bits_nan_as_nan(got, want):
    bad = (_bits(got) != _bits(want)) & ~(np.isnan(got) & np.isnan(want))
    return int(np.sum(bad))


def _neighbours(v):
    v = np.float64(v)
    return [np.nextafter(v, -np.inf), v, np.nextafter(v, np.inf)]


def _qnan(sign):
    return np.array([0x7ff8000000000000 | (sign << 63)], dtype=np.uint64).view(np.float64)[0]


def _oracle_fn(oracle, name):
    fn = getattr(oracle.lib(), name)
    fn.restype = ctypes.c_double
    fn.argtypes = [ctypes.c_double]
    return lambda x: np.array([fn(float(v)) for v in x], dtype=np.float64)


# ---- high-precision references: mpmath when it imports, decimal otherwise; 60 digits ----
try:
    import mpmath as _mp
    _mp.mp.dps = 60

    def _hp(x):
        return _mp.mpf(float(x))
    _hp_exp = lambda x: _mp.exp(_hp(x))
    _hp_root5 = lambda x: _mp.root(_hp(x), 5)
    _hp_abs, _hp_float = abs, float
except ImportError:                                   # pragma: no cover
    import decimal as _dec
    _dec.getcontext().prec = 60
    _dec.getcontext().Emin, _dec.getcontext().Emax = -999999, 999999

    def _hp(x):
        return _dec.Decimal(float(x))
    _hp_exp = lambda x: _hp(x).exp()
    _hp_root5 = lambda x: (_hp(x).ln() / 5).exp()
    _hp_abs, _hp_float = abs, float


def _err_in_spacings(got, exact):
    """|got - exact| in units of got's spacing (2^-1074 for a subnormal or zero result); an infinite result counts as 2^1024, the value
    the overflow rounds from."""
    if math.isinf(got):
        g, sp = _hp(2.0 ** 1023) * 2, _hp(2.0 ** 971)
        if exact >= g:
            return 0.0
    else:
        g, sp = _hp(got), _hp(float(np.spacing(abs(np.float64(got)))))
    return _hp_float(_hp_abs(g - exact) / sp)


# =====================================================================================================================================
# exp
# =====================================================================================================================================
@pytest.fixture(scope="module")
def exp_points(ion, gpu):
    rng = np.random.default_rng(0)
    edge = []
    for v in (EXP_HI, EXP_LO, 708.0, -708.0):
        edge += _neighbours(v)
    special = [0.0, -0.0, 1e-300, -1e-300, TINY, -TINY, 2.2250738585072014e-308, -2.2250738585072014e-308, 1e-20, -1e-20, 1.0, -1.0,
               np.inf, -np.inf, 1e300, -1e300, 2.0 ** 31, -(2.0 ** 31), 2.0 ** 31 + 4096.0, -(2.0 ** 31) - 4096.0, 1e10, -1e10,
               _qnan(0), _qnan(1)]
    x = np.concatenate([rng.uniform(-20, 20, 60000), rng.uniform(-708, 708, 60000), 709.79 - rng.uniform(0, 1.79, 20000),
                        -708.0 - rng.uniform(0, 37.2, 40000)[::-1], rng.uniform(-760, -745, 2000), rng.uniform(709.7, 720, 2000),
                        np.array(edge), np.array(special)])
    x[120000:140000] = np.maximum(x[120000:140000], np.nextafter(708.0, np.inf))    # (708, 709.79]
    x[140000:180000] = np.minimum(x[140000:180000], np.nextafter(-708.0, -np.inf))  # [-745.2, -708)
    dev = {name: probe(ion, gpu, name, x) for name in ("det_exp", "det_exp_ldexp", "det_exp_s")}
    inr = np.abs(x) <= 708.0     # det_exp_inrange's contract (NaN excluded by the comparison)
    dev["det_exp_inrange"] = probe(ion, gpu, "det_exp_inrange", x[inr])
    return x, inr, dev


def test_exp_inputs_cover_every_range_case(exp_points):
    x, inr, dev = exp_points
    e = dev["det_exp"]
    assert x.size <= 1 << 20
    sub = (e > 0) & (e < 2.2250738585072014e-308)
    assert sub.sum() > 30000 and (e[x < EXP_LO] == 0).sum() > 1000 and np.isinf(e[x > EXP_HI]).sum() > 1000
    assert inr.sum() > 100000 and (~inr).sum() > 60000 and np.isnan(x).sum() == 2


@pytest.mark.parametrize("name", ["det_exp_ldexp", "det_exp_s", "det_exp_inrange"])
def test_exp_variants_return_det_exps_bits(exp_points, name):
    """v_ldexp_f64 scaling, scalar-operand constants, the selects behind the polynomial, the form without range cases: the same bits
    as det_exp on the device, subnormal results, both edges, NaN and inf included."""
    x, inr, dev = exp_points
    want = dev["det_exp"][inr] if name == "det_exp_inrange" else dev["det_exp"]
    bad = _bits(dev[name]) != _bits(want)
    xs = x[inr] if name == "det_exp_inrange" else x
    assert not bad.any(), (name, int(bad.sum()), xs[bad][:5], dev[name][bad][:5], want[bad][:5])


def test_exp_matches_the_oracle_bit_for_bit(exp_points, oracle):
    x, inr, dev = exp_points
    want = _oracle_fn(oracle, "det_exp")(x)
    for name in ("det_exp", "det_exp_ldexp", "det_exp_s"):
        bad = _bits(dev[name]) != _bits(want)
        assert not bad.any(), (name, int(bad.sum()), x[bad][:5], dev[name][bad][:5], want[bad][:5])
    assert _same_bits(dev["det_exp_inrange"], want[inr]) == 0


@pytest.mark.parametrize("name", ["det_exp", "det_exp_ldexp", "det_exp_s"])
def test_exp_range_cases(exp_points, name):
    x, _, dev = exp_points
    e = dev[name]
    nan = np.isnan(x)
    assert np.isnan(e[nan]).all() and not np.isnan(e[~nan]).any()
    assert (x > EXP_HI).sum() > 1000 and (e[x > EXP_HI] == np.inf).all()
    assert (x < EXP_LO).sum() > 1000 and (_bits(e[x < EXP_LO]) == 0).all()                 # +0, not -0
    assert e[x == 0.0].tolist() == [1.0, 1.0]


def test_expf_is_the_rounded_fp64_exp(ion, gpu, exp_points):
    """det_expf(x) == float32(det_exp(float64(x))), over fp32 arguments whose results are normal, subnormal (x in about [-103.3, -87.3]),
    zero, infinite and NaN."""
    x64, _, _ = exp_points
    rng = np.random.default_rng(1)
    with np.errstate(over="ignore"):
        x = np.concatenate([x64[:120000:3], rng.uniform(-104.5, -86.5, 30000), rng.uniform(88.0, 89.5, 5000), x64[-40:]]).astype(np.float32)
    got = probe(ion, gpu, "det_expf", x)
    with np.errstate(over="ignore", under="ignore"):
        want = probe(ion, gpu, "det_exp", x.astype(np.float64)).astype(np.float32)
    sub = (want > 0) & (want < np.finfo(np.float32).tiny)
    assert sub.sum() > 10000 and np.isinf(want).sum() > 1000 and np.isnan(want).sum() == 2
    assert _same_bits(got, want) == 0, (x[_bits(got) != _bits(want)][:5])


def test_exp_is_within_one_spacing_of_the_true_exponential(exp_points):
    """The header's claim (< 1 ulp), subnormal results and both edges included; the spacing of a subnormal or zero result is 2^-1074."""
    x, _, dev = exp_points
    e = dev["det_exp"]
    rng = np.random.default_rng(2)
    pick = np.concatenate([rng.choice(120000, 9000, replace=False), 120000 + rng.choice(20000, 3000, replace=False),
                           140000 + rng.choice(40000, 6000, replace=False), 180000 + rng.choice(4000, 1000, replace=False),
                           np.arange(184000, x.size)])
    pick = pick[np.isfinite(x[pick])]
    assert pick.size <= 20000
    worst, worst_sub, at = 0.0, 0.0, None
    for i in pick:
        err = _err_in_spacings(float(e[i]), _hp_exp(x[i]))
        if err > worst:
            worst, at = err, float(x[i])
        if 0 < e[i] < 2.2250738585072014e-308:
            worst_sub = max(worst_sub, err)
    print(f"det_exp on the device: max error {worst:.3f} spacings (at x = {at!r}); subnormal results {worst_sub:.3f}; {pick.size} points")
    assert worst < 1.0, (worst, at)


# =====================================================================================================================================
# fifth root
# =====================================================================================================================================
@pytest.fixture(scope="module")
def root5_points(ion, gpu):
    rng = np.random.default_rng(3)
    normal = np.concatenate([10.0 ** rng.uniform(-300, 300, 50000),
                             DBL_MAX * (1.0 - rng.uniform(0, 1e-3, 1000)), DBL_MAX * rng.uniform(0.01, 1.0, 1000),
                             [DBL_MAX, np.nextafter(DBL_MAX, 0), 2.2250738585072014e-308, 1.0, 32.0, 243.0, 1e-5, 0.01, 3.0]])
    sub = np.concatenate([rng.integers(1, 1 << 52, 3000).astype(np.uint64).view(np.float64),
                          (np.uint64(1) << rng.integers(0, 52, 200).astype(np.uint64)).view(np.float64),
                          [TINY, 2 * TINY, np.nextafter(2.2250738585072014e-308, 0)]])
    other = np.array([0.0, -0.0, -3.0, -1e-320, -np.inf, np.inf, _qnan(0), _qnan(1)])
    x = np.concatenate([normal, sub, other])
    return x, normal.size, sub.size, probe(ion, gpu, "det_root5", x)


def test_root5_matches_the_oracle_bit_for_bit(root5_points, oracle):
    """The device divides by five with div_by(.., 5.0, 0.2), the oracle writes `/ 5.0`: the same bits over the whole double range --
    normal, subnormal, near DBL_MAX -- and 0, -0, negative, inf and NaN come back unchanged."""
    x, n_norm, n_sub, got = root5_points
    want = _oracle_fn(oracle, "det_root5")(x)
    bad = _bits(got) != _bits(want)
    assert not bad.any(), (int(bad.sum()), x[bad][:5], got[bad][:5], want[bad][:5])
    assert (_bits(got[n_norm + n_sub:]) == _bits(x[n_norm + n_sub:])).all()


def test_root5_is_within_two_ulp_for_normal_inputs(root5_points):
    """The header's claim.  Subnormal inputs are outside it (seven Newton steps from the exponent-field guess do not converge there:
    det_root5(5e-324) = 5.5e-63 for 2.2e-65); for them only the equality with the oracle above is asserted."""
    x, n_norm, n_sub, got = root5_points
    rng = np.random.default_rng(4)
    pick = np.concatenate([rng.choice(50000, 17000, replace=False), np.arange(50000, n_norm)])
    assert pick.size <= 20000
    worst, at = 0.0, None
    for i in pick:
        err = _err_in_spacings(float(got[i]), _hp_root5(x[i]))
        if err > worst:
            worst, at = err, float(x[i])
    print(f"det_root5 on the device: max error {worst:.3f} ulp (at x = {at!r}); {pick.size} normal inputs")
    assert worst <= 2.0, (worst, at)
    s = got[n_norm:n_norm + n_sub]
    assert np.isfinite(s).all() and (s > 0).all()    # subnormal inputs: finite and positive, accuracy not claimed


# =====================================================================================================================================
# divisions
# =====================================================================================================================================
def _rand_scaled(rng, n, emin, emax):
    return np.ldexp(rng.uniform(1.0, 2.0, n), rng.integers(emin, emax + 1, n)) * rng.choice([-1.0, 1.0], n)


def test_div_by_is_the_ieee_quotient(ion, gpu):
    """RN(a / b) from a * RN(1 / b) and one fma correction: random operands with exponents in [-400, 400], the operands the kernels form
    (t - prot_t0 and voltage differences over prot_dt), the steps of det_root5's Newton iteration over 5, and the pass-through of
    zero, infinite and NaN quotients (returned as a * rb)."""
    rng = np.random.default_rng(5)
    n = 200000
    a, b = [_rand_scaled(rng, n, -400, 400)], [_rand_scaled(rng, n, -400, 400)]
    for dt in (0.1, 0.5, 1.0, 2.0, 1.0 / 3.0):
        t0 = rng.choice([0.0, 10.0, 0.3, 1234.5], 60000)
        t = np.concatenate([t0[:40000] + rng.uniform(0, 1e5, 40000), t0[40000:] + rng.integers(0, 100000, 20000) * dt])   # ... and grid points
        a += [t - t0, rng.uniform(-120, 60, 40000) - rng.uniform(-120, 60, 40000)]
        b += [np.full(60000, dt), np.full(40000, dt)]
    a += [10.0 ** rng.uniform(-100, 100, 50000)]
    b += [np.full(50000, 5.0)]
    a, b = np.concatenate(a), np.concatenate(b)
    assert a.size <= 1 << 20
    with np.errstate(all="ignore"):
        rb = 1.0 / b
        got = probe(ion, gpu, "div_by", a, b, rb)
        bad = _same_bits(got, a / b)
        print(f"div_by: {bad} mismatches of {a.size}")
        assert bad == 0
        # pass-through: the quotient a * rb is zero, infinite or NaN
        pa = np.array([0.0, -0.0, 0.0, np.inf, -np.inf, np.nan, 3.0, -3.0, 3.0, 0.0, 1e-200, 1e200, -1e200, 5e-324])
        pb = np.array([2.0, 2.0, -0.5, 2.0, 0.1, 1.0, np.inf, np.inf, 0.0, 0.0, 1e200, 1e-200, 1e-200, 3.0])
        prb = 1.0 / pb
        pq = pa * prb
        assert ((pq == 0) | ~np.isfinite(pq)).all()
        pg = probe(ion, gpu, "div_by", pa, pb, prb)
        assert _same_bits_nan_as_nan(pg, pq) == 0, (pg, pq)


def test_div_pos_is_the_ieee_quotient_on_its_domain(ion, gpu):
    """x = (t_k - t0) / (t1 - t0) of a dense-output sample, t0 < t_k <= t1: steps from 1e-9 to 1e3 ms at t0 up to 1e5 ms, plus a == 0
    (a zero stays +0) and a == b."""
    rng = np.random.default_rng(6)
    n = 400000
    t0 = np.concatenate([rng.uniform(0, 1e5, n // 2), rng.uniform(0, 100, n // 4), np.zeros(n // 4)])
    t1 = t0 + 10.0 ** rng.uniform(-9, 3, n)
    u = np.concatenate([rng.uniform(0, 1, n // 2), 2.0 ** rng.uniform(-40, 0, n // 2)])
    rng.shuffle(u)
    tk = np.minimum(np.maximum(t0 + u * (t1 - t0), np.nextafter(t0, np.inf)), t1)
    a, b = tk - t0, t1 - t0
    a = np.concatenate([a, np.zeros(1000), b[:1000]])
    b = np.concatenate([b, b[:1000], b[:1000]])
    assert (b > 0).all() and (a >= 0).all() and (a <= b).all() and ((a == 0) | (a / b >= 2.0 ** -70)).all()
    got = probe(ion, gpu, "div_pos", a, b, 1.0 / b)
    bad = _same_bits(got, a / b)
    print(f"div_pos: {bad} mismatches of {a.size}")
    assert bad == 0
    assert (_bits(got[n:n + 1000]) == 0).all() and (got[n + 1000:] == 1.0).all()


def test_div_const_is_the_ieee_quotient_over_the_whole_double_range(ion, gpu):
    """div_const(a, 100.0, 0.01): every exponent, quotients in the subnormal range and at the guard's two thresholds (where the true
    division takes over), zero, inf and NaN."""
    rng = np.random.default_rng(7)
    a = np.concatenate([rng.integers(0, 1 << 64, 400000, dtype=np.uint64).view(np.float64),          # every exponent, NaNs included
                        _rand_scaled(rng, 100000, -1074, -1000), _rand_scaled(rng, 50000, -905, -885), _rand_scaled(rng, 50000, 895, 915),
                        _rand_scaled(rng, 20000, 1010, 1023), rng.uniform(-180, 180, 100000),
                        rng.integers(0, 1 << 52, 20000, dtype=np.uint64).view(np.float64),              # subnormal a
                        [0.0, -0.0, np.inf, -np.inf, np.nan, DBL_MAX, -DBL_MAX, TINY, -TINY, 100 * TINY, 50 * TINY, 49 * TINY, 150 * TINY]])
    assert a.size <= 1 << 20
    with np.errstate(all="ignore"):
        want = a / 100.0
    got = probe(ion, gpu, "div_const_100", a)
    sub = (np.abs(want) > 0) & (np.abs(want) < 2.2250738585072014e-308)
    assert sub.sum() > 50000
    bad = _same_bits_nan_as_nan(got, want)
    print(f"div_const: {bad} mismatches of {a.size} ({int(sub.sum())} subnormal quotients)")
    assert bad == 0


def test_div_constf_equals_the_division_for_every_fp32_input(ion, gpu):
    """The exhaustive check csrc/ionode_math.hpp cites: all 2^32 bit patterns through div_constf(x, 1000.0f, 0.001f) against the
    device's own x / 1000.0f in one kernel (NaN compared as NaN), and 2^22 random patterns -- in chunks of 2^20 -- against numpy's
    float32 division."""
    bad, seen, same = probe_div_constf_sweep(ion, gpu)
    print(f"div_constf: {bad} mismatches of {seen} patterns ({seen - same} NaN results with other bits)")
    assert seen == 1 << 32
    assert bad == 0
    rng = np.random.default_rng(8)
    thousand = np.float32(1000.0)
    n_bad = 0
    for _ in range(4):
        x = rng.integers(0, 1 << 32, 1 << 20, dtype=np.uint64).astype(np.uint32).view(np.float32)
        with np.errstate(all="ignore"):
            want = x / thousand
        assert want.dtype == np.float32
        n_bad += _same_bits_nan_as_nan(probe(ion, gpu, "div_constf_1000", x), want)
    print(f"div_constf: {n_bad} mismatches of {4 << 20} random patterns against numpy")
    assert n_bad == 0


# =====================================================================================================================================
# the other primitives
# =====================================================================================================================================
def test_lrelu_is_leaky_relu_for_every_kind_of_input(ion, gpu):
    """v_max_f32(x, 0.01 x) issued from inline asm against nn.LeakyReLU(0.01)'s definition: equal bits for every non-NaN input (+-0,
    subnormals, +-inf included), NaN stays NaN (quiet or signalling, either sign)."""
    special = np.array([0x00000000, 0x80000000, 0x7f800000, 0xff800000, 0x7f7fffff, 0xff7fffff, 0x00800000, 0x80800000, 0x00000001,
                        0x80000001, 0x007fffff, 0x807fffff, 0x3f800000, 0xbf800000, 0x7fc00000, 0xffc00000, 0x7f800001, 0xff800001,
                        0x7fa00000, 0xffa00000, 0x7fffffff, 0xffffffff, 0x00000064, 0x80000064, 0x80000031, 0x80000032, 0x80000033],
                       dtype=np.uint32)
    rng = np.random.default_rng(9)
    x = np.concatenate([special, rng.integers(0, 1 << 32, (1 << 20) - special.size, dtype=np.uint64).astype(np.uint32)]).view(np.float32)
    assert x.size == 1 << 20
    got = probe(ion, gpu, "lrelu", x)
    with np.errstate(all="ignore"):
        want = np.where(x > 0, x, (x * np.float32(0.01)).astype(np.float32))
    nan = np.isnan(x)
    assert nan.sum() > 1000 and np.isnan(got[nan]).all()
    bad = _bits(got[~nan]) != _bits(want[~nan])
    assert not bad.any(), (int(bad.sum()), x[~nan][bad][:5], got[~nan][bad][:5], want[~nan][bad][:5])


def test_group8_sum_adds_in_the_documented_order(ion, gpu):
    """Three DPP steps -- lane ^ 1, lane ^ 2, the mirror of the half row -- in fp64: the same pairwise order in numpy, bit for bit, and
    every lane of a group of 8 holds the same sum."""
    rng = np.random.default_rng(10)
    x = (rng.normal(0, 1, 64 * 512) * 10.0 ** rng.uniform(-8, 8, 64 * 512)).reshape(-1, 8)
    x[:4] = [[1e16, 1.0, -1e16, 1.0, 3.0, 1e-3, -3.0, 7.0], [np.inf, 1, 2, 3, 4, 5, 6, 7], [0.0] * 8, [-0.0] * 8]
    i = np.arange(8)
    s1 = x + x[:, i ^ 1]
    s2 = s1 + s1[:, i ^ 2]
    want = s2 + s2[:, 7 - i]
    got = probe(ion, gpu, "group8_sum_f64", x.reshape(-1)).reshape(-1, 8)
    assert _same_bits_nan_as_nan(got, want) == 0
    assert (_bits(got[2:]) == _bits(got[2:, :1])).all()
    assert not np.array_equal(want[4:, 0], np.cumsum(x[4:], axis=1)[:, -1])    # the order matters on these inputs: left to right rounds differently somewhere


def test_mbcnt_counts_the_set_bits_below_the_lane(ion, gpu):
    rng = np.random.default_rng(11)
    n = 64 * 256
    m = rng.integers(0, 1 << 64, n, dtype=np.uint64)                      # a mask of its own per lane
    uni = np.repeat(rng.integers(0, 1 << 64, n // 64 // 2, dtype=np.uint64), 64)   # ... and wavefront-uniform masks, as the kernels pass
    m[:uni.size] = uni
    m[:64], m[64:128], m[128:192], m[192:256] = 0, 0xFFFFFFFFFFFFFFFF, 0xFFFFFFFF00000000, 0x00000000FFFFFFFF
    lane = (np.arange(n) % 64).astype(np.uint64)
    below = m & ((np.uint64(1) << lane) - np.uint64(1))
    want = np.array([bin(int(v)).count("1") for v in below], dtype=np.int32)
    assert np.array_equal(probe(ion, gpu, "mbcnt", m), want)
    acc = rng.integers(-1000, 1000, n).astype(np.int32)
    assert np.array_equal(probe(ion, gpu, "mbcnt", m, acc), want + acc)


def test_compose_cost_reads_costs_as_the_rule_says(ion, gpu):
    """csrc/ionode_compose.hpp: a non-finite or negative cost counts as 0, every other cost as itself."""
    rng = np.random.default_rng(12)
    c = np.concatenate([rng.integers(0, 1 << 64, 100000, dtype=np.uint64).view(np.float64), rng.uniform(-10, 5000, 10000),
                        [0.0, -0.0, np.inf, -np.inf, np.nan, -np.nan, DBL_MAX, -DBL_MAX, TINY, -TINY, 1.0, -1.0]])
    with np.errstate(all="ignore"):
        want = np.where(np.isfinite(c) & (c >= 0), c, 0.0)
    assert _same_bits(probe(ion, gpu, "compose_cost", c), want) == 0
