"""tests/site_expectation_statement.py -- the closed form behind `--site_proba expected` -- is the exact value, and the
reference's sampled site probabilities are estimates of it: every stored reference run lies within six of ITS OWN standard
errors (mc_sigma / sqrt(T), from the statement) of the statement's value.  No GPU."""
import math

import numpy as np
import pytest

import site_expectation_statement as SE

K = 20


def exact(p, k):
    """the same formula with math.fsum and Python integer powers: (site_prob, mc_sigma) as Python floats"""
    u = [1.0 - float(x) for x in p]
    n = len(u)
    m1, m2 = math.fsum(u) / n, math.fsum(x * x for x in u) / n
    q1, q2 = m1 ** k, m2 ** k
    return 1.0 - q1, math.sqrt(max(q2 - q1 * q1, 0.0))


def golden_bags(golden):
    """(name, read_prob, off) of every set of read probabilities under tests/golden that pairs up with its offsets"""
    s = golden("synthetic_small.npz")
    b, bp = golden("bundled_inputs.npz"), golden("bundled_readprob.npz")
    r = golden("reference_at_scale.npz")
    out = [("uniform20", s["uniform20_readprob"], s["uniform20_off"]), ("ragged", s["ragged_readprob"], s["ragged_off"])]
    out += [("bundled_" + m, bp[m], b["off"]) for m in bp.files]
    out += [("scale_hct116", r["uniform_hct116_readprob"][:20 * 2000], r["uniform_off"][:2001])]
    return out


@pytest.fixture(scope="module")
def against_fsum(golden):
    """per golden bag: (name, site, |site_prob - fsum formula| before the rounding to float32, |mc_sigma - fsum formula|)"""
    rows = []
    for name, p, off in golden_bags(golden):
        site, sigma, _ = SE.site_expectation(p, off, K)
        for s in range(off.size - 1):
            bag = p[off[s]:off[s + 1]]
            e_site, e_sigma = exact(bag, K)
            e64, g64 = SE.expectation_f64(bag[None, :], K)
            assert site[s] == np.float32(e64[0]) and sigma[s] == g64[0], (name, s)     # the float32 written is that float64, rounded
            rows.append((name, s, abs(float(e64[0]) - e_site), abs(float(sigma[s]) - e_sigma)))
    return rows


def test_statement_site_prob_is_the_exact_value(against_fsum):
    """site_prob before its rounding to float32, against math.fsum and Python powers: 1e-14 absolute (measured: 1.1e-16)"""
    print("largest |statement - fsum formula|, site_prob: %.3g" % max(r[2] for r in against_fsum))
    for name, s, d_site, _ in against_fsum:
        assert d_site <= 1e-14, (name, s, d_site)


def test_statement_mc_sigma_is_the_exact_value(against_fsum):
    """mc_sigma against the same formula with math.fsum and Python powers: 1e-14 absolute (measured: 3.9e-15).  The difference
    m2^K - (m1^K)^2 cancels, so this holds only because the statement's sums and powers are rounded once (pairs of doubles): with
    plain float64 sums and products the two evaluations were up to 5.3e-9 apart on these bags."""
    print("largest |statement - fsum formula|, mc_sigma: %.3g" % max(r[3] for r in against_fsum))
    for name, s, _, d_sigma in against_fsum:
        assert d_sigma <= 1e-14, (name, s, d_sigma)


@pytest.mark.parametrize("k", [1, 20, 64])
def test_value_edges(k):
    f32 = np.float32
    site, sigma, _ = SE.uniform_expectation(np.zeros((1, 20), f32), k)
    assert site[0] == 0.0 and not np.signbit(site[0]) and sigma[0] == 0.0      # all p = 0: exactly 0.0
    site, sigma, _ = SE.uniform_expectation(np.ones((1, 1), f32), k)
    assert site[0] == 1.0 and sigma[0] == 0.0                                   # one read with p = 1: exactly 1.0
    for n in (1, 2, 20, 65):                                                    # n = 1 and beyond, against the fsum formula
        for v in (f32(1e-30), f32(1.0) - f32(2.0 ** -24), f32(0.5), f32(1.0), f32(0.0)):
            bag = np.full((1, n), v, f32)
            e64, g64 = SE.expectation_f64(bag, k)
            e_site, e_sigma = exact(bag[0], k)
            assert abs(float(e64[0]) - e_site) <= 1e-14, (n, v)
            assert g64[0] <= 1e-7 and e_sigma <= 1e-7                           # equal reads: the variance is a rounding residue
    site, _, _ = SE.uniform_expectation(np.array([[1e-30]], f32), k)
    assert site[0] == 0.0                                                       # 1 - 1e-30 is 1.0 in float64
    site, _, _ = SE.uniform_expectation(np.array([[f32(1.0) - f32(2.0 ** -24)]], f32), k)
    assert site[0] == f32(1.0 - (2.0 ** -24) ** k)                              # u = 2^-24 exactly, its powers are exact
    empty = SE.site_expectation(np.zeros(0, f32), np.array([0, 0]), k, 0.5)
    assert all(np.isnan(x[0]) for x in empty)
    nan = SE.uniform_expectation(np.array([[0.25, np.nan, 0.5]], f32), k, 0.1)  # NaN propagates and is below every threshold
    assert np.isnan(nan[0][0]) and np.isnan(nan[1][0]) and nan[2][0] == 2.0 / 3.0
    site, sigma, _ = SE.uniform_expectation(np.array([[1.5, 0.25]], f32), k)    # outside [0, 1]: arithmetic, not a check
    assert site[0] == f32(1.0 - SE.int_power(np.array([(-0.5 + 0.75) / 2.0]), k)[0])


def test_one_order_for_every_bag_size():
    """a bag of <= 32 reads folded over 32 partial pairs gives the bits of 64 (what lets two kernel variants share the order), and
    the CSR form groups bags by size without changing a bit"""
    g = np.random.Generator(np.random.PCG64(5))
    for n in (1, 2, 19, 20, 21, 32):
        u = 1.0 - g.random((50, n), np.float32).astype(np.float64)
        pad = np.zeros((50, 32))
        pad[:, :n] = u
        a = SE.pair_add_double((np.zeros((50, 32)), np.zeros((50, 32))), pad)
        h = 16
        while h >= 1:
            a = SE.pair_add((a[0][:, :h], a[1][:, :h]), (a[0][:, h:2 * h], a[1][:, h:2 * h]))
            h //= 2
        assert np.array_equal(a[0][:, 0], SE.fold_sums(u))
    sizes = g.integers(1, 200, size=300)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    p = g.random(int(off[-1]), np.float32)
    site, sigma, mod = SE.site_expectation(p, off, K, 0.5)
    for s in (0, 17, 299):
        one = SE.uniform_expectation(p[off[s]:off[s + 1]][None, :], K, 0.5)
        assert (site[s], sigma[s], mod[s]) == (one[0][0], one[1][0], one[2][0])


def reference_runs(golden):
    """(name, reference site_prob, read_prob, off, T) -- every stored reference run whose read probabilities pair up with its offsets
    (the ragged_* arrays of reference_at_scale.npz do not: they are shorter than ragged_off[-1])"""
    r = golden("reference_at_scale.npz")
    off = r["uniform_off"][:10001]
    for m in ("hct116", "arabidopsis", "hek293t_glori", "hek293t_m6ace"):
        yield "scale_" + m, r["uniform_%s_site_T1000" % m], r["uniform_%s_readprob" % m][:int(off[-1])], off, 1000
    s = golden("synthetic_small.npz")
    for name in ("uniform20", "ragged"):
        for T in (100, 1000):
            yield "%s_T%d" % (name, T), s["%s_site_T%d" % (name, T)], s[name + "_readprob"], s[name + "_off"], T
    b, p = golden("bundled_inputs.npz"), golden("bundled_readprob.npz")["hct116"]
    site = golden("bundled_site.npz")
    for key, T in (("T5_bs16_spb2_seed0", 5), ("T50_bs8_spb3_seed0", 50), ("T100_bs16_spb2_seed0", 100), ("T1000_bs16_spb2_seed0", 1000)):
        w = site[key + "_written"].astype(bool)
        yield "bundled_" + key, (site[key + "_site"], w), p, b["off"], T


def test_the_reference_estimates_the_statement(golden):
    worst = (0.0, None)
    for name, ref, p, off, T in reference_runs(golden):
        mask = None
        if isinstance(ref, tuple):
            ref, mask = ref
        want, sigma, _ = SE.site_expectation(p, off, K)
        d = np.abs(ref.astype(np.float64) - want.astype(np.float64))
        bound = 6.0 * sigma / math.sqrt(T) + 2e-6
        if mask is not None:
            d, bound, sigma = d[mask], bound[mask], sigma[mask]
        ratio = np.max(np.where(d > 2e-6, d * math.sqrt(T) / np.maximum(sigma, 1e-300), 0.0))     # printed; the assertion is below
        print("%-32s T=%-4d sites %-6d largest |ref - E| %.4g, in standard errors %.2f" % (name, T, d.size, d.max(), ratio))
        worst = max(worst, (float(ratio), name))
        bad = np.flatnonzero(~(d <= bound))
        assert bad.size == 0, (name, bad[:5], d[bad[:5]], bound[bad[:5]])
    print("largest ratio", worst)
