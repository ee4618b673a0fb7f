"""tests/ks_exact_statement.py, the recurrence behind m6a_ks_exact (include/m6a.h), held to two things that are not it.
Exact rational path counts: the inside paths from (0, 0) to (n, m) counted in Python integers, p = 1 - inside / C(n + m, n) as a Fraction,
for all n, m <= 12 and every multiple of gcd(n, m) up to n m and one beyond -- relative error at most 4 (n + m) 2^-53 (a path takes n + m
steps and a step rounds three times: a product, the sum, the division; every term is positive, so the errors do not grow by cancellation),
and exactly 0.0 where the truth is 0.  scipy.stats.ks_2samp(method="exact") on drawn pairs from 20 + 20 to 999 + 1000 reads at several
shifts, h being tests/ks_statement.py's integers: 1e-10 relative, the project's tolerance for a p-value, and 0.0 where scipy gives 0.
And the undefined rules with both caps, at the cap and one past it."""
import math
from fractions import Fraction

import numpy as np
import pytest

import ks_exact_cases as KE
import ks_exact_statement as ST
import ks_statement as KS


def truth(n, m, h):
    """P(a uniformly drawn monotone path from (0, 0) to (n, m) meets a cell with |m i - n j| >= h), exactly"""
    if h <= 0:
        return Fraction(1)
    row = [0] * (m + 1)                                          # row[j]: the inside paths from (0, 0) to (i, j)
    for i in range(n + 1):
        for j in range(m + 1):
            if abs(m * i - n * j) >= h:
                row[j] = 0
            elif i == 0 and j == 0:
                row[j] = 1
            else:
                row[j] = (row[j] if i > 0 else 0) + (row[j - 1] if j > 0 else 0)
    return 1 - Fraction(row[m], math.comb(n + m, n))


def test_statement_against_exact_path_counts():
    worst = 0.0
    for n in range(1, 13):
        for m in range(1, 13):
            g = math.gcd(n, m)
            for h in list(range(0, n * m + 1, g)) + [n * m + g]:
                want, got = truth(n, m, h), ST.p_exact(n, m, h)
                if want == 0:
                    assert got == 0.0 and h > n * m, (n, m, h, got)
                    continue
                err = abs(Fraction(got) - want) / want
                worst = max(worst, float(err * 2 ** 53 / (n + m)))
                assert err <= Fraction(4 * (n + m), 2 ** 53), (n, m, h, got, float(want))
    print("worst relative error: %.3f (n + m) 2^-53" % worst)
    assert ST.p_exact(5, 7, 0) == 1.0 and ST.p_exact(5, 7, 1) == 1.0       # coprime sizes, h = 1: both neighbours of (0, 0) are outside


def test_statement_is_symmetric_to_the_bit():
    for n, m, h in ((3, 5, 7), (20, 35, 210), (64, 63, 1000), (129, 65, 3000), (12, 200, 900)):
        assert KE.same_bits([ST.p_exact(n, m, h)], [ST.p_exact(m, n, h)])


def test_statement_against_scipy():
    stats = pytest.importorskip("scipy.stats")
    rng = np.random.default_rng(7)
    worst, n_zero = 0.0, 0
    for n, m in ((20, 20), (20, 35), (50, 47), (100, 100), (250, 300), (999, 1000)):
        for shift in (0.0, 0.1, 0.3, 0.6, 1.0, 2.0, 9.0):              # 9.0: the bags apart, p = 2 / C(n + m, n), 0.0 at 999 + 1000
            a = rng.normal(0.0, 1.0, n).astype(np.float32)
            b = (rng.normal(shift, 1.0, m)).astype(np.float32)
            d_pos, d_neg, _, _ = KS.pair(a, b)
            got = ST.p_exact(n, m, max(d_pos, d_neg))
            r = stats.ks_2samp(a.astype(np.float64), b.astype(np.float64), method="exact")
            assert r.statistic == max(d_pos, d_neg) / (n * m)                     # the same statistic goes into both
            if r.pvalue == 0.0:
                n_zero += 1
                assert got == 0.0, (n, m, shift, got)
                continue
            ratio = abs(got - r.pvalue) / r.pvalue
            worst = max(worst, ratio)
            assert ratio <= 1e-10, (n, m, shift, got, r.pvalue)
    print("worst |statement - scipy| / scipy: %.3g over 42 pairs, %d of them 0.0 on both sides" % (worst, n_zero))
    assert n_zero >= 1


def test_undefined_items_and_both_caps():
    for n, m, h in ((0, 5, 1), (5, 0, 1), (-1, 5, 1), (5, 5, -1), (5, 5, -(1 << 40))):
        assert math.isnan(ST.p_exact(n, m, h)), (n, m, h)
    assert ST.SHORT == 2047 and ST.CELLS == 10 ** 8
    for name, item in KE.SPECIAL.items():
        if "cap" in name or name in KE.NAN:
            p = KE.statement(item)
            assert math.isnan(p) == (name in KE.NAN), (name, p)
            if name not in KE.NAN:
                assert 0.01 < p < 0.99, (name, p)                                 # a cap item that says something
    assert KE.same_bits([KE.statement(KE.SPECIAL["the cell cap"])], [KE.statement(KE.SPECIAL["the cell cap, swapped"])])
    assert ST.undefined(96, 1 << 20, 3) and not ST.undefined(95, 1 << 20, 3)      # 96 * 2^20 > 10^8 >= 95 * 2^20
    assert ST.undefined(1, 10 ** 8 + 1, 3) and not ST.undefined(1, 10 ** 8, 3) and not ST.undefined(10 ** 8, 1, 0)
    sub, zero = KE.statement(KE.SPECIAL["a subnormal result"]), KE.statement(KE.SPECIAL["a zero result"])
    assert 0.0 < sub < 2.0 ** -1022 and zero == 0.0             # 2 / C(2 n, n): about 1e-312 at n = 520, below the smallest subnormal at 600
