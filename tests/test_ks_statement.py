"""tests/ks_statement.py -- the Kolmogorov-Smirnov integers and the medians behind m6a_site_ks, m6a_site_signal_ks and `eventalign_diff
--ks` -- and what m6anet_amd/ranksum.py derives from them, held to scipy and NumPy:
  D        max(d_pos, d_neg) / (n m) is within 2^-52 of scipy.stats.ks_2samp(...).statistic (scipy subtracts two rounded quotients)
  p        within relative 1e-10 of scipy.stats.kstwobign.sf(lambda) wherever that is >= 1e-300, the bound tests/test_ranksum_statement.py
           uses for its p: both sides evaluate a rapidly converging series in doubles.  It is the Kolmogorov limit, not ks_2samp's p;
           the largest gap to ks_2samp(method="exact") on the bags of at most 65 reads is printed, with no bar
  medians  equal np.median in float64
  q        Benjamini-Hochberg by the existing ranksum.bh
and the cases of tests/ks_cases.py hold what they are named for."""
import math

import numpy as np
import pytest

import ks_cases as KC
import ks_statement as KS
import ranksum_statement as RS
from m6anet_amd import ranksum

f32 = np.float32


def defined_pairs():
    """(a, b) float32 bags: every defined (special pair, column) of the signal sets, every defined special pair of the scalar sets, and
    sized sites of both crossed"""
    out = []
    for cases in (KC.scalar, KC.signal):
        va, oa, vb, ob, _ = cases.sets()
        K = len(cases.base.SIZES)
        va, vb = va.reshape(-1, cases.columns), vb.reshape(-1, cases.columns)
        sites = [(k, k) for k in range(K, cases.n_sites())] + [(i, j) for i in range(0, K, 2) for j in range(1, K, 3)]
        for i, j in sites:
            for c in range(cases.columns):
                a, b = va[oa[i]:oa[i + 1], c], vb[ob[j]:ob[j + 1], c]
                if a.size and b.size and not np.isnan(a).any() and not np.isnan(b).any():
                    out.append((a, b))
    return out


def test_statement_against_scipy():
    stats = pytest.importorskip("scipy.stats")
    pairs = defined_pairs()
    assert len(pairs) > 97
    worst_d = worst_p = worst_exact = 0.0
    for a, b in pairs:
        d_pos, d_neg, med_a, med_b = KS.pair(a, b)
        n, m = a.size, b.size
        assert 0 <= d_pos <= n * m and 0 <= d_neg <= n * m
        a64, b64 = a.astype(np.float64), b.astype(np.float64)
        finite = np.isfinite(a64).all() and np.isfinite(b64).all()
        d = float(ranksum.ks_d([d_pos], [d_neg], [n], [m])[0])
        r = stats.ks_2samp(a64, b64, method="asymp")                   # (infinities are ordinary values there too)
        worst_d = max(worst_d, abs(d - r.statistic))
        assert abs(d - r.statistic) <= 2.0 ** -52, (n, m, d, r.statistic)
        for med, x in ((med_a, a64), (med_b, b64)):
            with np.errstate(invalid="ignore"):
                w = float(np.median(x))
            assert (math.isnan(med) and math.isnan(w)) or med == w, (med, w)
            assert not (med == 0 and np.signbit(med))
        lam = ranksum.ks_lambda(d, n, m)
        assert lam == math.sqrt(float(n) * float(m) / float(n + m)) * d
        p, sf = float(ranksum.ks_p_value([d], [n], [m])[0]), float(stats.kstwobign.sf(lam))
        assert 0.0 <= p <= 1.0
        if sf >= 1e-300:
            worst_p = max(worst_p, abs(p - sf) / sf)
            assert abs(p - sf) <= 1e-10 * sf, (n, m, lam, p, sf)
        if finite and max(n, m) <= 65:
            worst_exact = max(worst_exact, abs(p - stats.ks_2samp(a64, b64, method="exact").pvalue))
    print("largest |D - ks_2samp statistic| %.3g, largest relative difference in p to kstwobign.sf %.3g, largest |p - ks_2samp exact p| on "
          "bags of at most 65 reads %.3g (no bar), over %d pairs" % (worst_d, worst_p, worst_exact, len(pairs)))


def test_p_value_series_against_scipy_over_lambda():
    stats = pytest.importorskip("scipy.stats")
    worst = 0.0
    for lam in np.concatenate([np.linspace(0.01, 8.0, 4001), ranksum.KS_SWITCH + np.array([-1e-9, 0.0, 1e-9]), [12.0, 18.5, 26.0]]).tolist():
        sf = float(stats.kstwobign.sf(lam))
        p = ranksum.kolmogorov_sf(lam)
        assert 0.0 <= p <= 1.0
        if sf >= 1e-300:
            worst = max(worst, abs(p - sf) / sf)
            assert abs(p - sf) <= 1e-10 * sf, (lam, p, sf)
    print("largest relative difference to kstwobign.sf: %.3g" % worst)
    assert ranksum.kolmogorov_sf(0.0) == 1.0 and ranksum.kolmogorov_sf(1e-3) == 1.0 and math.isnan(ranksum.kolmogorov_sf(float("nan")))
    assert ranksum.kolmogorov_sf(40.0) == 0.0


def test_tables_and_sorted_copies_count_the_same():
    rng = np.random.default_rng(3303)
    for n, m in ((1, 1), (5, 4), (64, 65), (300, 257)):
        for draw in (RC_probs, RC_four):
            a, b = draw(rng, n), draw(rng, m)
            assert KS.d_by_table(a, b) == KS.d_by_sort(a, b)
    big_a, big_b = RC_probs(rng, 4000), RC_four(rng, 3000)
    assert KS.pair(big_a, big_b)[:2] == KS.d_by_sort(big_a, big_b)                 # past the table limit


def RC_probs(rng, n):
    return KC.RC.probs(rng, n)


def RC_four(rng, n):
    return KC.RC.four(rng, n)


def test_the_new_cases_hold_what_they_are_named_for():
    c = KC.scalar
    d_pos, d_neg, med_a, med_b = c.want()
    va, oa, vb, ob, names = c.sets()
    undefined = (d_pos == -1) & (d_neg == -1) & np.isnan(med_a) & np.isnan(med_b)
    assert ((d_pos == -1) == undefined).all() and ((d_neg == -1) == undefined).all()
    K = len(KC.RC.SIZES)
    assert not undefined[:K].any()
    for k, name in enumerate(names):
        assert undefined[K + k] == name.startswith(("empty", "both empty", "nan")), name
    k = c.site_of("bimodal against unimodal")
    a, b = va[oa[k]:oa[k + 1]], vb[ob[k]:ob[k + 1]]
    assert (a.size, b.size) == (60, 61) and med_a[k] == med_b[k] == 0.5               # an even and an odd bag, equal medians
    assert abs(RS.pair(a, b)[3]) < 1                                                # the rank-sum sees nothing ...
    d = ranksum.ks_d(d_pos[k:k + 1], d_neg[k:k + 1], [60], [61])[0]
    assert d > 0.3 and d == 0.5 and ranksum.ks_p_value([d], [60], [61])[0] < 1e-6   # ... where half of a lies below all of b
    k = c.site_of("odd and even")
    assert (med_a[k], med_b[k]) == (0.5, 0.375)
    k = c.site_of("zero middles")
    assert med_a[k] == 0 and med_b[k] == 0 and not np.signbit(med_a[k]) and not np.signbit(med_b[k])
    k = c.site_of("infinite middles")
    assert d_pos[k] >= 0 and math.isnan(med_a[k]) and med_b[k] == 0.5               # a defined pair whose median is NaN, as np.median's
    k = c.site_of("all equal")
    assert (d_pos[k], d_neg[k]) == (0, 0) and ranksum.ks_p_value([0.0], [70], [33])[0] == 1.0
    k = c.site_of("complete separation")                                             # all of b lies below all of a: B's CDF above
    assert (d_pos[k], d_neg[k]) == (0, 30 * 25) and ranksum.ks_sign(d_pos[k:k + 1], d_neg[k:k + 1])[0] == -1
    k = c.site_of("signed zeros")                                                    # a: -0 0 -0 .25; b: 0 -0 .5 -- at 0: 3 m - 2 n = 1
    assert (d_pos[k], d_neg[k]) == (4, 0) and med_a[k] == 0 and not np.signbit(med_a[k])


def test_signal_statement_is_the_statement_on_each_column():
    c = KC.signal
    Xa, oa, Xb, ob, names = c.sets()
    ia, ib = c.pair_lists()["65 drawn"]
    got = KS.site_signal_ks(Xa, oa, Xb, ob, ia, ib)
    for col in range(9):
        one = KS.site_ks(np.ascontiguousarray(Xa[:, col]), oa, np.ascontiguousarray(Xb[:, col]), ob, ia, ib)
        for g, w in zip(got, one):
            assert KC.same_bits(np.ascontiguousarray(g[:, col]), w), col
    assert all(KC.same_bits(g, w) for g, w in zip(got, c.want(ia, ib)))
    d_pos, d_neg, med_a, med_b = c.want()
    undefined = d_pos == -1
    expect = {"nan in column 4 of a": [4], "nan in column 8 of b": [8], "nan in every column": range(9), "empty a": range(9), "empty b": range(9),
              "both empty": range(9)}
    K = len(KC.SC.SIZES)
    for k, name in enumerate(names):
        assert np.flatnonzero(undefined[K + k]).tolist() == list(expect.get(name, [])), name
    k = c.site_of("bimodal against unimodal in column 8")
    assert med_a[k, 8] == med_b[k, 8] == 0.5 and d_pos[k, 8] == 30 * 61
    k = c.site_of("zero middles in column 0")
    assert med_a[k, 0] == 0 and not np.signbit(med_a[k, 0]) and not np.signbit(med_b[k, 0])
    k = c.site_of("infinite middles in column 6")
    assert math.isnan(med_a[k, 6]) and d_pos[k, 6] >= 0 and not np.isnan(np.delete(med_a[k], 6)).any()


def test_ks_text():
    d_pos = np.array([6, 0, -1, 2])
    d_neg = np.array([0, 6, -1, 2])
    med_a = np.array([0.25, 0.5, np.nan, np.nan])
    med_b = np.array([0.5, 0.25, np.nan, 1.0])
    n_a, n_b = [3, 2, 0, 2], [2, 3, 4, 2]
    text = ranksum.ks_text(["tx", "tx", "ty", "tz"], [7, 9, 3, 4], ["GGACT", "AAACA", "GGACA", "TGACT"], n_a, n_b, d_pos, d_neg, med_a, med_b)
    lines = text.splitlines()
    assert text.endswith("\n") and lines[0] == ranksum.KS_HEADER and len(lines) == 5
    assert ranksum.KS_HEADER == "transcript_id,transcript_position,kmer,n_reads_a,n_reads_b,median_a,median_b,median_shift,ks_d,ks_sign,p_value,q_value"
    assert (ranksum.KS_FILE, ranksum.SIGNAL_KS_FILE) == ("data.diff_ks.csv", "data.diff_signal_ks.csv")
    rows = [ln.split(",") for ln in lines[1:]]
    p = [ranksum.kolmogorov_sf(math.sqrt(6 / 5) * 1.0), ranksum.kolmogorov_sf(math.sqrt(6 / 5) * 1.0), float("nan"), ranksum.kolmogorov_sf(0.5)]
    q = ranksum.bh(np.array(p))                                                     # the existing Benjamini-Hochberg, over the three rows with a p
    assert rows[0] == ["tx", "7", "GGACT", "3", "2", "0.25", "0.5", "-0.25", "1.0", "1", repr(p[0]), repr(float(q[0]))]
    assert rows[1] == ["tx", "9", "AAACA", "2", "3", "0.5", "0.25", "0.25", "1.0", "-1", repr(p[1]), repr(float(q[1]))]
    assert rows[2] == ["ty", "3", "GGACA", "0", "4"] + ["nan"] * 7                   # an undefined pair
    assert rows[3] == ["tz", "4", "TGACT", "2", "2", "nan", "1.0", "nan", "0.5", "1", repr(p[3]), repr(float(q[3]))]   # d_pos == d_neg: +1
    assert q[0] == min(1.0, p[0] * 3 / 2) and math.isnan(q[2])
    assert ranksum.ks_text([], [], [], [], [], [], [], [], []) == ranksum.KS_HEADER + "\n"


def test_signal_ks_text():
    rng = np.random.default_rng(3304)
    d_pos, d_neg = rng.integers(0, 7, (2, 9)), rng.integers(0, 7, (2, 9))
    d_pos[1, 4] = d_neg[1, 4] = -1
    med_a, med_b = rng.normal(size=(2, 9)), rng.normal(size=(2, 9))
    med_a[1, 4] = med_b[1, 4] = np.nan
    text = ranksum.signal_ks_text(["tx", "ty"], [7, 9], ["GGACT", "AAACA"], [3, 2], [2, 3], d_pos, d_neg, med_a, med_b)
    lines = text.splitlines()
    assert text.endswith("\n") and lines[0] == ranksum.SIGNAL_KS_HEADER and len(lines) == 1 + 18
    assert ranksum.SIGNAL_KS_HEADER == ("transcript_id,transcript_position,kmer,n_reads_a,n_reads_b,position_offset,feature,median_a,median_b,"
                                        "median_shift,ks_d,ks_sign,p_value,q_value")
    rows = [ln.split(",") for ln in lines[1:]]
    assert [r[:5] for r in rows] == [["tx", "7", "GGACT", "3", "2"]] * 9 + [["ty", "9", "AAACA", "2", "3"]] * 9
    assert [(r[5], r[6]) for r in rows] == [(o, f) for o in ("-1", "0", "1") for f in ("dwell_time", "norm_std", "norm_mean")] * 2
    d = np.maximum(d_pos, d_neg).ravel() / 6.0
    p = np.array([float("nan") if v < 0 else ranksum.kolmogorov_sf(math.sqrt(6 / 5) * v) for v in d.tolist()])
    q = ranksum.bh(p)                                                               # one family: the 17 rows with a p, of both sites
    for k, r in enumerate(rows):
        if k == 13:
            assert r[7:] == ["nan"] * 7
            continue
        a, b = float(med_a.ravel()[k]), float(med_b.ravel()[k])
        assert r[7:] == [repr(a), repr(b), repr(a - b), repr(float(d[k])), "1" if d_pos.ravel()[k] >= d_neg.ravel()[k] else "-1", repr(float(p[k])),
                         repr(float(q[k]))]
    assert np.isnan(q[13]) and np.count_nonzero(~np.isnan(q)) == 17
