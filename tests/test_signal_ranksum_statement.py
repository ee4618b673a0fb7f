"""tests/signal_ranksum_statement.py -- the rank-sum test on the nine columns of X behind m6a_site_signal_ranksum and
`eventalign_diff --signal` -- is scipy's two-sided Mann-Whitney U test per column and tests/ranksum_statement.py's site_ranksum on each
de-interleaved column; the cases hold what they are named for; and m6anet_amd/ranksum.py's signal_text writes nine rows per pair with
one Benjamini-Hochberg family over all of them.

The bounds against scipy are those of tests/test_ranksum_statement.py: U1 is an integer and must agree exactly, p to relative 1e-10
(both sides evaluate one formula in doubles, a few roundings apart)."""
import math

import numpy as np
import pytest

import ranksum_statement as RS
import signal_ranksum_cases as SC
import signal_ranksum_statement as SS
from m6anet_amd import ranksum

f32 = np.float32


def test_statement_against_scipy_per_column():
    stats = pytest.importorskip("scipy.stats")
    Xa, oa, Xb, ob, _ = SC.sets()
    small = [k for k in range(SC.n_sites()) if 0 < oa[k + 1] - oa[k] <= 130 and 0 < ob[k + 1] - ob[k] <= 130]
    worst, seen = 0.0, 0
    for i in small:
        for j in small[::3]:
            A, B = Xa[oa[i]:oa[i + 1]], Xb[ob[j]:ob[j + 1]]
            for c, (gt, eq, tie, z) in enumerate(SS.pair(A, B)):
                if gt < 0:                                        # a NaN in this column: undefined, and scipy has no answer
                    assert np.isnan(A[:, c]).any() or np.isnan(B[:, c]).any()
                    continue
                r = stats.mannwhitneyu(A[:, c].astype(np.float64), B[:, c].astype(np.float64), use_continuity=True, alternative="two-sided",
                                       method="asymptotic")
                assert 2 * gt + eq == 2 * r.statistic             # U1, exactly
                p = float(ranksum.p_value(np.array([z]))[0])
                if z == 0:                                        # |d| <= 0.5 (all pooled values equal among them): p = 1, as scipy has it
                    assert p == 1.0 and abs(r.pvalue - 1.0) <= 1e-10
                else:
                    rel = abs(p - r.pvalue) / r.pvalue
                    worst = max(worst, rel)
                    assert rel <= 1e-10, (i, j, c, p, r.pvalue)
                seen += 1
    print("largest relative difference in p: %.3g over %d columns" % (worst, seen))
    assert seen > 9 * 100


def test_statement_is_site_ranksum_on_each_column():
    Xa, oa, Xb, ob, _ = SC.sets()
    ia, ib = SC.pair_lists()["65 drawn"]
    got = SS.site_signal_ranksum(Xa, oa, Xb, ob, ia, ib)
    for c in range(9):
        col = RS.site_ranksum(np.ascontiguousarray(Xa[:, c]), oa, np.ascontiguousarray(Xb[:, c]), ob, ia, ib)
        for g, w in zip(got, col):
            assert SC.same_bits(np.ascontiguousarray(g[:, c]), w), c
    assert all(SC.same_bits(g, w) for g, w in zip(got, SC.want(ia, ib)))
    assert all(SC.same_bits(g, w) for g, w in zip(SS.site_signal_ranksum(Xa, oa, Xb, ob), SC.want()))


def test_the_cases_hold_what_they_are_named_for():
    _, oa, _, ob, names = SC.sets()
    gt, eq, tie, z = SC.want()
    K = len(SC.SIZES)
    undefined = (gt == -1) & (eq == -1) & (tie == -1) & np.isnan(z)
    assert ((gt == -1) == undefined).all() and (np.isnan(z) == undefined).all()
    assert not undefined[:K].any()
    expect = {"nan in column 4 of a": [4], "nan in column 8 of b": [8], "nan in every column": range(9), "empty a": range(9), "empty b": range(9),
              "both empty": range(9)}
    for k, name in enumerate(names):
        assert np.flatnonzero(undefined[K + k]).tolist() == list(expect.get(name, [])), name
    for k in range(SC.n_sites()):                                # the column families: all equal, and a negation
        if not undefined[k].any():
            n, m = int(oa[k + 1] - oa[k]), int(ob[k + 1] - ob[k])
            assert (gt[k, 3], eq[k, 3], tie[k, 3], z[k, 3]) == (0, n * m, (n + m) ** 3 - (n + m), 0.0)
            assert gt[k, 5] == n * m - gt[k, 4] - eq[k, 4] and eq[k, 5] == eq[k, 4] and tie[k, 5] == tie[k, 4] and z[k, 5] == -z[k, 4]
    assert len({(int(gt[K - 1, c]), float(z[K - 1, c])) for c in range(9)}) == 9      # no two columns alike
    k = K + names.index("signed zeros in column 2")
    assert (gt[k, 2], eq[k, 2]) == (2, 6)
    k = K + names.index("infinities in column 6")
    assert (gt[k, 6], eq[k, 6]) == (2 * 2 + 1, 2 + 1)            # each +inf of a above 0.25 and 0.5 and equal to b's; 0.5 above 0.25, equal to 0.5
    k = K + names.index("complete separation in column 1")
    assert (gt[k, 1], eq[k, 1], tie[k, 1]) == (30 * 25, 0, 0) and z[k, 1] > 6 and (np.delete(gt[k], 1) < 30 * 25).all()


def test_signal_text():
    gt = np.array([[5, 4, 3, 2, 1, 0, 6, 5, -1], [0] * 9])
    eq = np.array([[1, 0, 0, 0, 0, 0, 0, 1, -1], [12] * 9])
    z = np.array([[1.5, 0.75, 0.0, -0.25, -1.0, -2.0, 2.5, 1.5, np.nan], [0.0] * 9])
    text = ranksum.signal_text(["tx", "ty"], [7, 9], ["GGACT", "AAACA"], [3, 4], [2, 3], gt, eq, z)
    lines = text.splitlines()
    assert text.endswith("\n") and lines[0] == ranksum.SIGNAL_HEADER and len(lines) == 1 + 2 * 9
    assert ranksum.SIGNAL_HEADER == "transcript_id,transcript_position,kmer,n_reads_a,n_reads_b,position_offset,feature,auc,z,p_value,q_value"
    assert ranksum.SIGNAL_FILE == "data.diff_signal.csv"
    rows = [ln.split(",") for ln in lines[1:]]
    assert [r[:5] for r in rows] == [["tx", "7", "GGACT", "3", "2"]] * 9 + [["ty", "9", "AAACA", "4", "3"]] * 9
    assert [(r[5], r[6]) for r in rows[:9]] == [(o, f) for o in ("-1", "0", "1") for f in ("dwell_time", "norm_std", "norm_mean")]
    assert [(r[5], r[6]) for r in rows[9:]] == [(r[5], r[6]) for r in rows[:9]]
    p = [float("nan") if math.isnan(v) else math.erfc(abs(v) / math.sqrt(2.0)) for v in z.ravel()]
    q = ranksum.bh(np.array(p))                                  # one family: the 17 rows with a p, of both sites
    assert rows[8][7:] == ["nan"] * 4 and math.isnan(q[8])
    keep = [k for k in range(18) if k != 8]
    order = sorted(keep, key=lambda k: p[k])
    assert q[order[0]] == min(p[k] * 17 / (r + 1) for r, k in enumerate(order))      # the smallest p of the family: p M / rank, M = 17, then the running minimum
    for k in keep:
        U = (2 * int(gt.ravel()[k]) + int(eq.ravel()[k])) / 2
        nm = 6 if k < 9 else 12
        assert rows[k][7:] == [repr(U / nm), repr(float(z.ravel()[k])), repr(p[k]), repr(float(q[k]))]
    assert rows[0][7:9] == [repr(5.5 / 6), "1.5"] and rows[9][7:] == ["0.5", "0.0", "1.0", "1.0"]
    assert ranksum.signal_text([], [], [], [], [], np.zeros((0, 9), np.int64), np.zeros((0, 9), np.int64), np.zeros((0, 9))) == ranksum.SIGNAL_HEADER + "\n"
