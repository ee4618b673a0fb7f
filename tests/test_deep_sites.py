"""The references of tests/test_gpu_deep_sites.py, and the host cores, on the shapes of tests/deep_site_cases.py: bags of more than
2^16 reads and pairs whose counts pass 2^32.  No GPU.

  * the scalar pairs and the nine-column pair hold the size conditions that give the GPU tests their teeth (a count, a tie sum and
    m A - n B above 2^32, a tie group above 2^16), stated here so that the inputs cannot drift below them;
  * the statements give the closed forms where there are any (n m, N^3 - N, the medians) and agree with scipy under the bounds of
    tests/test_ranksum_statement.py and tests/test_ks_statement.py: U1 exactly, the tie correction to 1e-12, p to relative 1e-10, D to
    2^-52, the medians np.median's;
  * the host cores (m6a_ranksum.h `count`, m6a_ks.h, through libm6a_io.so as tests/test_ranksum_core.py, tests/test_ks_core.py and
    tests/test_signal_ranksum_core.py reach them) give the statements' bits there, and on a pair of 2^20 pooled reads (the largest
    defined one) and of 2^20 + 1 (undefined);
  * the oracle's pooling is the NumPy statement (tests/test_oracle_golden.py: np_pool_one_group) on edge_probs of the bags BIG;
  * tests/site_expectation_statement.py is the math.fsum formula within 1e-14 on bags of up to 131 073 reads."""
import math

import numpy as np
import pytest

import deep_site_cases as D
import ranksum_statement as RS
import site_expectation_statement as SE
from m6anet_amd import ranksum
from oracle import m6a_oracle as orc
from test_ks_core import call as ks_core
from test_oracle_golden import THR, edge_probs, np_pool_one_group
from test_ranksum_core import call as ranksum_core
from test_signal_ranksum_core import call as signal_ranksum_core
from test_site_expectation_statement import exact

NM = D.N_A * D.N_B
POOLED = D.N_A + D.N_B


def test_the_scalar_pairs_cross_what_they_are_there_to_cross():
    assert NM > 2 ** 32 and 2 ** 16 < POOLED < RS.MAX_POOLED
    gt, eq, tie, z = D.scalar_ranksum_want()
    d_pos, d_neg, med_a, med_b = D.scalar_ks_want()
    name = D.NAMES.index
    k = name("separated")
    assert gt[k] == NM > 2 ** 32 and eq[k] == 0 and z[k] > 300                      # gt above 2^32
    assert (d_pos[k], d_neg[k]) == (0, NM)                                          # d_neg above 2^32
    k = name("separated, swapped")
    assert (gt[k], eq[k]) == (0, 0) and z[k] == -z[name("separated")]
    assert (d_pos[k], d_neg[k]) == (NM, 0)                                          # d_pos above 2^32, in another pair
    for k in (name("all equal"), name("all equal, swapped")):
        assert (gt[k], eq[k], tie[k]) == (0, NM, POOLED ** 3 - POOLED)              # eq above 2^32, tie far above it
        assert tie[k] == 2299967999868000 and z[k] == 0 and not np.signbit(z[k])
        assert (d_pos[k], d_neg[k], med_a[k], med_b[k]) == (0, 0, 0.5, 0.5)
    (a, b), (c, d) = D.scalar_pairs()[1], D.scalar_pairs()[2]
    assert D.largest_tie_group(a, b) == POOLED > 2 ** 16                            # a tie group whose square leaves 32 bits
    assert 2 ** 14 < D.largest_tie_group(c, d) < 2 ** 16
    k, s = name("four values"), name("four values, swapped")
    assert tie[k] == tie[s] > 2 ** 32 and eq[k] == eq[s] > 2 ** 29                  # tie above 2^32 in a second pair
    assert gt[k] > 2 ** 30 and gt[k] + gt[s] + eq[k] == NM                          # every (a_i, b_j) is above, below or equal
    assert (d_pos[k], d_neg[k]) == (d_neg[s], d_pos[s]) and (med_a[k], med_b[k]) == (med_b[s], med_a[s])
    sep_a, sep_b = D.scalar_pairs()[0]
    k = name("separated")
    assert (med_a[k], med_b[k]) == (np.median(sep_a.astype(np.float64)), np.median(sep_b.astype(np.float64)))
    assert sep_b.max() < sep_a.min()


def test_the_signal_pair_crosses_them_in_its_columns():
    n, m = D.SIGNAL_ROWS
    Xa, oa, Xb, ob = D.signal_sets()
    assert Xa.shape == (n, 9) and Xb.shape == (m, 9) and n * m > 2 ** 30 and n + m > 2 ** 16
    gt, eq, tie, z = (x[0] for x in D.signal_ranksum_want())
    d_pos, d_neg, med_a, med_b = (x[0] for x in D.signal_ks_want())
    assert np.flatnonzero(np.isnan(Xa).any(axis=0)).tolist() == [2] and np.isnan(Xa).sum() == 1 and not np.isnan(Xb).any()
    assert np.flatnonzero(gt == -1).tolist() == [2] and np.flatnonzero(d_pos == -1).tolist() == [2]     # the NaN's column alone is undefined
    assert eq[2] == tie[2] == d_neg[2] == -1 and np.isnan([z[2], med_a[2], med_b[2]]).all()
    assert (gt[0], eq[0], d_pos[0], d_neg[0]) == (n * m, 0, 0, n * m)                                   # separated, in column 0
    assert (gt[4], eq[4], tie[4], z[4]) == (0, n * m, (n + m) ** 3 - (n + m), 0.0) and (d_pos[4], d_neg[4]) == (0, 0)   # all equal, in column 4
    assert D.largest_tie_group(Xa[:, 4], Xb[:, 4]) == n + m > 2 ** 16
    assert tie[8] > 2 ** 32 and eq[8] > 2 ** 27 and gt[8] > 2 ** 28                                     # four values, in column 8


def test_statements_against_scipy():
    stats = pytest.importorskip("scipy.stats")
    gt, eq, tie, z = D.scalar_ranksum_want()
    d_pos, d_neg, med_a, med_b = D.scalar_ks_want()
    va, oa, vb, ob = D.scalar_sets()
    for k, name in enumerate(D.NAMES):
        a, b = va[oa[k]:oa[k + 1]].astype(np.float64), vb[ob[k]:ob[k + 1]].astype(np.float64)
        n, m = a.size, b.size
        r = stats.mannwhitneyu(a, b, use_continuity=True, alternative="two-sided", method="asymptotic")
        assert 2 * int(gt[k]) + int(eq[k]) == 2 * r.statistic, name                  # U1, exactly
        N = n + m
        assert abs((1 - int(tie[k]) / (N ** 3 - N)) - stats.tiecorrect(stats.rankdata(np.concatenate([a, b])))) <= 1e-12, name
        p = float(ranksum.p_value(z[k:k + 1])[0])
        if "all equal" in name:                                   # no variance left: scipy divides 0 by 0 where the statement says z = 0, p = 1
            assert p == 1.0
        elif r.pvalue > 0:
            assert abs(p - r.pvalue) <= 1e-10 * r.pvalue, (name, p, r.pvalue)
        else:
            assert p == 0 and "separated" in name                 # |z| = 314: both underflow
        d = float(ranksum.ks_d(d_pos[k:k + 1], d_neg[k:k + 1], [n], [m])[0])
        s = stats.ks_2samp(a, b, method="asymp")
        assert abs(d - s.statistic) <= 2.0 ** -52, (name, d, s.statistic)
        assert (med_a[k], med_b[k]) == (np.median(a), np.median(b)), name
        p, sf = float(ranksum.ks_p_value([d], [n], [m])[0]), float(stats.kstwobign.sf(ranksum.ks_lambda(d, n, m)))
        assert 0.0 <= p <= 1.0
        if sf >= 1e-300:
            assert abs(p - sf) <= 1e-10 * sf, (name, p, sf)


@pytest.mark.parametrize("n_threads", [1, 4])
def test_host_cores_give_the_statements_on_the_scalar_pairs(n_threads):
    va, oa, vb, ob = D.scalar_sets()
    rc, *got = ranksum_core(va, oa, vb, ob, None, None, len(D.NAMES), n_threads=n_threads)
    assert rc == 0
    for g, w, what in zip(got, D.scalar_ranksum_want(), ("gt", "eq", "tie", "z")):
        assert D.same_bits(g, w), (what, g, w)
    rc, *got = ks_core("scalar", va, oa, vb, ob, None, None, len(D.NAMES), n_threads=n_threads)
    assert rc == 0
    for g, w, what in zip(got, D.scalar_ks_want(), ("d_pos", "d_neg", "med_a", "med_b")):
        assert D.same_bits(g, w), (what, g, w)


def test_host_cores_give_the_statements_on_the_signal_pair():
    Xa, oa, Xb, ob = D.signal_sets()
    rc, *got = signal_ranksum_core(Xa, oa, Xb, ob, None, None, 1)
    assert rc == 0
    for g, w, what in zip(got, D.signal_ranksum_want(), ("gt", "eq", "tie", "z")):
        assert D.same_bits(g, w), (what, g, w)
    rc, *got = ks_core("signal", Xa, oa, Xb, ob, None, None, 1)
    assert rc == 0
    for g, w, what in zip(got, D.signal_ks_want(), ("d_pos", "d_neg", "med_a", "med_b")):
        assert D.same_bits(g, w), (what, g, w)


@pytest.mark.parametrize("pooled,defined", [(RS.MAX_POOLED, True), (RS.MAX_POOLED + 1, False)])
def test_host_cores_at_the_largest_defined_pair_and_one_read_past_it(pooled, defined):
    va, oa, vb, ob = D.limit_sets(pooled)
    assert (oa[1] - oa[0]) + (ob[1] - ob[0]) == pooled
    want_rs, want_ks = D.limit_want(pooled)
    assert (want_rs[0][0] >= 0) == defined and (want_ks[0][0] >= 0) == defined and want_rs[0][1] >= 0 and want_ks[0][1] >= 0
    if not defined:
        assert [int(w[0]) for w in want_rs[:3]] == [-1, -1, -1] and np.isnan(want_rs[3][0])
        assert [int(w[0]) for w in want_ks[:2]] == [-1, -1] and np.isnan(want_ks[2][0]) and np.isnan(want_ks[3][0])
    rc, *got = ranksum_core(va, oa, vb, ob, None, None, 2)
    assert rc == 0 and all(D.same_bits(g, w) for g, w in zip(got, want_rs)), (got, want_rs)
    rc, *got = ks_core("scalar", va, oa, vb, ob, None, None, 2)
    assert rc == 0 and all(D.same_bits(g, w) for g, w in zip(got, want_ks)), (got, want_ks)


@pytest.mark.parametrize("T", [7, 100])
def test_oracle_pooling_is_the_numpy_statement_on_the_big_bags(T):
    p, off = edge_probs(D.BIG, D.SEED)
    site, mod = orc.site_pool(p, off, T, THR, seed=D.SEED, save_per_batch=1)
    want_site, want_mod = np_pool_one_group(p, off, T, THR, D.SEED)
    assert np.array_equal(site, want_site, equal_nan=True)
    assert np.array_equal(mod, want_mod)
    assert np.isnan(want_site).any() and not np.isnan(want_site).all()


@pytest.mark.parametrize("K", [20, 64])
def test_expectation_statement_is_the_fsum_formula_on_the_big_bags(K):
    """site_prob before its rounding to float32 and mc_sigma against math.fsum and Python powers: 1e-14 absolute, the bound of
    tests/test_site_expectation_statement.py"""
    rng = np.random.default_rng(D.SEED)
    off = D.csr(D.EXPECTATION_BAGS)
    p = RS_probs(rng, int(off[-1]))
    site, sigma, _ = SE.site_expectation(p, off, K)
    for s in range(off.size - 1):
        bag = p[off[s]:off[s + 1]]
        e_site, e_sigma = exact(bag, K)
        e64, g64 = SE.expectation_f64(bag[None, :], K)
        assert site[s] == np.float32(e64[0]) and sigma[s] == g64[0], s
        assert abs(float(e64[0]) - e_site) <= 1e-14 and abs(float(g64[0]) - e_sigma) <= 1e-14, (s, float(e64[0]) - e_site, float(g64[0]) - e_sigma)
    assert math.isfinite(float(sigma.max()))


def RS_probs(rng, n):
    return D.RC.probs(rng, n)
