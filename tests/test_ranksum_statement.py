"""tests/ranksum_statement.py -- the rank-sum test behind m6a_site_ranksum and `eventalign_diff` -- is scipy's two-sided Mann-Whitney U
test (midranks, tie-corrected variance, continuity correction, normal approximation), and m6anet_amd/ranksum.py's p, q and join are what
they say; the command refuses its argument errors with exit status 2 before it writes anything.

The bounds against scipy: U1 and the tie term are integers and must agree exactly (the tie correction to 1e-12, scipy's being a double);
p to relative 1e-10 -- both sides evaluate the same formula in doubles, a few roundings apart (a few 1e-14 at worst on these families; the test prints it),
while a wrong continuity or tie correction is off by 1e-3 or more; q to 1e-12."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import ranksum_statement as RS
from m6anet_amd import ranksum

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def families(seed=2, per_family=1000):
    """seeded pairs with n, m in 1..69: heavy ties from four values, skewed uniforms, complete separation"""
    rng = np.random.default_rng(seed)
    for k in range(3 * per_family):
        n, m = (int(x) for x in rng.integers(1, 70, 2))
        kind = k % 3
        if kind == 0:
            yield rng.choice(np.array([0, 0.25, 0.5, 1], f32), n), rng.choice(np.array([0, 0.25, 0.5, 1], f32), m)
        elif kind == 1:
            yield (rng.random(n) ** 4).astype(f32), (rng.random(m) ** 2).astype(f32)
        else:                                                     # a above b, or b above a
            hi, lo = (0.5 + rng.random(n) * 0.4).astype(f32), (rng.random(m) * 0.4).astype(f32)
            yield (hi, lo) if k % 2 else (lo, hi)


def test_statement_against_scipy():
    stats = pytest.importorskip("scipy.stats")
    worst, ps = 0.0, []
    for a, b in families():
        n, m = a.size, b.size
        gt, eq, tie, z = RS.pair(a, b)
        r = stats.mannwhitneyu(a.astype(np.float64), b.astype(np.float64), use_continuity=True, alternative="two-sided", method="asymptotic")
        assert 2 * gt + eq == 2 * r.statistic                     # U1, exactly
        N = n + m
        assert abs((1 - tie / (N ** 3 - N)) - stats.tiecorrect(stats.rankdata(np.concatenate([a, b])))) <= 1e-12
        assert (gt, eq, tie) == RS.counts_by_sort(a, b)           # the two ways of counting agree
        p = float(ranksum.p_value(np.array([z]))[0])
        assert p > 0 and r.pvalue > 0                             # no underflow at these sizes: no case is left out
        rel = abs(p - r.pvalue) / r.pvalue
        worst = max(worst, rel)
        assert rel <= 1e-10, (n, m, p, r.pvalue)
        assert (z > 0) == (2 * gt + eq > n * m) or z == 0         # z > 0: the reads of a score higher
        ps.append(p)
    print("largest relative difference in p: %.3g" % worst)
    ps = np.array(ps)
    assert np.abs(ranksum.bh(ps) - stats.false_discovery_control(ps, method="bh")).max() <= 1e-12
    some = ps[:50].copy()                                          # NaN rows take no part and stay NaN
    some[::7] = np.nan
    q = ranksum.bh(some)
    keep = ~np.isnan(some)
    assert np.isnan(q[~keep]).all() and np.abs(q[keep] - stats.false_discovery_control(some[keep], method="bh")).max() <= 1e-12


def test_degenerate_pairs():
    assert RS.pair(np.full(5, 0.5, f32), np.full(9, 0.5, f32)) == (0, 45, 14 ** 3 - 14, 0.0)       # all pooled values equal: z = 0, p = 1
    assert ranksum.p_value(np.array([0.0, -0.0, np.nan])).tolist()[:2] == [1.0, 1.0] and math.isnan(ranksum.p_value(np.array([np.nan]))[0])
    for a, b in ((np.zeros(0, f32), np.ones(3, f32)), (np.ones(3, f32), np.zeros(0, f32)), (np.array([0.5, np.nan], f32), np.ones(3, f32)),
                 (np.ones(3, f32), np.array([np.nan], f32))):
        r = RS.pair(a, b)
        assert r[:3] == (-1, -1, -1) and math.isnan(r[3])
    gt, eq, tie, z = RS.pair(np.array([-0.0, 0.0], f32), np.array([0.0], f32))                     # -0.0 == 0.0
    assert (gt, eq, tie, z) == (0, 2, 24, 0.0)
    gt, eq, tie, z = RS.pair(np.array([np.inf, 1.0], f32), np.array([np.inf, -np.inf, -np.inf], f32))   # infinities are ordinary values
    assert (gt, eq, tie) == (4, 1, 12) and z > 0
    one = RS.pair(np.array([0.75], f32), np.array([0.25], f32))                                    # |d| = 0.5: the continuity correction takes all of it
    assert one[:3] == (1, 0, 0) and one[3] == 0 and not math.copysign(1, one[3]) < 0
    assert math.copysign(1, RS.pair(np.array([0.25], f32), np.array([0.75], f32))[3]) < 0          # ... and z keeps d's sign: -0.0
    auc = ranksum.auc(np.array([3, -1]), np.array([1, -1]), np.array([2, 0]), np.array([2, 5]))
    assert auc[0] == 3.5 / 4 and math.isnan(auc[1])


def test_bh_at_its_edges():
    assert ranksum.bh(np.zeros(0)).size == 0
    assert ranksum.bh(np.array([0.03])).tolist() == [0.03]
    assert np.isnan(ranksum.bh(np.array([np.nan, np.nan]))).all()
    q = ranksum.bh(np.array([0.01, np.nan, 0.04, 0.03, 0.9]))
    assert math.isnan(q[1]) and q[[0, 2, 3, 4]].tolist() == [0.01 * 4 / 1, min(0.04 * 4 / 3, 0.9), min(0.03 * 4 / 2, 0.04 * 4 / 3), 0.9]
    assert ranksum.bh(np.array([0.5, 0.5, 0.9])).tolist() == [0.75, 0.75, 0.9]                     # equal p: equal q
    assert ranksum.bh(np.array([0.9, 1.0])).tolist() == [1.0, 1.0]                                 # capped at 1


def test_join_at_its_edges():
    none = np.zeros(0, np.int64)
    for got in (ranksum.join([], [], [], []), ranksum.join(["t"], [5], [], []), ranksum.join([], [], ["t"], [5])):
        assert got[0].dtype == got[1].dtype == np.int64 and got[0].size == got[1].size == 0
    assert [x.tolist() for x in ranksum.join(["t"], [5], ["t"], [5])] == [[0], [0]]
    assert [x.tolist() for x in ranksum.join(["t"], [5], ["t"], [6])] == [none.tolist(), none.tolist()]
    # one transcript name at several positions, tables in different orders: an inner join in the order of the first table
    a = (["t1", "t1", "t2", "t1", "t3"], [10, 20, 10, 30, 10])
    b = (["t2", "t1", "t4", "t1"], [10, 30, 10, 10])
    pa, pb = ranksum.join(*a, *b)
    assert pa.tolist() == [0, 2, 3] and pb.tolist() == [3, 0, 1]
    pa, pb = ranksum.join(*b, *a)
    assert pa.tolist() == [0, 1, 3] and pb.tolist() == [2, 3, 0]
    pa, pb = ranksum.join(np.array([b"t", b"u"], object), np.array([1, 2]), np.array([b"u", b"t"], object), np.array([2, 1]))   # bytes and arrays
    assert pa.tolist() == [0, 1] and pb.tolist() == [1, 0]


def test_diff_text():
    rows = ranksum.diff_rows(["tx"] * 2, [7, 9], ["GGACT", "AAACA"], [3, 0], [2, 4], np.array([0.5, 0.25], f32), np.array([0.125, 1], f32),
                             np.array([1 / 3, 0.0]), np.array([0.5, 1.0]), np.array([5, -1]), np.array([1, -1]), np.array([1.5, np.nan]))
    p = math.erfc(1.5 / math.sqrt(2.0))
    assert rows[0] == "tx,7,GGACT,3,2,0.5000000000000000,0.1250000000000000,%.16f,0.5000000000000000,%r,1.5,%r,%r\n" % (1 / 3, 5.5 / 6, p, p)
    assert rows[1] == "tx,9,AAACA,0,4,0.2500000000000000,1.0000000000000000,0.0000000000000000,1.0000000000000000,nan,nan,nan,nan\n"
    assert ranksum.diff_text(*([[]] * 9), np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0)) == ranksum.DIFF_HEADER + "\n"


GOOD = ["--eventalign_a", "a.txt", "--eventalign_b", "b.txt"]


@pytest.mark.parametrize("argv", [
    ["--eventalign_b", "b.txt"],                                  # a condition without a file
    ["--eventalign_a", "--eventalign_b", "b.txt"],
    ["--eventalign_a", "a.txt", "--eventalign_b"],
    ["--eventalign_a", "-", "--eventalign_b", "-"],               # the standard input for both conditions
    ["--eventalign_a", "-", "a.txt", "-", "--eventalign_b", "b.txt"],
    GOOD + ["--num_iterations", "0"],
    GOOD + ["--num_iterations", "-3"],
    GOOD + ["--batch_size", "0"],
    GOOD + ["--save_per_batch", "0"],
    GOOD + ["--window_mb", "-1"],
    GOOD + ["--seed", "-1"],
    GOOD + ["--seed", str(2 ** 32)],
    GOOD + ["--readcount_min", "0"],
    GOOD + ["--device", "cpu"],
    GOOD + ["--site_proba", "exact"],
    GOOD + ["--drop_unflushed_tail"],                             # flags of eventalign_inference that this command does not take
    GOOD + ["--eventalign", "c.txt"],
    GOOD + ["--no_out_dir"],
])
def test_argument_errors_exit_2_and_write_nothing(tmp_path, argv):
    out = tmp_path / "out"
    tail = [] if argv[-1] == "--no_out_dir" else ["--out_dir", str(out)]
    r = subprocess.run([sys.executable, "-m", "m6anet_amd", "eventalign_diff"] + [a for a in argv if a != "--no_out_dir"] + tail, cwd=str(tmp_path), env=dict(os.environ, PYTHONPATH=REPO), capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 2, (r.returncode, r.stderr[-1500:])
    assert "error" in r.stderr and not out.exists() and os.listdir(str(tmp_path)) == []
