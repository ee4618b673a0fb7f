"""`eventalign_diff --ks` on the two small generated conditions of tests/test_gpu_eventalign_diff_signal.py, built again here by its
write_conditions.  With --ks, and with --signal --ks, OUT/a, OUT/b, data.diff.csv and data.diff_signal.csv keep the bytes of the run
without --ks; data.diff_ks.csv and data.diff_signal_ks.csv are the text m6anet_amd/ranksum.py writes from tests/ks_statement.py applied to
the two conditions taken here through prep_sites: X and off through inputs(), the read probabilities through infer_ptrs and fetch.  B's
reads of ENST0001.1's second site were generated with the current mean 118.25 at all three positions, so that site's three norm_mean rows
carry the three smallest p of the signal file, and A's median lies below B's there.  The same with --window_mb 1; the conditions swapped
leave ks_d and p_value alone to the digit, negate ks_sign except where d_pos == d_neg, and negate median_shift; without the flag neither
file is written."""
import os

import numpy as np
import pytest

import ks_statement as KS
import test_gpu_eventalign_diff_signal as DS
from m6anet_amd import _io, ranksum
from m6anet_amd.constants import N_SAMPLES, PRETRAINED_CONFIGS
from m6anet_amd.data_utils import load_norm_factors
from m6anet_amd.engine import M6ANetEngine

pytestmark = pytest.mark.gpu
ULP_BELOW = 1.0 - 2.0 ** -52                 # q = p M / rank is a product and a quotient, each rounded once: at rank M it may fall an ulp below p
SITES_LINE = "eventalign_diff: 3 sites in both conditions, 1 only in A, 2 only in B"


@pytest.fixture(scope="module")
def conditions(tmp_path_factory):
    return DS.write_conditions(tmp_path_factory.mktemp("diff_ks"))


@pytest.fixture(scope="module")
def tables(conditions, weights):
    """the two conditions through prep_sites: X, off, the site table, and the read probabilities of the command's inference"""
    thr, norm = PRETRAINED_CONFIGS[DS.MODEL][1], load_norm_factors(PRETRAINED_CONFIGS[DS.MODEL][2])
    out = {}
    eng = M6ANetEngine(weights=weights["hct116"], device=0)
    try:
        for c in "ab":
            files = conditions[c]
            with _io.prep_sites(files[0] if len(files) == 1 else files, 1, 1000, 1, norm=norm, n_threads=4) as s:
                X, _, off = s.inputs()
                i = s.info
                eng.set_host_offsets(s.off)
                eng.infer_ptrs(i.X, i.site_kmers, i.off, s.n_sites, 5, N_SAMPLES, thr, 0, 16, 2, i.read_prob, i.site_prob, i.mod_ratio)
                eng.sync()
                rp = s.fetch()[0]
                out[c] = dict(X=X, rp=rp, off=off, tx=[s.names[t] for t in s.site_tx], pos=s.tx_pos.copy(),
                              kmer=[bytes(k[1:6]).decode() for k in s.kmer7])
    finally:
        eng.close()
    return out


def expected(a, b, signal):
    pa, pb = ranksum.join(a["tx"], a["pos"], b["tx"], b["pos"])
    head = ([a["tx"][k] for k in pa], a["pos"][pa], [a["kmer"][k] for k in pa], np.diff(a["off"])[pa], np.diff(b["off"])[pb])
    if signal:
        return ranksum.signal_ks_text(*head, *KS.site_signal_ks(a["X"], a["off"], b["X"], b["off"], pa, pb))
    return ranksum.ks_text(*head, *KS.site_ks(a["rp"], a["off"], b["rp"], b["off"], pa, pb))


def read(d, fn):
    with open(os.path.join(d, fn), "rb") as f:
        return f.read()


def same_but_for(with_ks, without, added, shared):
    """the files of `shared` and OUT/a, OUT/b byte for byte; --ks adds the files of `added` and nothing else"""
    for fn in [os.path.join(c, f) for c in "ab" for f in DS.CSVS] + list(shared):
        assert read(with_ks, fn) == read(without, fn), fn
    assert sorted(os.listdir(with_ks)) == sorted(["a", "b"] + list(shared) + list(added))
    for c in "ab":
        assert sorted(os.listdir(os.path.join(with_ks, c))) == sorted(DS.CSVS)


def rows_of(d, fn):
    lines = read(d, fn).decode().splitlines()
    return lines[0], [ln.split(",") for ln in lines[1:]]


def test_outputs(conditions, tables):
    without, stdout0 = DS.diff(conditions, "signal", "a", "b", ["--signal"])
    assert sorted(os.listdir(without)) == ["a", "b", ranksum.DIFF_FILE, ranksum.SIGNAL_FILE]      # without the flag neither file exists
    only, stdout1 = DS.diff(conditions, "ks", "a", "b", ["--ks"])
    both, stdout2 = DS.diff(conditions, "signal_ks", "a", "b", ["--signal", "--ks"])
    assert stdout0 == stdout1 == stdout2 and stdout0.splitlines()[-1] == SITES_LINE
    same_but_for(only, without, [ranksum.KS_FILE], [ranksum.DIFF_FILE])
    same_but_for(both, without, [ranksum.KS_FILE, ranksum.SIGNAL_KS_FILE], [ranksum.DIFF_FILE, ranksum.SIGNAL_FILE])
    text = read(both, ranksum.KS_FILE).decode()
    assert text == expected(tables["a"], tables["b"], False) and read(only, ranksum.KS_FILE).decode() == text
    assert read(both, ranksum.SIGNAL_KS_FILE).decode() == expected(tables["a"], tables["b"], True)
    head, rows = rows_of(both, ranksum.KS_FILE)
    _, sites = rows_of(both, ranksum.DIFF_FILE)
    assert head == ranksum.KS_HEADER and [r[:5] for r in rows] == [s[:5] for s in sites] and len(rows) == 3
    for r in rows:
        ma, mb, shift, d, sign, p, q = (float(x) for x in r[5:])
        assert shift == ma - mb and 0 <= d <= 1 and sign in (1, -1) and 0 < p <= 1 and p * ULP_BELOW <= q <= 1 and 0 <= ma <= 1 and 0 <= mb <= 1
    head, rows = rows_of(both, ranksum.SIGNAL_KS_FILE)
    _, signal_rows = rows_of(both, ranksum.SIGNAL_FILE)
    assert head == ranksum.SIGNAL_KS_HEADER and [r[:7] for r in rows] == [s[:7] for s in signal_rows] and len(rows) == 27   # data.diff_signal.csv's order
    p = np.array([float(r[12]) for r in rows])
    q = np.array([float(r[13]) for r in rows])
    assert not np.isnan(p).any() and ((0 < p) & (p <= 1) & (p * ULP_BELOW <= q) & (q <= 1)).all()
    shifted = [k for k, r in enumerate(rows) if (r[0], int(r[1])) == DS.SHIFTED and r[6] == "norm_mean"]
    assert [rows[k][5] for k in shifted] == ["-1", "0", "1"]
    assert sorted(np.argsort(p, kind="stable")[:3].tolist()) == shifted and p[shifted].max() < np.delete(p, shifted).min()
    assert all(float(rows[k][9]) < 0 for k in shifted)                             # A's levels are drawn from 60..130, most below 118.25
    assert all(rows[k][11] == "1" for k in shifted)                                # ... so A's CDF lies above B's at the widest gap


def test_windows(conditions):
    plain, _ = DS.diff(conditions, "signal_ks", "a", "b", ["--signal", "--ks"])
    windows, stdout = DS.diff(conditions, "windows_signal_ks", "a", "b", ["--window_mb", "1", "--signal", "--ks"])
    assert stdout.splitlines()[-1] == SITES_LINE
    for fn in (ranksum.KS_FILE, ranksum.SIGNAL_KS_FILE, ranksum.DIFF_FILE, ranksum.SIGNAL_FILE):
        assert read(windows, fn) == read(plain, fn), fn


def test_conditions_swapped(conditions, tables):
    ab, _ = DS.diff(conditions, "signal_ks", "a", "b", ["--signal", "--ks"])
    ba, stdout = DS.diff(conditions, "swap_ba_signal_ks", "b", "a", ["--signal", "--ks"])
    assert stdout.splitlines()[-1] == "eventalign_diff: 3 sites in both conditions, 2 only in A, 1 only in B"
    for fn, key_columns, first, n in ((ranksum.KS_FILE, (0, 1, 2), 5, 3), (ranksum.SIGNAL_KS_FILE, (0, 1, 2, 5, 6), 7, 27)):
        assert read(ba, fn).decode() == expected(tables["b"], tables["a"], fn == ranksum.SIGNAL_KS_FILE)      # the statement, B against A
        rows_ab = {tuple(r[c] for c in key_columns): r for r in rows_of(ab, fn)[1]}
        rows_ba = {tuple(r[c] for c in key_columns): r for r in rows_of(ba, fn)[1]}
        assert sorted(rows_ab) == sorted(rows_ba) and len(rows_ab) == n
        for key, r in rows_ab.items():
            s = rows_ba[key]
            assert (r[3], r[4]) == (s[4], s[3])
            ma, mb, shift, d, sign, p, q = r[first:]
            assert (s[first], s[first + 1]) == (mb, ma)                           # the medians change places
            assert float(s[first + 2]) == -float(shift)                           # median_shift negated
            assert (s[first + 3], s[first + 5]) == (d, p)                         # ks_d and p_value unchanged, to the digit
            # ks_sign negated except where d_pos == d_neg, which is +1 both ways (the statement above decides which rows those are)
            assert int(s[first + 4]) == -int(sign) or (sign == "1" and s[first + 4] == "1")
