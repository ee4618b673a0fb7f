"""`eventalign_diff --ks --ks_exact` on the two small generated conditions of tests/test_gpu_eventalign_diff_ks.py (its fixtures, built
again for this module).  With the flag, every file but the two KS files keeps the bytes of the run without it, and in the two KS files
every column but p_value and q_value is the run's without it, with p_method appended: p_value is repr of tests/ks_exact_statement.py's
value at the file's own n_reads_a and n_reads_b and the d_pos, d_neg the engine returns for the pair, q_value is ranksum.bh of the
p_value column, p_method is `exact` in every row (the bags hold tens of reads).  The run without the flag is the text
m6anet_amd/ranksum.py writes from tests/ks_statement.py with no exact p-values, as before.  --ks_exact without --ks is an argument
error: exit status 2, one line on stderr, nothing written."""
import os
import subprocess
import sys

import numpy as np
import pytest

import ks_exact_statement as ST
import test_gpu_eventalign_diff_ks as DK
import test_gpu_eventalign_diff_signal as DS
from m6anet_amd import ranksum
from m6anet_amd.engine import M6ANetEngine
from test_gpu_eventalign_diff_ks import conditions, tables  # noqa: F401  (module-scoped fixtures, instantiated for this module)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def integers(tables, weights):  # noqa: F811
    """d_pos, d_neg of the shared sites as the engine returns them: [P] on the read probabilities and [P, 9] on X"""
    a, b = tables["a"], tables["b"]
    pa, pb = ranksum.join(a["tx"], a["pos"], b["tx"], b["pos"])
    eng = M6ANetEngine(weights=weights["hct116"], device=0)
    try:
        return {False: eng.site_ks(a["rp"], a["off"], b["rp"], b["off"], pa, pb)[:2], True: eng.site_signal_ks(a["X"], a["off"], b["X"], b["off"], pa, pb)[:2]}
    finally:
        eng.close()


def test_exact_p_values_in_both_files(conditions, tables, integers):  # noqa: F811
    without, stdout0 = DS.diff(conditions, "signal_ks", "a", "b", ["--signal", "--ks"])
    exact, stdout1 = DS.diff(conditions, "signal_ks_exact", "a", "b", ["--signal", "--ks", "--ks_exact"])
    assert stdout0 == stdout1 and stdout1.splitlines()[-1] == DK.SITES_LINE
    for signal, fn in ((False, ranksum.KS_FILE), (True, ranksum.SIGNAL_KS_FILE)):
        assert DK.read(without, fn).decode() == DK.expected(tables["a"], tables["b"], signal)     # without the flag: the text as it was
    assert sorted(os.listdir(exact)) == sorted(os.listdir(without))
    for fn in [os.path.join(c, f) for c in "ab" for f in DS.CSVS] + [ranksum.DIFF_FILE, ranksum.SIGNAL_FILE]:
        assert DK.read(exact, fn) == DK.read(without, fn), fn
    for signal, fn, first, n_rows in ((False, ranksum.KS_FILE, 5, 3), (True, ranksum.SIGNAL_KS_FILE, 7, 27)):
        head0, rows0 = DK.rows_of(without, fn)
        head1, rows1 = DK.rows_of(exact, fn)
        at_p = first + 5                                         # median_a median_b median_shift ks_d ks_sign p_value q_value
        assert head1 == head0 + ",p_method" and len(rows1) == len(rows0) == n_rows
        assert [r[:at_p] for r in rows1] == [r[:at_p] for r in rows0] and all(len(r) == at_p + 3 for r in rows1)
        d_pos, d_neg = (np.asarray(x).ravel() for x in integers[signal])
        assert d_pos.size == n_rows and (d_pos >= 0).all()
        want = [ST.p_exact(int(r[3]), int(r[4]), int(max(dp, dn))) for r, dp, dn in zip(rows1, d_pos, d_neg)]
        assert [r[at_p] for r in rows1] == [repr(p) for p in want]
        assert [r[at_p + 1] for r in rows1] == [repr(float(q)) for q in ranksum.bh(np.array(want))]
        assert all(r[at_p + 2] == "exact" for r in rows1)
        assert [r[at_p] for r in rows1] != [r[at_p] for r in rows0]                   # not the limit distribution's values
    # the whole text, from the module that writes it
    a, b = tables["a"], tables["b"]
    pa, pb = ranksum.join(a["tx"], a["pos"], b["tx"], b["pos"])
    head = ([a["tx"][k] for k in pa], a["pos"][pa], [a["kmer"][k] for k in pa], np.diff(a["off"])[pa], np.diff(b["off"])[pb])
    ks = DK.KS.site_ks(a["rp"], a["off"], b["rp"], b["off"], pa, pb)
    p = ST.p_exact_many(head[3], head[4], ST.ks_h(ks[0], ks[1]))
    assert DK.read(exact, ranksum.KS_FILE).decode() == ranksum.ks_text(*head, *ks, p_exact=p)


def test_ks_alone_with_exact_p_values(conditions, tables):  # noqa: F811
    both, _ = DS.diff(conditions, "signal_ks_exact", "a", "b", ["--signal", "--ks", "--ks_exact"])
    only, _ = DS.diff(conditions, "ks_exact", "a", "b", ["--ks", "--ks_exact"])
    assert sorted(os.listdir(only)) == ["a", "b", ranksum.DIFF_FILE, ranksum.KS_FILE]
    assert DK.read(only, ranksum.KS_FILE) == DK.read(both, ranksum.KS_FILE)


def test_the_flag_without_ks_is_an_argument_error(conditions):  # noqa: F811
    out = str(conditions["dir"] / "refused")
    argv = ["--eventalign_a"] + conditions["a"] + ["--eventalign_b"] + conditions["b"] + ["--out_dir", out, "--ks_exact"] + DS.FLAGS
    r = subprocess.run([sys.executable, "-m", "m6anet_amd", "eventalign_diff"] + argv, env=dict(os.environ, PYTHONPATH=DS.REPO), capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 2 and "--ks_exact" in r.stderr and r.stdout == "" and not os.path.exists(out)
