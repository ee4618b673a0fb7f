"""`eventalign_diff --signal` on the two small generated conditions of tests/test_gpu_eventalign_diff.py (built here again from
tests/eventalign_gen.py: the first has two replicate files, each has sites the other lacks).  With the flag OUT/a, OUT/b and
data.diff.csv keep the bytes of the run without it, and data.diff_signal.csv is the text m6anet_amd/ranksum.py writes from
tests/signal_ranksum_statement.py applied to the X of the two conditions, taken here through prep_sites(...).inputs(): nine rows per
shared site in data.diff.csv's order of sites and X's order of columns, one Benjamini-Hochberg family.  B's reads of ENST0001.1's
second site were generated with the current mean 118.25 at all three positions (site_reads passes `mean` to every line of its
2 flank + 1 positions), so that site's three norm_mean rows carry the smallest p of the file.  The same with --window_mb; the
conditions swapped negate z, mirror the AUC and leave p alone; without the flag the file is not written."""
import os
import subprocess
import sys

import numpy as np
import pytest

import eventalign_gen as G
import signal_ranksum_statement as SS
from m6anet_amd import _io, ranksum
from m6anet_amd.constants import PRETRAINED_CONFIGS
from m6anet_amd.data_utils import load_norm_factors

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSVS = ("data.site_proba.csv", "data.indiv_proba.csv")
MODEL = "HCT116_RNA002"
FLAGS = ["--min_segment_count", "1", "--num_iterations", "5", "--n_processes", "4"]
SITES = (3, 12, 21, 30)
SHIFTED = ("ENST0001.1", 100 + SITES[1] + 2)                     # the site whose reads in B have another current level (a site's
                                                                 # position is that of its 5-mer's centre)


def write_conditions(d):
    """A: two replicates, T1 sites 0 1 2 and T2 site 0.  B: one file, T1 sites 1 2 3 and T2 sites 0 1.  Shared: three sites.  T1
    site 0 has its 20 reads only over both replicates; B's reads of T1 site 1 have another current level."""
    rng = np.random.default_rng(41)
    t1, t2 = G.Tx(rng, "ENST0001.1", 40, SITES, base=100), G.Tx(rng, "ENST0002.3", 40, SITES, base=7)
    a1, a2, b1 = G.File(rng), G.File(rng), G.File(rng)
    for f, tx, site, reads, kw in ((a1, t1, 0, range(0, 11), {}), (a1, t1, 1, range(100, 125), {}), (a1, t1, 2, range(200, 214), {}),
                                   (a1, t2, 0, range(500, 522), {}), (a2, t1, 0, range(0, 9), {}), (a2, t1, 2, range(220, 241), {}),
                                   (a2, t1, 1, range(130, 138), {}), (b1, t2, 1, range(600, 623), {}), (b1, t1, 3, range(300, 321), {}),
                                   (b1, t1, 1, range(100, 140), dict(mean="118.25")), (b1, t1, 2, range(205, 227), {}),
                                   (b1, t2, 0, range(500, 564), {})):
        G.site_reads(f, tx, tx.base + SITES[site], list(reads), mismatch=0, **kw)
    paths = {}
    for name, f in (("a1", a1), ("a2", a2), ("b1", b1)):
        paths[name] = str(d / (name + ".txt"))
        with open(paths[name], "wb") as out:
            out.write(f.bytes())
    return {"a": [paths["a1"], paths["a2"]], "b": [paths["b1"]], "dir": d}


@pytest.fixture(scope="module")
def conditions(tmp_path_factory):
    return write_conditions(tmp_path_factory.mktemp("diff_signal"))


def diff(conditions, tag, first, second, extra=()):
    """the command into a directory of its own under the module's; a tag is run once and its result shared"""
    out = str(conditions["dir"] / tag)
    if tag in conditions.setdefault("ran", {}):
        return out, conditions["ran"][tag]
    argv = ["--eventalign_a"] + conditions[first] + ["--eventalign_b"] + conditions[second] + ["--out_dir", out] + list(extra) + FLAGS
    r = subprocess.run([sys.executable, "-m", "m6anet_amd", "eventalign_diff"] + argv, env=dict(os.environ, PYTHONPATH=REPO), capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    conditions["ran"][tag] = r.stdout
    return out, r.stdout


@pytest.fixture(scope="module")
def tables(conditions):
    """the two conditions through prep_sites: X, off and the site table -- what the statement is applied to"""
    norm = load_norm_factors(PRETRAINED_CONFIGS[MODEL][2])
    out = {}
    for c in "ab":
        files = conditions[c]
        with _io.prep_sites(files[0] if len(files) == 1 else files, 1, 1000, 1, norm=norm, n_threads=4) as s:
            X, _, off = s.inputs()
            out[c] = dict(X=X, off=off, tx=[s.names[t] for t in s.site_tx], pos=s.tx_pos.copy(), kmer=[bytes(k[1:6]).decode() for k in s.kmer7])
    return out


def expected_text(a, b):
    pa, pb = ranksum.join(a["tx"], a["pos"], b["tx"], b["pos"])
    gt, eq, _, z = SS.site_signal_ranksum(a["X"], a["off"], b["X"], b["off"], pa, pb)
    return ranksum.signal_text([a["tx"][k] for k in pa], a["pos"][pa], [a["kmer"][k] for k in pa], np.diff(a["off"])[pa], np.diff(b["off"])[pb],
                               gt, eq, z)


def same_tree(with_flag, without):
    """OUT/a, OUT/b and data.diff.csv byte for byte; the flag adds one file and nothing else"""
    for fn in [os.path.join(c, f) for c in "ab" for f in CSVS] + [ranksum.DIFF_FILE]:
        with open(os.path.join(with_flag, fn), "rb") as f0, open(os.path.join(without, fn), "rb") as f1:
            assert f0.read() == f1.read(), fn
    assert sorted(os.listdir(without)) == ["a", "b", ranksum.DIFF_FILE]
    assert sorted(os.listdir(with_flag)) == ["a", "b", ranksum.DIFF_FILE, ranksum.SIGNAL_FILE]
    for c in "ab":
        assert sorted(os.listdir(os.path.join(with_flag, c))) == sorted(os.listdir(os.path.join(without, c))) == sorted(CSVS)


@pytest.mark.parametrize("tag, extra", [("plain", []), ("windows", ["--window_mb", "1"])])
def test_outputs(conditions, tables, tag, extra):
    without, stdout0 = diff(conditions, tag, "a", "b", extra)
    assert not os.path.exists(os.path.join(without, ranksum.SIGNAL_FILE))          # without the flag the file does not exist
    out, stdout = diff(conditions, tag + "_signal", "a", "b", list(extra) + ["--signal"])
    assert stdout == stdout0 and stdout.splitlines()[-1] == "eventalign_diff: 3 sites in both conditions, 1 only in A, 2 only in B"
    same_tree(out, without)
    text = open(os.path.join(out, ranksum.SIGNAL_FILE)).read()
    assert text == expected_text(tables["a"], tables["b"])
    lines = text.splitlines()
    assert lines[0] == ranksum.SIGNAL_HEADER and len(lines) == 1 + 3 * 9
    rows = [ln.split(",") for ln in lines[1:]]
    sites = [ln.split(",")[:5] for ln in open(os.path.join(out, ranksum.DIFF_FILE)).read().splitlines()[1:]]
    assert [r[:5] for r in rows] == [s for s in sites for _ in range(9)]           # data.diff.csv's sites, in its order, nine rows each
    assert [(r[0], int(r[3]), int(r[4])) for r in rows[::9]] == [("ENST0001.1", 33, 40), ("ENST0001.1", 35, 22), ("ENST0002.3", 22, 64)]
    assert [(r[5], r[6]) for r in rows] == [(o, f) for o in ("-1", "0", "1") for f in ("dwell_time", "norm_std", "norm_mean")] * 3
    p = np.array([float(r[9]) for r in rows])
    q = np.array([float(r[10]) for r in rows])
    assert not np.isnan(p).any() and ((0 < p) & (p <= q) & (q <= 1)).all()         # p <= q <= 1
    shifted = [k for k, r in enumerate(rows) if (r[0], int(r[1])) == SHIFTED and r[6] == "norm_mean"]
    assert [rows[k][5] for k in shifted] == ["-1", "0", "1"]                       # `mean` went to all three positions
    assert sorted(np.argsort(p, kind="stable")[:3].tolist()) == shifted and p[shifted].max() < np.delete(p, shifted).min()
    assert all(float(rows[k][8]) < 0 for k in shifted)                             # A's levels are drawn from 60..130, most below 118.25: B above A


def test_conditions_swapped(conditions):
    ab, _ = diff(conditions, "plain_signal", "a", "b", ["--signal"])
    ba, stdout = diff(conditions, "swap_ba_signal", "b", "a", ["--signal"])
    assert stdout.splitlines()[-1] == "eventalign_diff: 3 sites in both conditions, 2 only in A, 1 only in B"

    def table(d):
        rows = [ln.split(",") for ln in open(os.path.join(d, ranksum.SIGNAL_FILE)).read().splitlines()[1:]]
        return {(r[0], r[1], r[2], r[5], r[6]): r for r in rows}
    rows_ab, rows_ba = table(ab), table(ba)
    assert sorted(rows_ab) == sorted(rows_ba) and len(rows_ab) == 27
    for key, r in rows_ab.items():
        s = rows_ba[key]
        assert (r[3], r[4]) == (s[4], s[3])
        z, zs = float(r[8]), float(s[8])
        assert zs == -z and np.signbit(zs) != np.signbit(z)                       # z negated, a zero's sign included
        assert r[9] == s[9]                                                       # p unchanged, to the digit
        # the AUC mirrored: U_ab + U_ba = n m exactly -- the two AUCs are that sum's two parts over n m, each rounded once
        nm = int(r[3]) * int(r[4])
        u = float(r[7]) * nm
        assert float(s[7]) == (nm - round(2 * u) / 2) / nm and float(r[7]) == round(2 * u) / 2 / nm
