"""`eventalign_diff` on two small generated conditions (tests/eventalign_gen.py): the first has two replicate files, and each has sites
the other lacks.  OUT/a and OUT/b are byte for byte what `eventalign_inference` writes for the condition; data.diff.csv is the text
m6anet_amd/ranksum.py writes from tests/ranksum_statement.py applied to the read probabilities of the two conditions, taken here through
prep_sites -> infer_ptrs -> fetch; the same with --site_proba expected and with --window_mb; and the conditions swapped negate z,
mirror the AUC and leave p alone."""
import os
import subprocess
import sys

import numpy as np
import pytest

import eventalign_gen as G
import ranksum_statement as RS
from m6anet_amd import _io, ranksum
from m6anet_amd.constants import N_SAMPLES, PRETRAINED_CONFIGS
from m6anet_amd.data_utils import load_norm_factors
from m6anet_amd.engine import M6ANetEngine

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSVS = ("data.site_proba.csv", "data.indiv_proba.csv")
MODEL = "HCT116_RNA002"
FLAGS = ["--min_segment_count", "1", "--num_iterations", "5", "--n_processes", "4"]
SITES = (3, 12, 21, 30)


@pytest.fixture(scope="module")
def conditions(tmp_path_factory):
    """A: two replicates, T1 sites 0 1 2 and T2 site 0.  B: one file, T1 sites 1 2 3 and T2 sites 0 1.  Shared: three sites.  T1
    site 0 has its 20 reads only over both replicates; B's reads of T1 site 1 have another current level."""
    d = tmp_path_factory.mktemp("diff")
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


def command(name, argv):
    r = subprocess.run([sys.executable, "-m", "m6anet_amd", name] + argv + FLAGS, env=dict(os.environ, PYTHONPATH=REPO), capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stdout


def diff(conditions, tag, first, second, extra=()):
    """the command into a directory of its own under the module's; a tag is run once and its result shared"""
    out = str(conditions["dir"] / tag)
    if tag in conditions.setdefault("ran", {}):
        return out, conditions["ran"][tag]
    stdout = command("eventalign_diff", ["--eventalign_a"] + conditions[first] + ["--eventalign_b"] + conditions[second] + ["--out_dir", out] + list(extra))
    conditions["ran"][tag] = stdout
    return out, stdout


@pytest.fixture(scope="module")
def single(conditions):
    """`eventalign_inference` on each condition, per --site_proba mode: {(condition, mode): directory}"""
    out = {}
    for mode in ("sampled", "expected"):
        for c in "ab":
            out[c, mode] = str(conditions["dir"] / ("single_%s_%s" % (c, mode)))
            command("eventalign_inference", ["--eventalign"] + conditions[c] + ["--out_dir", out[c, mode], "--site_proba", mode])
    return out


@pytest.fixture(scope="module")
def scored(conditions, weights):
    """the two conditions through prep_sites -> infer_ptrs -> fetch, per mode: what the statement is applied to"""
    thr, norm = PRETRAINED_CONFIGS[MODEL][1], load_norm_factors(PRETRAINED_CONFIGS[MODEL][2])
    out = {}
    for mode in ("sampled", "expected"):
        eng = M6ANetEngine(weights=weights["hct116"], device=0)
        try:
            eng.set_site_mode(mode)
            for c in "ab":
                files = conditions[c]
                with _io.prep_sites(files[0] if len(files) == 1 else files, 1, 1000, 1, norm=norm, n_threads=4) as s:
                    i = s.info
                    eng.set_host_offsets(s.off)
                    eng.infer_ptrs(i.X, i.site_kmers, i.off, s.n_sites, 5, N_SAMPLES, thr, 0, 16, 2, i.read_prob, i.site_prob, i.mod_ratio)
                    eng.sync()
                    rp, sp, mr = s.fetch()
                    out[c, mode] = dict(rp=rp, sp=sp, mr=mr, off=s.off.copy(), tx=[s.names[t] for t in s.site_tx], pos=s.tx_pos.copy(),
                                        kmer=[bytes(k[1:6]).decode() for k in s.kmer7])
        finally:
            eng.close()
    return out


def expected_text(a, b):
    pa, pb = ranksum.join(a["tx"], a["pos"], b["tx"], b["pos"])
    gt, eq, _, z = RS.site_ranksum(a["rp"], a["off"], b["rp"], b["off"], pa, pb)
    return ranksum.diff_text([a["tx"][k] for k in pa], a["pos"][pa], [a["kmer"][k] for k in pa], np.diff(a["off"])[pa], np.diff(b["off"])[pb],
                             a["sp"][pa], b["sp"][pb], a["mr"][pa], b["mr"][pb], gt, eq, z)


def same_files(d0, d1):
    for fn in CSVS:
        with open(os.path.join(d0, fn), "rb") as f0, open(os.path.join(d1, fn), "rb") as f1:
            assert f0.read() == f1.read(), (d0, d1, fn)
    assert sorted(os.listdir(d0)) == sorted(os.listdir(d1)) == sorted(CSVS)


@pytest.mark.parametrize("tag, mode, extra", [("plain", "sampled", []), ("expected", "expected", ["--site_proba", "expected"]),
                                              ("windows", "sampled", ["--window_mb", "1"])])
def test_outputs(conditions, single, scored, tag, mode, extra):
    out, stdout = diff(conditions, tag, "a", "b", extra)
    assert stdout.splitlines()[-1] == "eventalign_diff: 3 sites in both conditions, 1 only in A, 2 only in B"
    same_files(os.path.join(out, "a"), single["a", mode])
    same_files(os.path.join(out, "b"), single["b", mode])
    assert sorted(os.listdir(out)) == ["a", "b", ranksum.DIFF_FILE]
    text = open(os.path.join(out, ranksum.DIFF_FILE)).read()
    assert text == expected_text(scored["a", mode], scored["b", mode])
    lines = text.splitlines()
    assert lines[0] == ranksum.DIFF_HEADER and len(lines) == 4
    rows = [ln.split(",") for ln in lines[1:]]
    assert [r[0] for r in rows] == ["ENST0001.1", "ENST0001.1", "ENST0002.3"]      # the order of the first table
    assert [(int(r[3]), int(r[4])) for r in rows] == [(33, 40), (35, 22), (22, 64)]
    assert all(0 < float(r[11]) <= float(r[12]) <= 1 for r in rows)                # p <= q <= 1


def test_conditions_swapped(conditions):
    ab, _ = diff(conditions, "plain", "a", "b")
    ba, stdout = diff(conditions, "swap_ba", "b", "a")
    assert stdout.splitlines()[-1] == "eventalign_diff: 3 sites in both conditions, 2 only in A, 1 only in B"
    same_files(os.path.join(ab, "a"), os.path.join(ba, "b"))
    rows_ab = {tuple(r[:3]): r for r in (ln.split(",") for ln in open(os.path.join(ab, ranksum.DIFF_FILE)).read().splitlines()[1:])}
    rows_ba = {tuple(r[:3]): r for r in (ln.split(",") for ln in open(os.path.join(ba, ranksum.DIFF_FILE)).read().splitlines()[1:])}
    assert sorted(rows_ab) == sorted(rows_ba) and len(rows_ab) == 3
    for key, r in rows_ab.items():
        s = rows_ba[key]
        assert (r[3], r[4], r[5], r[6], r[7], r[8]) == (s[4], s[3], s[6], s[5], s[8], s[7])
        z, zs = float(r[10]), float(s[10])
        assert zs == -z and np.signbit(zs) != np.signbit(z)                       # z negated, a zero's sign included
        assert r[11] == s[11]                                                     # p unchanged, to the digit
        # the AUC mirrored: U_ab + U_ba = n m exactly -- the two AUCs are that sum's two parts over n m, each rounded once
        nm = int(r[3]) * int(r[4])
        u, us = float(r[9]) * nm, float(s[9]) * nm
        assert round(2 * u) + round(2 * us) == 2 * nm and float(s[9]) == (nm - round(2 * u) / 2) / nm and float(r[9]) == round(2 * u) / 2 / nm
