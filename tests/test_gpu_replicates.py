"""`eventalign_inference --eventalign rep0.txt rep1.txt ...` (m6a_prep_sites_build_multi, include/m6a.h): replicates pooled on the device.
The device's arrays equal m6a_io_load_sites' on `dataprep` of every file -- X bit for bit, read_rep included -- and both equal
tests/replicate_statement.py; the command's CSVs are byte-identical to K `dataprep`s and one `inference`; only ids, probabilities and
4 K bytes per kept site cross to the host; a file's text is in HBM once, not K times; errors are the loader's and leave no CSV."""
import os
import subprocess
import sys

import numpy as np
import pytest

import eventalign_gen as G
import eventalign_statement as ES
import replicate_fixtures as F
import replicate_statement as RS
from m6anet_amd import _io
from m6anet_amd.constants import PRETRAINED_CONFIGS
from m6anet_amd.data_utils import load_norm_factors

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = F.GOLD
CSVS = ("data.site_proba.csv", "data.indiv_proba.csv")


def norm_of(model):
    return None if model is None else load_norm_factors(PRETRAINED_CONFIGS[model][2])


def prep_dirs(tmp_path, files, tag="", **kw):
    """`dataprep --device cpu` of every file (one directory per distinct path and setting)"""
    dirs = []
    for f in files:
        d = str(tmp_path / ("prep_%s_%s" % (os.path.basename(f), tag)))
        if not os.path.exists(d):
            _io.dataprep(f, d, n_threads=4, device="cpu", **kw)
        dirs.append(d)
    return dirs


def message(e):
    return str(e).split(": ", 1)[1]


def device_equals_loader(tmp_path, files, norm, tag, readcount_max=1000, min_segment_count=1, statement=None):
    """The device's arrays against the loader's on the two-step output (and against `statement`, replicate_statement.sites()' dict);
    returns the number of pooled sites (0 where the loader finds none)."""
    dirs = prep_dirs(tmp_path, files, "%s_%d_%d" % (tag, readcount_max, min_segment_count), readcount_max=readcount_max,
                     min_segment_count=min_segment_count)
    try:
        nat = _io.NativeSites(dirs, 20, norm, 4)
    except _io.M6AIOError as e:
        assert message(e).startswith("no site with at least"), tag
        with _io.prep_sites(files, 1, readcount_max, min_segment_count, norm=norm, n_threads=4) as p:
            assert p.n_sites == 0 and p.n_reads == 0 and p.n_replicates == len(files), tag
        return 0
    with _io.prep_sites(files, 1, readcount_max, min_segment_count, norm=norm, n_threads=4) as p:
        X, km, off = p.inputs()
        S = len(nat.tx_pos)
        assert p.n_sites == S and p.n_reads == nat.X.shape[0], tag
        assert np.array_equal(X.view(np.uint32), nat.X.view(np.uint32)), tag
        assert np.array_equal(km, nat.site_kmers) and np.array_equal(off, nat.off) and np.array_equal(p.off, nat.off), tag
        assert np.array_equal(p.tx_pos, nat.tx_pos), tag
        assert np.array_equal(p.read_ids.view(np.uint64), nat.read_id_values.view(np.uint64)), tag
        assert np.array_equal(p.read_rep, nat.read_rep) and p.read_rep.dtype == np.int32, tag
        assert [p.names[t] for t in p.site_tx] == [nat.tx_id(i) for i in range(S)], tag
        assert [bytes(k[1:6]).decode() for k in p.kmer7] == [nat.kmer5(i) for i in range(S)], tag
        assert p.n_replicates == nat.n_replicates == len(files), tag
        if statement is not None:
            w = statement
            assert np.array_equal(X.view(np.uint32), w["X"].view(np.uint32)) and np.array_equal(km, w["km"]) and np.array_equal(off, w["off"]), tag
            assert np.array_equal(p.tx_pos, w["tx_pos"]) and np.array_equal(p.read_ids.view(np.uint64), w["read_ids"].view(np.uint64)), tag
            assert np.array_equal(p.read_rep, w["read_rep"]) and [p.names[t] for t in p.site_tx] == w["tx"], tag
            assert [bytes(k).decode() for k in p.kmer7] == w["kmer7"], tag
    nat.close()
    return S


# ---- 1. arrays ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", ["HCT116_RNA002", "arabidopsis_RNA002", None])
@pytest.mark.parametrize("fixture", sorted(F.FIXTURES))
def test_device_arrays_equal_the_loader(tmp_path, fixture, model):
    files = F.write(tmp_path, fixture)
    assert device_equals_loader(tmp_path, files, norm_of(model), fixture) > 50


@pytest.mark.parametrize("kw", [dict(min_segment_count=5), dict(min_segment_count=20), dict(readcount_max=40)])
def test_device_arrays_equal_the_loader_with_site_flags(tmp_path, kw):
    files = F.write(tmp_path, "split")
    norm = norm_of("HCT116_RNA002")
    want = RS.sites([RS.file_records(F.parts()[c], 1, kw.get("readcount_max", 1000), kw.get("min_segment_count", 1)) for c in "ab"], norm)
    assert device_equals_loader(tmp_path, files, norm, "split", statement=want, **kw) == len(want["tx"]) > 0


# ---- 2. edges of the new kernels -----------------------------------------------------------------------------------------------
def write_files(tmp_path, tag, blobs):
    out = []
    for k, data in enumerate(blobs):
        p = tmp_path / ("%s_%d.txt" % (tag, k))
        p.write_bytes(data)
        out.append(str(p))
    return out


def held_to_statement_and_loader(tmp_path, tag, blobs, norm, min_segment_count=1):
    files = write_files(tmp_path, tag, blobs)
    try:
        want = RS.sites([RS.file_records(b, 1, 1000, min_segment_count) for b in blobs], norm)
    except ES.StatementError as e:
        assert e.text.startswith("no site with at least")
        want = None
    n = device_equals_loader(tmp_path, files, norm, tag, min_segment_count=min_segment_count, statement=want)
    assert n == (0 if want is None else len(want["tx"]))
    return want


SITES = (3, 12, 21, 30, 39)


def small_parts(seed=11):
    """Four files over TXA (five sites) and TXAB (its name continues TXA's): per site the reads of each file
         site 0   1 + 1 + 1 (+ 17 in the fourth file)      site 1   19 + 1      site 2   20 + 0      site 3   10 + 10
         site 4   nothing in file 0: 12 in file 1, 9 in file 2 (one of them declined: exponent-form floats)
         TXAB     11 in file 1 only, 9 in file 2 -> first seen in file 1"""
    rng = np.random.default_rng(seed)
    a = G.Tx(rng, "TXA", 50, SITES, base=100)
    ab = G.Tx(rng, "TXAB", 50, SITES, base=7)
    fs = [G.File(rng) for _ in range(4)]
    plan = {0: [(a, 0, range(0, 1)), (a, 1, range(100, 119)), (a, 2, range(200, 220)), (a, 3, range(300, 310))],
            1: [(ab, 1, range(600, 611)), (a, 0, range(1, 2)), (a, 1, range(119, 120)), (a, 3, range(310, 320)), (a, 4, range(400, 412))],
            2: [(a, 4, range(412, 420)), (ab, 1, range(611, 620)), (a, 0, range(2, 3))],
            3: [(a, 0, range(3, 20))]}
    for k, items in plan.items():
        for tx, site, reads in items:
            G.site_reads(fs[k], tx, tx.base + SITES[site], list(reads), mismatch=0)
    G.site_reads(fs[2], a, a.base + SITES[4], [420], mismatch=0, mean="7.512e1")          # declined: the host half's rows
    return [f.bytes() for f in fs], a, ab


@pytest.mark.parametrize("model", ["HCT116_RNA002", None])
def test_parts_of_one_read_and_sums_at_the_floor(tmp_path, model):
    blobs, a, ab = small_parts()
    norm = norm_of(model)
    three = held_to_statement_and_loader(tmp_path, "small3", blobs[:3], norm)
    four = held_to_statement_and_loader(tmp_path, "small4", blobs, norm)
    key = lambda w: list(zip(w["tx"], w["tx_pos"].tolist()))
    site0 = ("TXA", a.base + SITES[0] + 2)
    assert site0 not in key(three) and site0 in key(four)                 # 1 + 1 + 1 < 20; + 17 = 20
    assert four["parts"][key(four).index(site0)] == [(0, 1), (1, 1), (2, 1), (3, 17)]
    assert [p for p in three["parts"]] == [[(0, 19), (1, 1)], [(0, 20)], [(0, 10), (1, 10)], [(1, 11), (2, 9)], [(1, 12), (2, 9)]]
    assert key(three)[3][0] == "TXAB" and key(three)[4] == ("TXA", a.base + SITES[4] + 2)
    with _io.prep_on_device(write_files(tmp_path, "decl", blobs[2:3])[0], 1) as t:        # the exponent-form read was declined
        d = _io.table_arrays(t.contents)
    assert 420 in {int(r) for r, st in zip(d["run_read"], d["run_status"]) if st != 0}


def test_positions_that_need_the_wide_key(tmp_path):
    """18 transcripts (5 bits) and positions from 5 to 9e17 (60 bits): the pooled key takes 65 bits, so the sort takes two passes"""
    rng = np.random.default_rng(12)
    bases = [3, 9 * 10 ** 17] + [int(x) for x in rng.integers(10 ** 3, 10 ** 17, 16)]
    txs = [G.Tx(rng, "W%d" % t, 12, (3,), base=bases[t]) for t in range(18)]
    f0, f1 = G.File(rng), G.File(rng)
    for t in rng.permutation(18):
        G.site_reads(f0, txs[t], txs[t].base + 3, list(range(11)), mismatch=0)
    for t in rng.permutation(18):
        G.site_reads(f1, txs[t], txs[t].base + 3, list(range(50, 60)), mismatch=0)
    want = held_to_statement_and_loader(tmp_path, "wide", [f0.bytes(), f1.bytes()], None)
    assert len(want["tx"]) == 18 and ES.bits_for(max(bases) - min(bases)) + ES.bits_for(17) > 64


def test_more_candidate_sites_than_a_radix_tile(tmp_path):
    """4 500 candidate sites of one read in file 0 (the sort's tiles hold 4 096 keys); file 1 lists the transcripts the other way
    round and brings 19 more reads to every 150th site"""
    rng = np.random.default_rng(13)
    txs = [G.Tx(rng, "RT%d" % t, 48, SITES, base=int(rng.integers(0, 10 ** 6))) for t in range(900)]
    f0, f1 = G.File(rng), G.File(rng)
    for t in range(900):
        for k in range(5):
            G.site_reads(f0, txs[t], txs[t].base + SITES[k], [10 * k], events=(1, 2), mismatch=0)
    n = 0
    for t in reversed(range(900)):
        for k in range(5):
            if (5 * t + k) % 150 == 0:
                G.site_reads(f1, txs[t], txs[t].base + SITES[k], list(range(100 + 20 * k, 119 + 20 * k)), events=(1, 2), mismatch=0)
                n += 1
    want = held_to_statement_and_loader(tmp_path, "tiles", [f0.bytes(), f1.bytes()], norm_of("HCT116_RNA002"))
    assert len(want["tx"]) == n == 30 and all(p == [(0, 1), (1, 19)] for p in want["parts"])
    assert len(RS.union([RS.file_records(f0.bytes(), 1, 1000, 1)])) == 4500


# ---- 3. CLI bytes ------------------------------------------------------------------------------------------------------------
def run(args, timeout=900, env=None, check=True):
    return subprocess.run([sys.executable, "-m", "m6anet_amd"] + args, cwd=REPO, timeout=timeout, env=env, check=check,
                          stdout=subprocess.PIPE, stderr=subprocess.PIPE)


def two_step_and_fused(tmp_path, files, tag, flags=(), env=None, expect_fail=False):
    """K `dataprep`s and one `inference` against the fused command; returns (two-step out_dir, fused out_dir, the fused run)"""
    two, fused = (str(tmp_path / (tag + s)) for s in ("_two", "_fused"))
    site = [f for f in flags if f.split("=")[0] in ("--readcount_min", "--readcount_max", "--min_segment_count")]
    dirs = []
    for f in files:
        d = str(tmp_path / ("cli_%s_%s" % (os.path.basename(f), "".join(site).replace("-", ""))))
        if not os.path.exists(d):
            run(["dataprep", "--eventalign", f, "--out_dir", d] + site, env=env)
        dirs.append(d)
    infer = [f for f in flags if f not in site]
    a = run(["inference", "--input_dir"] + dirs + ["--out_dir", two] + infer, env=env, check=not expect_fail)
    b = run(["eventalign_inference", "--eventalign"] + list(files) + ["--out_dir", fused] + list(flags), env=env, check=not expect_fail)
    assert (a.returncode != 0) == (b.returncode != 0) == expect_fail, b.stderr.decode()[-2000:]
    for fn in CSVS:
        assert open(os.path.join(two, fn), "rb").read() == open(os.path.join(fused, fn), "rb").read(), (tag, fn)
    return two, fused, b


@pytest.mark.parametrize("tag, flags, env", [
    ("default", [], None),
    ("fast", ["--encoder", "fast"], None),
    ("tail", ["--drop_unflushed_tail", "--batch_size", "8", "--save_per_batch", "3", "--seed", "5"], None),
    ("arabidopsis", ["--pretrained_model", "arabidopsis_RNA002"], None),
    ("msc1_rc40", ["--min_segment_count=1", "--readcount_max=40", "--num_iterations", "100"], None),
    ("chunk4", [], {"M6A_PREP_CHUNK_KB": "4"}),
])
def test_cli_bytes_equal_the_two_step_path(tmp_path, tag, flags, env):
    env = None if env is None else dict(os.environ, **env)
    for fixture in ("split", "three", "overlap", "gap"):
        two, fused, _ = two_step_and_fused(tmp_path, F.write(tmp_path, fixture), fixture + "_" + tag, flags, env=env)
        rows = open(os.path.join(fused, CSVS[1])).read().splitlines()[1:]
        reps = {r.split(",")[2].rsplit("_", 1)[1] for r in rows}
        assert rows and reps == ({"0", "2"} if fixture == "gap" else {str(k) for k in range(len(F.FIXTURES[fixture]))}), fixture


def test_the_bundled_file_twice_against_the_reference_replicate_run(tmp_path):
    """The two-step path byte for byte, and the reference's own replicate run in what does not depend on the order of reads inside
    a site (that order is the project's rule from eventalign, the reference's comes from an unstable argsort of its data.json)."""
    import pandas as pd
    files = F.write(tmp_path, "twice")
    flags = ["--n_processes", "1", "--num_iterations", "5", "--min_segment_count", "1"]
    two, fused = (str(tmp_path / s) for s in ("two", "fused"))
    prep = str(tmp_path / "prep")
    run(["dataprep", "--eventalign", files[0], "--out_dir", prep, "--min_segment_count", "1", "--n_processes", "1"])
    run(["inference", "--input_dir", prep, prep, "--out_dir", two, "--n_processes", "1", "--num_iterations", "5"])
    run(["eventalign_inference", "--eventalign"] + files + ["--out_dir", fused] + flags)
    for fn in CSVS:
        assert open(os.path.join(two, fn), "rb").read() == open(os.path.join(fused, fn), "rb").read(), fn
    key_s = ["transcript_id", "transcript_position"]
    ts = pd.read_csv(os.path.join(fused, CSVS[0])).sort_values(key_s).reset_index(drop=True)
    gs = pd.read_csv(os.path.join(GOLD, "replicate_site_proba.csv")).sort_values(key_s).reset_index(drop=True)
    ts = ts.merge(gs[key_s], on=key_s).sort_values(key_s).reset_index(drop=True)          # the rows the golden holds
    assert len(ts) == len(gs) > 0
    for k in key_s + ["n_reads", "kmer"]:
        assert (ts[k] == gs[k]).all(), k
    assert np.allclose(ts["mod_ratio"], gs["mod_ratio"])
    key_i = key_s + ["read_index"]
    ti = pd.read_csv(os.path.join(fused, CSVS[1])).sort_values(key_i).reset_index(drop=True)
    gi = pd.read_csv(os.path.join(GOLD, "replicate_indiv_proba.csv.gz")).sort_values(key_i).reset_index(drop=True)
    ti = ti.merge(gs[key_s], on=key_s).sort_values(key_i).reset_index(drop=True)
    assert (ti[key_i].values == gi[key_i].values).all() and set(x.rsplit("_", 1)[1] for x in ti["read_index"]) == {"0", "1"}
    assert np.allclose(ti["probability_modified"], gi["probability_modified"], rtol=2e-5, atol=1e-7)


# ---- 4. errors ---------------------------------------------------------------------------------------------------------------
def other_flank(rng, tx, site):
    """`tx` again (same name, base and sequence) but for the base before the DRACH at `site`: a different 7-mer there, still an
    N-DRACH-N context, and no new DRACH (the 5-mer that starts one base early reads x D R A C: its third and fourth are R A)"""
    twin = G.Tx(rng, tx.name, 5, (), base=tx.base)
    seq = list(tx.seq)
    seq[SITES[site] - 1] = "ACGT"[("ACGT".index(seq[SITES[site] - 1]) + 1) % 4]
    twin.seq = "".join(seq)
    assert all(ES.is_drach(tx.seq[i:i + 5].encode()) == ES.is_drach(twin.seq[i:i + 5].encode()) for i in range(len(tx.seq) - 4))
    return twin


def disagreeing(site, seed=21):
    """two files, each consistent in itself: site 0 has 12 + 12 reads, site 1 has 3 + 4, site 2 has 25 + 0; the second file's
    transcript differs from the first's in the base before `site`"""
    rng = np.random.default_rng(seed)
    tx = G.Tx(rng, "ENSTX", 50, SITES, base=40)
    twin = other_flank(rng, tx, site)
    f0, f1 = G.File(rng), G.File(rng)
    G.site_reads(f0, tx, tx.base + SITES[0], list(range(12)), mismatch=0)
    G.site_reads(f0, tx, tx.base + SITES[1], list(range(20, 23)), mismatch=0)
    G.site_reads(f0, tx, tx.base + SITES[2], list(range(30, 55)), mismatch=0)
    G.site_reads(f1, twin, tx.base + SITES[0], list(range(60, 72)), mismatch=0)
    G.site_reads(f1, twin, tx.base + SITES[1], list(range(80, 84)), mismatch=0)
    return [f0.bytes(), f1.bytes()], tx, twin


def test_replicates_that_disagree_on_a_kept_site(tmp_path):
    blobs, tx, twin = disagreeing(0)
    files = write_files(tmp_path, "dis", blobs)
    norm = norm_of("HCT116_RNA002")
    with pytest.raises(ES.StatementError) as st:
        RS.sites([RS.file_records(b, 1, 1000, 1) for b in blobs], norm)
    with pytest.raises(_io.M6AIOError) as want:
        _io.NativeSites(prep_dirs(tmp_path, files, "dis", min_segment_count=1), 20, norm, 2)
    with pytest.raises(_io.M6AIOError) as got:
        _io.prep_sites(files, 1, 1000, 1, norm=norm)
    text = "replicates disagree on the sequence of ENSTX:%d" % (tx.base + SITES[0] + 2)
    assert message(want.value) == message(got.value) == st.value.text == text and got.value.code == want.value.code == -4
    dirs = []
    for k, f in enumerate(files):
        dirs.append(str(tmp_path / ("dis_cli_%d" % k)))
        run(["dataprep", "--eventalign", f, "--out_dir", dirs[-1], "--min_segment_count=1"])
    two, fused = str(tmp_path / "dis_two"), str(tmp_path / "dis_fused")
    r = run(["inference", "--input_dir"] + dirs + ["--out_dir", two], check=False)
    assert r.returncode != 0 and text.encode() in r.stderr
    r = run(["eventalign_inference", "--eventalign"] + files + ["--out_dir", fused, "--min_segment_count=1"], check=False)
    assert r.returncode != 0 and text.encode() in r.stderr
    assert not any(os.path.exists(os.path.join(fused, f)) for f in CSVS)


def test_a_dropped_site_is_not_checked(tmp_path):
    """the same edit in a site whose pooled reads stay below 20: no error, the same bytes; and a norm table without a 5-mer that
    only that site uses: no error either"""
    blobs, tx, twin = disagreeing(1)
    files = write_files(tmp_path, "drop", blobs)
    norm = norm_of("HCT116_RNA002")
    want = RS.sites([RS.file_records(b, 1, 1000, 1) for b in blobs], norm)
    assert device_equals_loader(tmp_path, files, norm, "drop", statement=want) == 2
    two_step_and_fused(tmp_path, files, "drop_cli", ["--min_segment_count=1"])
    used = {k7[c:c + 5] for k7 in want["kmer7"] for c in range(3)}
    at = SITES[1] - 1
    only = [k for k in (s.seq[at + c:at + c + 5] for s in (tx, twin) for c in range(3)) if k not in used]
    assert only
    del norm[only[0]]
    again = RS.sites([RS.file_records(b, 1, 1000, 1) for b in blobs], norm)
    assert device_equals_loader(tmp_path, files, norm, "drop_norm", statement=again) == 2
    kept_only = sorted(used)[0]                              # and one that a kept site uses: the loader's text
    del norm[kept_only]
    with pytest.raises(_io.M6AIOError) as e1:
        _io.NativeSites(prep_dirs(tmp_path, files, "drop_norm", min_segment_count=1), 20, norm, 2)
    with pytest.raises(_io.M6AIOError) as e2:
        _io.prep_sites(files, 1, 1000, 1, norm=norm)
    assert message(e1.value) == message(e2.value) and "no normalisation factors for" in message(e2.value) and e2.value.code == -4


def test_errors_leave_no_csv(tmp_path):
    files = F.write(tmp_path, "split")
    out = str(tmp_path / "missing")
    r = run(["eventalign_inference", "--eventalign", files[0], str(tmp_path / "nope.txt"), "--out_dir", out], check=False)
    assert r.returncode != 0 and b"cannot open" in r.stderr
    assert not any(os.path.exists(os.path.join(out, f)) for f in CSVS)
    out = str(tmp_path / "budget")
    r = run(["eventalign_inference", "--eventalign"] + files + ["--out_dir", out], env=dict(os.environ, M6A_PREP_BUDGET_MB="1"), check=False)
    assert r.returncode != 0 and b"two-step path" in r.stderr
    assert not any(os.path.exists(os.path.join(out, f)) for f in CSVS)
    empty = [str(tmp_path / "rep_h.txt")] * 2
    open(empty[0], "wb").write(F.parts()["h"])
    two, fused, b = two_step_and_fused(tmp_path, empty, "empty", ["--min_segment_count=1"], expect_fail=True)
    assert len(open(os.path.join(fused, CSVS[0])).read().splitlines()) == 1 and len(open(os.path.join(fused, CSVS[1])).read().splitlines()) == 1
    assert b"no site with at least 20 reads" in b.stderr


# ---- 5. what crosses the link --------------------------------------------------------------------------------------------------
def test_x_stays_on_the_device(tmp_path):
    files = F.write(tmp_path, "three")
    K = len(files)
    with _io.prep_sites(files, 1, 1000, 1, norm=norm_of("HCT116_RNA002")) as p:
        _, d2h = p.times()
        R, S = p.n_reads, p.n_sites
        assert (S, R) == (132, 8186)
        assert d2h < 36 * R, (d2h, R)
        assert d2h < 16 * R + (64 + 4 * K) * S + K * (len(p.tx_blob) + 24 * len(p.names)), (d2h, R, S)
        p.fetch()
        assert p.times()[1] == d2h + 4 * R + 12 * S


# ---- 6. memory is per file, not per job ------------------------------------------------------------------------------------------
def test_a_files_text_is_in_hbm_once(tmp_path):
    """Three times the 200 MB file of test_gpu_eventalign_inference.test_200mb_file.  What stays per file is X (36 B) and the id
    (8 B) of each read of its sites with >= min_segment_count reads -- at the default 20 those are the one-file run's R1 reads in
    S1 sites -- and 27 B per such site; the pooled arrays are X, id, read_prob per read (48 B) and under 64 B per site.  So with
    the bounds of the design, kept = 48 R1 + 64 S1 and pooled = 52 R + 64 S, no term of the size of the text comes K times."""
    from test_dataprep_rows import unpack
    text = open(unpack(tmp_path, "ref_tests_data")).read()
    header, body = text.split("\n", 1)
    ev = str(tmp_path / "big.txt")
    with open(ev, "w", buffering=16 << 20) as f:
        f.write(header + "\n")
        for k in range(100):
            f.write(body.replace("ENST", "C%dENST" % k) if k else body)
    assert os.path.getsize(ev) > 200e6
    with _io.prep_sites(ev, n_threads=8) as p:
        peak1, R1, S1 = p.peak_bytes, p.n_reads, p.n_sites
    with _io.prep_sites([ev] * 3, n_threads=8) as p:
        peak3, R, S = p.peak_bytes, p.n_reads, p.n_sites
    assert R == 3 * R1 > 0 and S == S1 > 0
    kept, pooled = 48 * R1 + 64 * S1, 52 * R + 64 * S
    print("peak_bytes: one file %d, three files %d, bound %d (kept %d, pooled %d)" % (peak1, peak3, peak1 + 3 * kept + pooled, kept, pooled))
    assert peak1 > os.path.getsize(ev)
    assert peak3 <= peak1 + 3 * kept + pooled, (peak1, peak3, kept, pooled)
    two_step_and_fused(tmp_path, [ev] * 3, "big", ["--n_processes", "8", "--num_iterations", "100"])
