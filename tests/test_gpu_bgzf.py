"""BGZF input on the device (m6anet_amd/csrc/m6a_bgzf.h; include/m6a.h states the format): the inflate and CRC kernels against the
plain statement (tests/bgzf_statement.py) on every fixture of tests/bgzf_fixtures.py, and `eventalign_inference` on a compressed
file against the same call on its text -- arrays bit for bit, errors word for word, both CSV files byte for byte.  The malformed
fixtures went through the same decode core on the CPU first (tests/test_bgzf_statement.py, tests/sanitize.sh)."""
import filecmp
import gzip
import os

import numpy as np
import pytest

import bgzf_fixtures as F
import bgzf_statement as B
import eventalign_gen as G
import replicate_fixtures as R
from m6anet_amd import _io, bgzf
from test_eventalign_statement import hct116
from test_gpu_eventalign_inference import CSVS, run
from test_gpu_prep_edges import SITE_CASES

pytestmark = pytest.mark.gpu
GOOD, BAD = sorted(F.good()), sorted(F.malformed())
EINVAL, ENOMEM, EFORMAT = -1, -2, -4


def message(e):
    """the library's text, behind `m6a_prep error <code>: `"""
    return str(e.value if hasattr(e, "value") else e).split(": ", 1)[1]


def write(tmp_path, name, data):
    p = tmp_path / name
    p.write_bytes(data)
    return str(p)


def one_correct_call(tmp_path):
    """after an error: the same process still inflates, and still parses a compressed file"""
    data = F.good()["family_plain"]
    path = write(tmp_path, "after.gz", data)
    assert _io.bgzf_inflate(path) == F.inflated("family_plain")[0]
    with _io.prep_sites(path, n_threads=2) as p:
        assert p.n_sites == len(G.case("plain", 1).sites["tx_pos"]) and p.n_bgzf_blocks == len(F.inflated("family_plain")[1])


# ---- 1. the kernels are the statement on good files, also with every header, footer and stream across 4 KB upload chunks
@pytest.mark.parametrize("chunk_kb", [None, 4])
@pytest.mark.parametrize("name", GOOD)
def test_inflate_is_the_statement(tmp_path, monkeypatch, name, chunk_kb):
    if chunk_kb:
        monkeypatch.setenv("M6A_PREP_CHUNK_KB", str(chunk_kb))
    else:
        monkeypatch.delenv("M6A_PREP_CHUNK_KB", raising=False)
    data = F.good()[name]
    text, blocks = F.inflated(name)
    stats = {}
    got = _io.bgzf_inflate(write(tmp_path, name + ".gz", data), stats=stats)
    assert len(got) == len(text) and got == text, (name, chunk_kb)
    assert stats["n_blocks"] == len(blocks) and stats["compressed_bytes"] == len(data)
    assert stats["d2h_bytes"] == len(text) + 8                # the text and one status record: nothing per block


# ---- 2. malformed files: the statement's block and reason, then one correct call
@pytest.mark.parametrize("name", BAD)
def test_malformed_is_eformat_with_the_statements_block_and_reason(tmp_path, name):
    data, reason, index = F.malformed()[name]
    path = write(tmp_path, name + ".gz", data)
    want = "%s: BGZF block at byte %d: %s" % (path, F.offset_of(data, index), reason)
    with pytest.raises(_io.M6AIOError) as e:
        _io.bgzf_inflate(path)
    assert e.value.code == EFORMAT and message(e) == want
    with pytest.raises(_io.M6AIOError) as e:                  # and through the command's own entry: nothing is parsed
        _io.prep_sites(path, n_threads=2)
    assert e.value.code == EFORMAT and message(e) == want
    one_correct_call(tmp_path)


# ---- 3. the arrays of a compressed file are those of its text
def arrays(p):
    X, km, off = p.inputs()
    return dict(X=X, site_kmers=km, off=off, off_host=p.off, tx_pos=p.tx_pos, read_ids=p.read_ids, site_tx=p.site_tx, kmer7=p.kmer7,
                names=p.names, n=(p.n_sites, p.n_reads), rep=p.read_rep)


def same_arrays(a, b, tag):
    assert a.keys() == b.keys()
    for k in a:
        if isinstance(a[k], np.ndarray):
            assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), (tag, k)   # bit for bit
        else:
            assert a[k] == b[k], (tag, k)


@pytest.mark.parametrize("family, seed", SITE_CASES)
def test_sites_of_a_compressed_file_are_those_of_its_text(tmp_path, family, seed):
    c = G.case(family, seed)
    ev, _ = c.write(tmp_path)
    gz = write(tmp_path, "%s_%d.txt.gz" % (family, seed), bgzf.compress(c.data))
    blocks = B.inflate_file(open(gz, "rb").read())[1]
    args = (c.kw.get("readcount_min", 1), c.kw.get("readcount_max", 1000), c.kw.get("min_segment_count", 20))
    for norm in (None, hct116()):
        try:
            with _io.prep_sites(ev, *args, norm=norm, n_threads=2) as p:
                want = arrays(p)
                assert p.n_bgzf_blocks == 0 and p.compressed_bytes == 0 and p.ms_inflate == 0
        except _io.M6AIOError as plain:                       # the same code and words, the path apart (`short line at byte` is the text's)
            with pytest.raises(_io.M6AIOError) as e:
                _io.prep_sites(gz, *args, norm=norm, n_threads=2)
            assert e.value.code == plain.code and message(e).replace(gz, ev) == message(plain), (family, seed)
            one_correct_call(tmp_path)
            continue
        with _io.prep_sites(gz, *args, norm=norm, n_threads=2) as p:
            same_arrays(arrays(p), want, (family, seed, norm is not None))
            assert p.n_bgzf_blocks == len(blocks) and p.compressed_bytes == os.path.getsize(gz) and p.n_windows == 1


def test_the_declined_family_reaches_the_host_half(tmp_path):
    """the runs the device declines are read by the host half from the temporary file: the family has them, and their rows arrive"""
    c = G.case("declined", 1)
    assert G.FAMILIES["declined"].get("declined") and c.sites is not None
    gz = write(tmp_path, "declined.gz", bgzf.compress(c.data))
    before = set(os.listdir(os.environ.get("TMPDIR") or "/tmp"))
    with _io.prep_sites(gz, n_threads=2) as p:
        assert p.n_reads == len(c.sites["read_ids"]) and sorted(p.read_ids) == sorted(c.sites["read_ids"])
    left = set(os.listdir(os.environ.get("TMPDIR") or "/tmp")) - before
    assert not [f for f in left if f.startswith("m6a_declined_")]


# ---- 4. replicates: compressed, plain, compressed
def test_replicates_mix_compressed_and_plain(tmp_path):
    files = R.write(tmp_path, "three")
    mixed = list(files)
    for k in (0, 2):
        mixed[k] = write(tmp_path, "rep_%d.gz" % k, bgzf.compress(open(files[k], "rb").read()))
    with _io.prep_sites(files, 1, 1000, 1, n_threads=2) as p:
        want = arrays(p)
    with _io.prep_sites(mixed, 1, 1000, 1, n_threads=2) as p:
        same_arrays(arrays(p), want, "three")
        assert p.n_replicates == 3 and p.n_sites > 0
        assert p.compressed_bytes == os.path.getsize(mixed[0]) + os.path.getsize(mixed[2])
        assert p.n_bgzf_blocks == sum(len(B.inflate_file(open(m, "rb").read())[1]) for m in (mixed[0], mixed[2]))


# ---- 5. the command
@pytest.mark.parametrize("csv", ["host", "device"])
@pytest.mark.parametrize("n_files", [1, 3])
def test_command_writes_the_same_bytes_from_gz(tmp_path, n_files, csv):
    files = R.write(tmp_path, "three")[:n_files]
    gz = [write(tmp_path, "cli_%d.txt.gz" % k, bgzf.compress(open(f, "rb").read())) for k, f in enumerate(files)]
    a, b = str(tmp_path / "plain"), str(tmp_path / "gz")
    flags = ["--min_segment_count=1", "--csv", csv]
    run(["eventalign_inference", "--eventalign"] + files + ["--out_dir", a] + flags)
    run(["eventalign_inference", "--eventalign"] + gz + ["--out_dir", b] + flags)
    for fn in CSVS:
        assert os.path.getsize(os.path.join(a, fn)) > 100 and filecmp.cmp(os.path.join(a, fn), os.path.join(b, fn), shallow=False), fn


# ---- 6. refusals, each followed by one correct call
def test_refusals(tmp_path, monkeypatch):
    gz = write(tmp_path, "plain.gz", F.good()["family_plain"])
    with pytest.raises(_io.M6AIOError) as e:
        _io.prep_sites(gz, n_threads=2, window_kb=8)
    assert e.value.code == EINVAL and "windows over compressed input are not implemented" in message(e) and "fit resident" in message(e)
    one_correct_call(tmp_path)
    monkeypatch.setenv("M6A_PREP_WINDOW_KB", "8")
    with pytest.raises(_io.M6AIOError) as e:
        _io.prep_sites(gz, n_threads=2)
    assert e.value.code == EINVAL and "windows over compressed input are not implemented" in message(e)
    monkeypatch.delenv("M6A_PREP_WINDOW_KB")
    one_correct_call(tmp_path)
    with pytest.raises(_io.M6AIOError) as e:
        _io.prep_on_device(gz, 1)
    assert e.value.code == EFORMAT and "eventalign_inference" in message(e)
    one_correct_call(tmp_path)
    single = write(tmp_path, "single.gz", gzip.compress(G.case("plain", 1).data))
    for call in (lambda: _io.prep_sites(single, n_threads=2), lambda: _io.bgzf_inflate(single)):
        with pytest.raises(_io.M6AIOError) as e:
            call()
        assert e.value.code == EFORMAT and "is gzip but not BGZF" in message(e) and "bgzip" in message(e)
    one_correct_call(tmp_path)


# ---- 7. no per-block traffic, and the budget counts the compressed bytes
def test_traffic_and_budget(tmp_path, monkeypatch):
    c = G.case("plain", 1)
    ev, _ = c.write(tmp_path)
    gz = write(tmp_path, "plain.gz", F.good()["family_plain"])
    with _io.prep_sites(ev, n_threads=2) as p:
        plain_d2h, names = p.times()[1], sum(len(n) for n in p.names)
    with _io.prep_sites(gz, n_threads=2) as p:
        d2h = p.times()[1]
        print("d2h bytes: plain %d, compressed %d, names %d, segments %d" % (plain_d2h, d2h, names, len(segments_of(c))))
        assert plain_d2h <= d2h <= plain_d2h + names + 4096
        assert p.peak_bytes >= os.path.getsize(gz) + len(c.data)
    big = write(tmp_path, "big.gz", bgzf.compress(F.text(np.random.default_rng(5), 300000) * 8, level=1))
    monkeypatch.setenv("M6A_PREP_BUDGET_MB", "1")
    with pytest.raises(_io.M6AIOError) as e:
        _io.prep_sites(big, n_threads=2)
    assert e.value.code == ENOMEM
    monkeypatch.delenv("M6A_PREP_BUDGET_MB")
    one_correct_call(tmp_path)


def segments_of(c):
    """segments of equal contig bytes: each sends its name once (the plain path reads them from the file instead)"""
    tx = [r["tx"] for r in c.runs]
    return [t for i, t in enumerate(tx) if i == 0 or t != tx[i - 1]]
