"""BGZF on the CPU: the plain statement (tests/bgzf_statement.py) against zlib on every fixture of tests/bgzf_fixtures.py, and the
decode core the HIP kernels compile (m6anet_amd/csrc/m6a_bgzf.h, here through libm6a_io.so's m6a_io_bgzf_inflate) against the
statement -- the text, or the first bad block's offset and reason.  Every malformed stream goes through the core here, under the
sanitizers of tests/sanitize.sh, before tests/test_gpu_bgzf.py sends it to a device."""
import gzip
import subprocess
import sys
import zlib

import numpy as np
import pytest

import bgzf_fixtures as F
import bgzf_statement as B
from m6anet_amd import _io, bgzf

GOOD, BAD = sorted(F.good()), sorted(F.malformed())
BGZF_ONLY = {"bsize_past_the_end"}


def test_the_marker_is_the_specifications():
    assert F.good()["eof_only"] == bgzf.EOF_MARKER and len(bgzf.EOF_MARKER) == 28


@pytest.mark.parametrize("name", GOOD)
def test_statement_is_gzip_on_good_files(name):
    data = F.good()[name]
    text, blocks = F.inflated(name)
    assert text == gzip.decompress(data) and sum(b["isize"] for b in blocks) == len(text)


def test_fixtures_reach_their_edges():
    report = {name: F.inflated(name)[1] for name in F.good()}
    assert [b["types"] for b in report["stored"][:1]] == [[0, 0]] and len(F.good()["stored"]) == 65316 + 28
    assert report["fixed"][0]["types"] == [1] and report["dynamic"][0]["types"] == [2]
    a = report["all_A"][0]
    assert a["isize"] == 65536 and a["distance"] == 1 and a["length"] == 258
    f = report["far_match"][0]
    assert f["types"] == [2] and f["distance"] == 32768 and f["length"] == 258
    assert len(report["two_deflate_blocks"][0]["types"]) >= 2
    assert [b["isize"] for b in report["empty_in_the_middle"]] == [3000, 0, 3000, 0]
    assert len(report["small_300"]) == 301 and report["no_eof_marker"][-1]["isize"] > 0
    assert all(b["isize"] == 0xff00 for b in report["family_plain"][:-2])


@pytest.mark.parametrize("name", BAD)
def test_statement_refuses_what_zlib_refuses(name):
    data, reason, index = F.malformed()[name]
    with pytest.raises(B.Bad) as e:
        B.inflate_file(data)
    assert (e.value.offset, e.value.reason) == (F.offset_of(data, index), reason)
    if name not in BGZF_ONLY:                        # gzip does not read BSIZE: a fault in it alone is the chain's, not zlib's
        with pytest.raises((OSError, EOFError, zlib.error)):
            gzip.decompress(data)


def zlib_accepts(stream):
    d = zlib.decompressobj(-15)
    try:
        d.decompress(stream)
    except zlib.error:
        return False
    return d.eof


def test_code_length_sets_as_zlib(tmp_path):
    """seeded random literal/length and distance sets, sent through a complete code-length code and followed by the end-of-block
    code where there is one: the statement accepts exactly the streams zlib accepts, and the host build of the decode core
    (m6a_io_bgzf_inflate) gives the statement's verdict on each of them as a BGZF block"""
    rng = np.random.default_rng(7)
    seen = {True: 0, False: 0}
    for trial in range(400):
        kind = trial % 4
        if kind == 0:                                 # a complete set, then damaged in one place
            ll = F.flat_lengths(int(rng.integers(257, 287)))
            ll[int(rng.integers(0, len(ll)))] = int(rng.integers(0, 16))
            dd = F.flat_lengths(int(rng.integers(1, 31)))
        elif kind == 1:                               # sparse sets: single codes, none at all
            ll = [0] * 257
            for s in rng.choice(257, int(rng.integers(1, 4)), replace=False):
                ll[int(s)] = int(rng.integers(1, 3))
            ll[256] = int(rng.integers(0, 3))
            dd = [0] * int(rng.integers(1, 31))
            if rng.integers(0, 2):
                dd[int(rng.integers(0, len(dd)))] = int(rng.integers(1, 3))
        elif kind == 2:
            ll = F.flat_lengths(286)
            dd = F.flat_lengths(int(rng.integers(1, 31)))
            dd[int(rng.integers(0, len(dd)))] = int(rng.integers(0, 16))
        else:
            ll = [int(v) for v in rng.integers(0, 16, int(rng.integers(257, 287)))]
            dd = [int(v) for v in rng.integers(0, 16, int(rng.integers(1, 31)))]
        w = F.BitWriter().bits(1, 1).bits(2, 2)
        F.put_lengths(w, ll, dd)
        codes = F.codes_of(ll)
        if 256 in codes and codes[256][1] <= 15 and B.accepted(*B.code_of(ll)[1:]):
            w.code(*codes[256])
        stream = w.done()
        try:
            B.inflate(stream, 0)
            ours, want = True, None
        except B.Refused as e:
            ours, want = False, "BGZF block at byte 0: " + e.args[0]
        assert ours == zlib_accepts(stream), (trial, ll, dd)
        path = tmp_path / "set.gz"
        path.write_bytes(bgzf.wrap(stream, 0, 0))
        try:
            assert _io.bgzf_inflate_host(str(path)) == b"" and ours, (trial, ll, dd)
        except _io.M6AIOError as e:
            assert not ours and e.code == -4 and str(e).endswith("%s: %s" % (path, want)), (trial, ll, dd, str(e))
        seen[ours] += 1
    assert seen[True] > 20 and seen[False] > 20


def write(tmp_path, name, data):
    p = tmp_path / (name + ".gz")
    p.write_bytes(data)
    return str(p)


@pytest.mark.parametrize("name", GOOD)
def test_host_core_is_the_statement_on_good_files(tmp_path, name):
    data = F.good()[name]
    path = write(tmp_path, name, data)
    assert _io.bgzf_inflate_host(path) == F.inflated(name)[0]
    assert _io.is_bgzf(path) and B.is_bgzf(data)


@pytest.mark.parametrize("name", BAD)
def test_host_core_is_the_statement_on_malformed_files(tmp_path, name):
    data, reason, index = F.malformed()[name]
    path = write(tmp_path, name, data)
    with pytest.raises(_io.M6AIOError) as e:
        _io.bgzf_inflate_host(path)
    assert e.value.code == -4 and str(e.value).endswith("%s: BGZF block at byte %d: %s" % (path, F.offset_of(data, index), reason))


def test_host_core_carries_blocks_across_pieces(tmp_path):
    """the whole-file call is one piece; a file of 300 small blocks and one of full blocks give the same text block by block"""
    for name in ("small_300", "family_plain", "extra_subfields"):
        data = F.good()[name]
        assert _io.bgzf_inflate_host(write(tmp_path, name, data)) == gzip.decompress(data)


def test_gzip_that_is_not_bgzf_and_plain_text(tmp_path):
    path = write(tmp_path, "single", gzip.compress(b"contig\tposition\n" * 50))
    assert not _io.is_bgzf(path) and bgzf.is_gzip(path)
    with pytest.raises(_io.M6AIOError) as e:
        _io.bgzf_inflate_host(path)
    assert e.value.code == -4 and "is gzip but not BGZF" in str(e.value) and "bgzip" in str(e.value)
    plain = tmp_path / "plain.txt"
    plain.write_bytes(b"contig\tposition\n")
    assert not _io.is_bgzf(str(plain)) and not bgzf.is_gzip(str(plain))
    with pytest.raises(_io.M6AIOError) as e:
        _io.bgzf_inflate_host(str(plain))
    assert e.value.code == -4 and "not a gzip file" in str(e.value)


def test_bgzip_subcommand(tmp_path):
    rng = np.random.default_rng(3)
    data = F.text(rng, 200000)
    src = tmp_path / "sample.txt"
    src.write_bytes(data)
    subprocess.run([sys.executable, "-m", "m6anet_amd", "bgzip", str(src), "--level", "4", "--n_processes", "2"], check=True, timeout=120)
    out = (tmp_path / "sample.txt.gz").read_bytes()
    assert out.endswith(bgzf.EOF_MARKER) and gzip.decompress(out) == data
    text, blocks = B.inflate_file(out)
    assert text == data and [b["isize"] for b in blocks[:3]] == [0xff00] * 3 and _io.bgzf_inflate_host(str(src) + ".gz") == data
