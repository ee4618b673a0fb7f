"""bgzf_inflate_kernel and bgzf_crc_kernel (m6anet_amd/csrc/m6a_bgzf.h) against zlib and the plain statement (tests/bgzf_statement.py)
on the generated corpus of tests/deflate_gen.py: every good stream, the match-copy grid, a sample of the damaged streams, one flipped
output byte at every edge of the CRC kernel's 64 parts, and the upload's 4 KB chunk edges.  Everything is byte for byte or word for
word.  These exact bytes went through the host build of the same decode core and through tests/bgzf_core_main.cpp under ASan and
UBSan first (tests/test_bgzf_generated.py, not marked gpu): a malformed stream reaches a device only after the CPU has shown that the
core gives a reason for it and touches nothing outside its buffers."""
import gzip
import time

import pytest

import bgzf_statement as B
import deflate_gen as D
from m6anet_amd import _io, bgzf
from test_gpu_bgzf import EFORMAT, message, one_correct_call, write

pytestmark = pytest.mark.gpu
GROUPS = list(B.REASONS) + ["accepted"]


def chunked(monkeypatch, chunk_kb):
    if chunk_kb:
        monkeypatch.setenv("M6A_PREP_CHUNK_KB", str(chunk_kb))
    else:
        monkeypatch.delenv("M6A_PREP_CHUNK_KB", raising=False)


def refused(path, offset, reason):
    with pytest.raises(_io.M6AIOError) as e:
        _io.bgzf_inflate(path)
    assert e.value.code == EFORMAT and message(e) == "%s: BGZF block at byte %d: %s" % (path, offset, reason)


# ---- 1. every generated stream, about 256 blocks to a file: zlib's text
@pytest.mark.parametrize("chunk_kb", [None, 4])
def test_inflate_is_zlib_on_the_whole_corpus(tmp_path, monkeypatch, chunk_kb):
    chunked(monkeypatch, chunk_kb)
    n = 0
    for k, (data, text, n_blocks) in enumerate(D.packed(D.corpus())):
        stats = {}
        t0 = time.perf_counter()
        got = _io.bgzf_inflate(write(tmp_path, "corpus_%d.gz" % k, data), stats=stats)
        print("file %d: %d blocks, %d -> %d bytes, %.1f ms" % (k, n_blocks, len(data), len(text), 1e3 * (time.perf_counter() - t0)))
        assert len(got) == len(text) and got == text == gzip.decompress(data), (k, chunk_kb)
        assert stats["n_blocks"] == n_blocks and stats["compressed_bytes"] == len(data)
        n += n_blocks - 1
    assert n == len(D.corpus())                           # no stream generated on the CPU is left out


# ---- 2. the all-lane match copy, one case per (distance, length)
@pytest.mark.parametrize("dist, length", [(d, n) for d in D.GRID_D for n in D.GRID_L])
def test_match_copy_grid(tmp_path, dist, length):
    s = D.grid()[dist, length]
    assert "grid_%d_%d" % (dist, length) in s.features and "dist_eq_pos" in s.features
    got = _io.bgzf_inflate(write(tmp_path, "grid.gz", D.member(s) + bgzf.EOF_MARKER))
    assert got == s.data, (dist, length)


# ---- 3. damaged streams: the statement's block and reason, word for word; then one correct call
@pytest.mark.parametrize("group", GROUPS)
def test_mutants_give_the_statements_message(tmp_path, group):
    mutants, verdicts, picked = D.all_mutants(), D.verdicts(), D.sample_by_reason()[group]
    assert len(picked) >= 3 and sum(map(len, D.sample_by_reason().values())) <= 300
    t0 = time.perf_counter()
    for i in picked:
        data = D.in_file(mutants[i])
        path = write(tmp_path, "mutant.gz", data)
        if verdicts[i] is None:
            assert group == "accepted" and _io.bgzf_inflate(path) == D.statement_on(data), mutants[i].name
        else:
            assert verdicts[i][1] == group
            refused(path, *verdicts[i])
    print("%s: %d mutants, %.1f ms a call" % (group, len(picked), 1e3 * (time.perf_counter() - t0) / len(picked)))
    one_correct_call(tmp_path)


# ---- 4. every output byte is under the CRC
@pytest.mark.parametrize("name", [str(n) for n in D.CRC_SIZES] + ["compressible"])
def test_one_flipped_byte_is_a_crc_mismatch_wherever_it_lies(tmp_path, name):
    data, files = D.crc_cases()[name]
    assert [p for p, _ in files] == D.crc_positions(len(data))
    for p, file in files:
        refused(write(tmp_path, "crc.gz", file), len(D.around()[0]), B.CRC)
    one_correct_call(tmp_path)


# ---- 5. the upload's chunks: headers and footers across a chunk's end at each of their bytes, files that end on one, cut files
def test_chunk_edges(tmp_path, monkeypatch):
    chunked(monkeypatch, 4)
    cases = D.chunk_cases()
    assert sum(name.startswith("header_at_") for name in cases) == 41 and sum(name.startswith("footer_at_") for name in cases) == 9
    for name, data in cases.items():
        want = D.statement_on(data)
        path = write(tmp_path, "chunk.gz", data)
        if isinstance(want, bytes):
            stats = {}
            assert _io.bgzf_inflate(path, stats=stats) == want, name
            assert stats["n_blocks"] == len(B.inflate_file(data)[1])
        else:
            assert name.startswith("cut_in_") and want[1] == (B.HEADER if name.startswith("cut_in_header") else B.BSIZE)
            refused(path, *want)
    one_correct_call(tmp_path)
