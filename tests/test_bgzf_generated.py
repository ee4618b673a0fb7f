"""The BGZF decode core against zlib on generated and damaged streams, on the CPU.  tests/deflate_gen.py writes deflate that covers the
format (its `features` records prove it) and damages it; zlib is the judge of the generator and of the plain statement
(tests/bgzf_statement.py), and the statement is the judge of the decode core the HIP kernels compile (m6anet_amd/csrc/m6a_bgzf.h): through
libm6a_io.so's m6a_io_bgzf_inflate, and through tests/bgzf_core_main.cpp, a program of its own built here with ASan and UBSan that
also feeds the block walk in pieces of every size.  Every byte string tests/test_gpu_bgzf_generated.py sends to a device goes through
both here first."""
import collections
import gzip
import os
import re
import subprocess
import time
import zlib

import pytest

import bgzf_fixtures as F
import bgzf_statement as B
import deflate_gen as D
from m6anet_amd import _io, bgzf

HERE = os.path.dirname(os.path.abspath(__file__))
EFORMAT = -4


def write(tmp_path, name, data):
    p = tmp_path / name
    p.write_bytes(data)
    return str(p)


def host_core(path):
    """the host core's text, or (offset, reason) parsed from its message"""
    try:
        return _io.bgzf_inflate_host(path)
    except _io.M6AIOError as e:
        m = re.search(re.escape(path) + r": BGZF block at byte (\d+): (.*)$", str(e))
        assert e.code == EFORMAT and m, str(e)
        return int(m.group(1)), m.group(2)


# ---- the generator
def test_generator_against_zlib():
    """zlib inflates every generated stream to the generator's own expansion, and ends where the stream ends"""
    for s in D.corpus():
        d = zlib.decompressobj(-15)
        assert d.decompress(s.body) == s.data and d.eof and not d.unused_data, s.name
        assert D.zlib_accepts(D.member(s)), s.name


def test_corpus_reaches_every_listed_feature():
    reached = collections.Counter(f for s in D.corpus() for f in s.features)
    print("features reached (streams):", ", ".join("%s %d" % (f, reached[f]) for f in D.FEATURES))
    assert not [f for f in D.FEATURES if not reached[f]]
    assert all(("grid_%d_%d" % k) in s.features for k, s in D.grid().items())
    sizes = sorted(len(s.data) for s in D.corpus())
    assert sizes[-3] <= 8192 and sizes[-2:] == [65535, 65536]          # a few KB each, the two full-size members apart


# ---- good streams
def test_statement_and_host_core_on_good_streams(tmp_path):
    n = 0
    for k, (data, text, n_blocks) in enumerate(D.packed(D.corpus())):
        got, blocks = B.inflate_file(data)
        assert got == text == gzip.decompress(data) and len(blocks) == n_blocks, k
        assert host_core(write(tmp_path, "good_%d.gz" % k, data)) == got, k
        n += n_blocks - 1
    assert n == len(D.corpus())
    print("good streams: %d in %d files" % (n, k + 1))


def test_host_core_on_the_match_copy_grid(tmp_path):
    """each (distance, length) alone in its file, as the device sees them: a distance equal to the bytes so far, then the same match again"""
    for (dist, length), s in D.grid().items():
        assert {"grid_%d_%d" % (dist, length), "dist_eq_pos"} <= s.features and B.inflate_file(D.member(s))[0] == s.data
        assert host_core(write(tmp_path, "grid.gz", D.member(s) + bgzf.EOF_MARKER)) == s.data, (dist, length)


# ---- damaged streams
def test_statement_refuses_the_mutants_zlib_refuses():
    """every mutant: zlib accepts when decompressobj(-15) reaches eof with nothing unused, gives ISIZE bytes and the CRC matches.
    gzip does not read BSIZE, so the mutants of that field alone are the block chain's and have no verdict of zlib's."""
    n = 0
    for m, v in zip(D.all_mutants(), D.verdicts()):
        if m.name.startswith("header/bsize"):
            continue
        if m.name.startswith("header/"):                  # the magic bytes and ISIZE are gzip's to judge, on the file
            with pytest.raises((OSError, EOFError, zlib.error)):
                gzip.decompress(D.in_file(m))
            assert v is not None
        else:
            assert D.zlib_accepts(m.block) == (v is None), (m.name, v)
        n += 1
    assert n >= len(D.all_mutants()) - 6


def test_host_core_is_the_statement_on_every_mutant(tmp_path):
    g0 = D.around()[0]
    count = collections.Counter()
    for i, (m, v) in enumerate(zip(D.all_mutants(), D.verdicts())):
        got = host_core(write(tmp_path, "m.gz", D.in_file(m)))
        if v is None:
            assert got == D.statement_on(D.in_file(m)), m.name
            count["accepted"] += 1
        else:
            assert got == v and v[0] == len(g0), (m.name, got, v)
            count[v[1]] += 1
    print("streams %d, mutants %d" % (len(D.corpus()), len(D.all_mutants())))
    for reason in B.REASONS + ("accepted",):
        print("  %-50s %d" % (reason, count[reason]))
    assert sum(count.values()) == len(D.all_mutants()) == len(D.corpus()) * D.N_MUTANTS + len(D.directed()) + len(D.header_level())
    assert all(count[reason] >= 3 for reason in B.REASONS), count
    assert all(len(idx) >= 3 for reason, idx in D.sample_by_reason().items() if reason != "accepted")
    assert sum(map(len, D.sample_by_reason().values())) <= 300


def test_directed_mutants_give_their_reasons():
    """what random damage does not reach is reached on purpose"""
    want = {"literal_length_code_286": B.SYMBOL, "literal_length_code_287": B.SYMBOL, "distance_code_30": B.SYMBOL, "distance_code_31": B.SYMBOL,
            "unused_code_of_a_single_distance_code": B.SYMBOL, "first_code_length_symbol_16": B.CODELEN, "repeat_past_hlit_and_hdist": B.CODELEN,
            "zero_repeat_past_hlit_and_hdist": B.CODELEN, "zeroed_end_of_block_length": B.CODELEN, "hclen_4": B.CODELEN,
            "distance_one_byte_too_far": B.DISTANCE, "distance_one_byte_too_far_dynamic": B.DISTANCE, "block_type_3": B.BTYPE,
            "block_type_3_not_last": B.BTYPE, "wrong_nlen": B.STORED, "nlen_is_len": B.STORED}
    seen = collections.Counter()
    for m, v in zip(D.all_mutants(), D.verdicts()):
        if m.name.startswith("directed/") and "/isize_" not in m.name:
            kind = m.name.split("/")[1].rsplit("_", 1)[0]
            assert v is not None and v[1] == want[kind], (m.name, v)
            seen[kind] += 1
        elif m.name.startswith("directed/"):
            assert v is not None and v[1] == (B.OVERFLOW if m.name.endswith("-1") else B.LENGTH), (m.name, v)
            seen["isize"] += 1
    assert set(seen) == set(want) | {"isize"} and all(n >= 3 for n in seen.values())


# ---- every output byte is under the CRC; the upload's chunk edges (the files of the GPU tests)
def test_host_core_refuses_one_flipped_byte_wherever_it_lies(tmp_path):
    g0 = D.around()[0]
    for name, (data, files) in D.crc_cases().items():
        assert len(files) >= (1 if len(data) == 1 else 2)
        for p, file in files:
            assert D.statement_on(file) == (len(g0), B.CRC), (name, p)
            assert host_core(write(tmp_path, "crc.gz", file)) == (len(g0), B.CRC), (name, p)


def test_statement_and_host_core_at_the_chunk_edges(tmp_path):
    cases = D.chunk_cases()
    for name, data in cases.items():
        want = D.statement_on(data)
        if name.startswith("cut_in_"):
            first = int(name.split("_")[3])
            assert want == (first, B.HEADER if name.startswith("cut_in_header") else B.BSIZE), name
        else:
            assert want == gzip.decompress(data), name
        assert host_core(write(tmp_path, "chunk.gz", data)) == want, name
    assert len(cases["ends_on_a_chunk"]) == 2 * D.CHUNK and len(cases["one_block_is_one_chunk"]) == D.CHUNK
    assert len(cases["marker_ends_on_a_chunk"]) == 2 * D.CHUNK


# ---- the core as a program of its own, under ASan and UBSan, the block walk fed in pieces
def test_core_as_a_sanitized_program_of_its_own(tmp_path):
    exe = str(tmp_path / "bgzf_core")
    t0 = time.time()
    subprocess.run(["g++", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g", "-O1", "-std=c++17",
                    "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(HERE, "..", "m6anet_amd", "csrc"), os.path.join(HERE, "bgzf_core_main.cpp"),
                    "-o", exe], check=True, timeout=300)
    t_build = time.time() - t0
    files = {}                                            # name: (bytes, the statement's text or (offset, reason))
    for name, data in F.good().items():
        files["good_" + name] = (data, F.inflated(name)[0])
    for name, (data, reason, index) in F.malformed().items():
        files["malformed_" + name] = (data, (F.offset_of(data, index), reason))
    for k, (data, text, _) in enumerate(D.packed(D.corpus())):
        files["corpus_%d" % k] = (data, text)
    for i, (m, v) in enumerate(zip(D.all_mutants(), D.verdicts())):
        data = D.in_file(m)
        files["mutant_%d" % i] = (data, v if v else D.statement_on(data))
    for name, (_, crc_files) in D.crc_cases().items():
        for p, data in crc_files:
            files["crc_%s_%d" % (name, p)] = (data, (len(D.around()[0]), B.CRC))
    for name, data in list(D.chunk_cases().items()) + list(D.truncation_cases().items()):
        files[name] = (data, D.statement_on(data))
    assert sum(1 for name in files if name.startswith("truncated_")) >= 60
    names = sorted(files)
    for name in names:
        write(tmp_path, name, files[name][0])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    t0 = time.time()
    parts = [names[k::4] for k in range(4)]
    children = [subprocess.Popen([exe] + part, cwd=str(tmp_path), env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for part in parts]
    for part, child in zip(parts, children):
        out, err = child.communicate(timeout=600)
        assert child.returncode == 0 and not err, (child.returncode, out[-300:], err[-3000:])
        lines = out.splitlines()
        assert len(lines) == len(part)
        for name, line in zip(part, lines):
            want, f = files[name][1], line.split("\t")
            assert f[0] == name
            if isinstance(want, bytes):
                assert f[1:] == ["ok", str(len(want)), "%08x" % zlib.crc32(want)], (line, len(want))
            else:
                assert f[1:] == [str(want[0]), want[1]], (line, want)
    print("%d files through the sanitized program in %.1f s (built in %.1f s)" % (len(names), time.time() - t0, t_build))
