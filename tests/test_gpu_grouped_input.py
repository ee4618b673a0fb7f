"""`eventalign_inference --grouped` (include/m6a.h: m6a_prep_group; tests/grouped_statement.py): on input whose transcripts each form
one stretch the batches' arrays, one after the other, are the whole-file call's, X bit for bit, every batch but the last ends on a
flush boundary, and both CSV files of the command are the bytes of the command without the flag -- at every window size, group size
and flush geometry, from a file and from a stream; on any other input the statement's error, the same at every size; and what is
kept on the device at once is a small part of the file's runs and rows.

No test here can hang: streams come from test_gpu_pipe_input.Feed (a daemon thread that always closes), `-` through a subprocess with
its stdin a pipe and a timeout."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import eventalign_gen as G
import grouped_gen as GG
import grouped_statement as GS
from m6anet_amd import _io
from test_eventalign_statement import hct116
from test_grouped_statement import GROUPED, NOT_GROUPED
from test_gpu_eventalign_inference import CSVS, REPO, site_args
from test_gpu_pipe_input import Feed
from test_gpu_prep_edges import one_correct_call

pytestmark = pytest.mark.gpu
WINDOWS_KB = [4, 8, 64]
GROUPS_KB = [4, 64]
GEOMETRY = [(1, 2), (3, 3), (16, 2)]


@functools.lru_cache(maxsize=None)
def source(name):
    """(bytes, the site filters) of a generated family at seed 1 or of one of grouped_gen's files"""
    if name in G.FAMILIES:
        c = G.case(name, 1)
        return c.data, site_args(c.kw)
    return GG.file(name), (1, 1000, 20)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("grouped")
    made = {}

    def path(name):
        if name not in made:
            made[name] = str(d / (name + ".txt"))
            with open(made[name], "wb") as f:
                f.write(source(name)[0])
        return made[name]
    return path


def arrays(p):
    """a handle's arrays with the transcripts by name"""
    X, km, off = p.inputs()
    assert np.array_equal(off, p.off) and p.off[0] == 0 and p.off[-1] == p.n_reads == len(X)
    return dict(X=X.view(np.uint32), km=km, reads=np.diff(p.off), tx=[p.names[t] for t in p.site_tx], tx_pos=p.tx_pos, kmer7=p.kmer7,
                read_ids=p.read_ids.view(np.uint64), read_rep=p.read_rep)


_whole = {}


def whole(files, name):
    """the whole-file call's arrays, computed once per file"""
    if name not in _whole:
        with _io.prep_sites(files(name), *source(name)[1], norm=hct116(), n_threads=2) as p:
            _whole[name] = arrays(p)
    return _whole[name]


def batches(path, args, **kw):
    """([arrays of every batch], [first_site of every batch], counts)"""
    out, firsts = [], []
    with _io.prep_sites_grouped(path, *args, norm=hct116(), n_threads=2, **kw) as g:
        for p in g:
            out.append(arrays(p))
            firsts.append(g.first_site)
        return out, firsts, g.counts()


def joined(parts):
    if not parts:
        return None
    return {k: sum((a[k] for a in parts), []) if k == "tx" else np.concatenate([a[k] for a in parts]) for k in parts[0]}


def assert_batches_are_the_whole(parts, firsts, counts, want, bs, spb, tag):
    n = [len(a["tx"]) for a in parts]
    assert all(n), tag                                                          # a batch without a site is not delivered
    assert firsts == [int(x) for x in np.cumsum([0] + n)[:-1]], tag                # first_site is the running sum
    for first, k in list(zip(firsts, n))[:-1]:                                  # every batch but the last ends on a flush boundary
        end = first + k
        assert end % bs == 0 and (end // bs) % spb != 0, (tag, end)
    got = joined(parts)
    if got is None:
        assert len(want["tx"]) == 0, tag
    else:
        assert got["tx"] == want["tx"], tag
        for k in want:
            if k != "tx":
                assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (tag, k)
    assert counts["n_batches"] == len(parts) and (not parts or (counts["n_sites"], counts["first_site"]) == (n[-1], firsts[-1])), tag
    assert counts["max_kept_runs"] <= counts["total_runs"] and counts["max_kept_rows"] <= counts["total_rows"], tag


# ---- 1. equal arrays --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group_kb", GROUPS_KB)
@pytest.mark.parametrize("window_kb", WINDOWS_KB)
@pytest.mark.parametrize("name", [f for f in GROUPED] + list(GG.GROUPED_FILES))
def test_the_batches_are_the_whole_file_call(files, name, window_kb, group_kb):
    want = whole(files, name)
    for bs, spb in GEOMETRY:
        tag = (name, window_kb, group_kb, bs, spb)
        parts, firsts, counts = batches(files(name), source(name)[1], window_kb=window_kb, group_kb=group_kb, batch_size=bs, save_per_batch=spb)
        assert_batches_are_the_whole(parts, firsts, counts, want, bs, spb, tag)
        assert counts["group_bytes"] == group_kb << 10 and counts["stream_bytes"] == 0 and counts["window_bytes"] >= window_kb << 10, tag
        if name == "many" and (bs, spb) == (1, 2):                              # a condition, so that the test cannot pass on a single batch
            assert counts["n_batches"] >= 4, tag
        if name == "tail" and (bs, spb) == (3, 3):                              # 13 sites: the last batch holds the short group
            assert len(want["tx"]) == 13 and (firsts[-1] + len(parts[-1]["tx"])) == 13, tag


# ---- 2. the same from a FIFO ------------------------------------------------------------------------------------------------------------
STREAMS = [("combine", 1, 4, 4), ("combine", 7, 4, 4), ("combine", 65537, 4, 4), ("declined", 7, 4, 4), ("many", 65537, 8, 8), ("tail", 65537, 64, 4)]


@pytest.mark.parametrize("name, piece, window_kb, group_kb", STREAMS)
def test_a_stream_gives_the_files_batches_and_counters(tmp_path, files, name, piece, window_kb, group_kb):
    data, args = source(name)
    kw = dict(window_kb=window_kb, group_kb=group_kb, batch_size=1, save_per_batch=2)
    want_parts, want_firsts, want_counts = batches(files(name), args, **kw)
    feed = Feed(tmp_path, data, piece)
    try:
        parts, firsts, counts = batches(feed.path, args, **kw)
    finally:
        feed.done()
    assert_batches_are_the_whole(parts, firsts, counts, whole(files, name), 1, 2, (name, piece))
    assert firsts == want_firsts and [len(a["tx"]) for a in parts] == [len(a["tx"]) for a in want_parts]
    assert counts["stream_bytes"] == len(data) and want_counts["stream_bytes"] == 0
    for k in ("n_batches", "n_sites", "n_reads", "first_site", "max_kept_runs", "max_kept_rows", "total_runs", "total_rows", "n_windows",
              "window_bytes", "group_bytes"):
        assert counts[k] == want_counts[k], (name, piece, k)


# ---- 3. not grouped ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NOT_GROUPED + ["moved"])
def test_input_that_is_not_grouped_is_the_statements_error_at_every_size(tmp_path, files, name):
    data, args = source(name)
    offender, start = GS.offender(data)
    if name == "moved":
        assert (offender, start) == GG.moved_offender()
    path = files(name)
    want = "m6a_prep error -7: " + GS.error_text(path, offender, start)
    for window_kb in WINDOWS_KB:
        for group_kb in GROUPS_KB:
            with pytest.raises(_io.M6AIOError) as e:
                batches(path, args, window_kb=window_kb, group_kb=group_kb, batch_size=1, save_per_batch=2)
            assert e.value.code == _io.prep_sites._CODES[-7] and str(e.value) == want, (name, window_kb, group_kb, str(e.value))
    one_correct_call(tmp_path)


# ---- 4. the command ---------------------------------------------------------------------------------------------------------------------
QUICK = ["--num_iterations", "50", "--n_processes", "2"]
TAIL = ["--drop_unflushed_tail", "--batch_size", "8", "--save_per_batch", "3", "--seed", "5"]
COMMANDS = [("host_file", ["--csv", "host"], False), ("device_file", ["--csv", "device"], False), ("host_tail_file", ["--csv", "host"] + TAIL, False),
            ("device_tail_stdin", ["--csv", "device"] + TAIL, True), ("expected_stdin", ["--csv", "host", "--site_proba", "expected"], True)]


def command(flags, ev, out, stdin=None, env=None, check=True):
    argv = [sys.executable, "-m", "m6anet_amd", "eventalign_inference", "--eventalign", "-" if stdin else ev, "--out_dir", out] + QUICK + flags
    feed = dict(input=open(stdin, "rb").read()) if stdin else dict(stdin=subprocess.DEVNULL)         # a pipe: the text comes once
    return subprocess.run(argv, cwd=REPO, timeout=600, env=env, check=check, stdout=subprocess.PIPE, stderr=subprocess.PIPE, **feed)


@pytest.mark.parametrize("tag, flags, stdin", COMMANDS, ids=[c[0] for c in COMMANDS])
def test_the_command_writes_the_bytes_of_the_command_without_the_flag(tmp_path, files, tag, flags, stdin):
    import json
    ev = files("many")
    plain, grouped = str(tmp_path / "plain"), str(tmp_path / "grouped")
    command(flags, ev, plain)
    env = dict(os.environ, M6A_PREP_WINDOW_KB="64", M6A_PREP_GROUP_KB="16", M6A_EVENTALIGN_TIMES="1")
    r = command(flags + ["--grouped"], ev, grouped, stdin=ev if stdin else None, env=env)
    for fn in CSVS:
        a, b = open(os.path.join(plain, fn), "rb").read(), open(os.path.join(grouped, fn), "rb").read()
        assert len(a.splitlines()) > 20 and a == b, (tag, fn)
    (line,) = [l for l in r.stdout.decode().splitlines() if l.startswith("M6A_TIMES ")]
    t = json.loads(line[len("M6A_TIMES "):])
    assert t["n_batches"] >= 4 and t["group_bytes"] == 16 << 10 and 0 < t["max_kept_rows"] < t["total_rows"] and t["max_kept_runs"] > 0, t
    assert (t["stream_bytes"] == os.path.getsize(ev)) == bool(stdin)


def test_the_command_on_input_that_is_not_grouped_leaves_no_csv(tmp_path, files):
    """the offender comes after a third of the file: rows had been written when the error came, and both files are gone afterwards"""
    ev = files("moved")
    out = str(tmp_path / "out")
    env = dict(os.environ, M6A_PREP_WINDOW_KB="64", M6A_PREP_GROUP_KB="16")
    r = command(["--grouped"], ev, out, env=env, check=False)
    name, start = GG.moved_offender()
    assert r.returncode != 0 and GS.error_text(ev, name, start) in r.stderr.decode(), r.stderr.decode()[-2000:]
    assert os.path.isdir(out) and not any(os.path.exists(os.path.join(out, fn)) for fn in CSVS)


def test_the_command_on_a_file_without_a_site_leaves_what_the_default_leaves(tmp_path, files):
    """the two header lines, then the loader's error"""
    ev = files("windows_2")
    plain, grouped = str(tmp_path / "plain"), str(tmp_path / "grouped")
    a = command([], ev, plain, check=False)
    b = command(["--grouped"], ev, grouped, env=dict(os.environ, M6A_PREP_WINDOW_KB="4", M6A_PREP_GROUP_KB="4"), check=False)
    assert a.returncode != 0 and b.returncode != 0
    assert "no site with at least 20 reads" in a.stderr.decode() and "no site with at least 20 reads" in b.stderr.decode()
    for fn in CSVS:
        text = open(os.path.join(grouped, fn), "rb").read()
        assert text == open(os.path.join(plain, fn), "rb").read() and text.count(b"\n") == 1, fn


# ---- 5. bounded -------------------------------------------------------------------------------------------------------------------------
def test_what_is_kept_at_once_is_a_small_part_of_the_file(files):
    """one open transcript (1 / 32), less than one group size of closed rows and one window's worth: about 4 % of the file's rows"""
    name = "many"
    parts, firsts, c = batches(files(name), source(name)[1], window_kb=8, group_kb=8, batch_size=16, save_per_batch=2)
    assert_batches_are_the_whole(parts, firsts, c, whole(files, name), 16, 2, "bounded")
    with _io.prep_sites(files(name), *source(name)[1], norm=hct116(), n_threads=2, window_kb=8) as p:
        windowed_peak, n_windows = p.peak_bytes, p.n_windows
    print("kept at once: %d of %d rows, %d of %d runs; peak %d B grouped, %d B in windows over the whole file; %d batches, %d windows"
          % (c["max_kept_rows"], c["total_rows"], c["max_kept_runs"], c["total_runs"], c["peak_bytes"], windowed_peak, c["n_batches"], c["n_windows"]))
    assert c["total_rows"] > 2000 and c["total_runs"] >= 32 * 20 and c["n_windows"] == n_windows
    assert c["max_kept_rows"] < c["total_rows"] / 4
    assert c["max_kept_runs"] < c["total_runs"] / 4
    assert 0 < c["peak_bytes"] < windowed_peak


# ---- 6. one transcript ------------------------------------------------------------------------------------------------------------------
def test_a_file_of_one_transcript_is_one_batch_at_the_end(files):
    want = whole(files, "one")
    for window_kb in WINDOWS_KB:
        parts, firsts, c = batches(files("one"), source("one")[1], window_kb=window_kb, group_kb=4, batch_size=1, save_per_batch=2)
        assert len(parts) == 1 and firsts == [0] and c["n_batches"] == 1 and c["n_windows"] > 1, window_kb
        assert_batches_are_the_whole(parts, firsts, c, want, 1, 2, window_kb)


def test_one_batch_at_a_time_and_no_compressed_input(tmp_path, files):
    """asking for the next batch while one is alive is M6A_EINVAL; BGZF content is refused with the windows' wording"""
    import ctypes as C
    with _io.prep_sites_grouped(files("many"), norm=hct116(), n_threads=2, window_kb=8, group_kb=8, batch_size=1, save_per_batch=2) as g:
        first = next(g)
        h = C.c_void_p()
        assert g._L.m6a_prep_group_next(g._g, C.byref(h)) == -1 and not h and b"still alive" in g._L.m6a_prep_last_error()
        assert first.n_sites > 0 and next(g).n_sites > 0                        # the iterator frees the batch at hand first
    from m6anet_amd import bgzf
    gz = str(tmp_path / "many.txt.gz")
    bgzf.compress_file(files("many"), gz)
    with pytest.raises(_io.M6AIOError) as e:
        _io.prep_sites_grouped(gz, norm=hct116(), n_threads=2, window_kb=8)
    assert e.value.code == -1 and "windows over compressed input are not implemented" in str(e.value)
