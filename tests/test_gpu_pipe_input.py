"""`eventalign_inference --eventalign -` and FIFOs (include/m6a.h: streams; m6a_prep.hip: front_stream): text that comes once and in
order gives what the same bytes in a regular file give at the same window size -- every array of the handle, X bit for bit, the
windows tests/window_statement.py states, every error's code and text -- whatever the pieces the writer delivers it in; the back half
gets its contig names and declined runs from what the windows saved; `--read_names`, replicates that mix files and streams, the
command with both CSV writers and with --compress; and what is refused is refused with a clear text and a correct call follows.

No test here can hang: a stream's writer is a daemon thread that opens the FIFO itself, swallows BrokenPipeError and always closes;
the main thread never opens a FIFO in blocking mode; `-` is tested through a subprocess with stdin=PIPE and a timeout."""
import json
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

import bgzf_statement as BS
import eventalign_gen as G
import eventalign_statement as S
import read_names_gen as NG
import replicate_fixtures as F
import window_statement as WS
from m6anet_amd import _io
from test_dataprep_rows import unpack
from test_eventalign_statement import hct116
from test_gpu_eventalign_inference import CSVS, REPO
from test_gpu_prep_edges import SITE_CASES, one_correct_call
from test_gpu_prep_windows import crafted_cuts, host_arrays, n_windows_of

pytestmark = pytest.mark.gpu


# ---- a stream --------------------------------------------------------------------------------------------------------------------
class Feed:
    """`data` through a FIFO under tmp_path.  The writer thread opens the FIFO (which waits for the reader), writes pieces of `piece`
    bytes (None: all at once) and closes; a reader that went away is a BrokenPipeError, swallowed."""
    count = 0

    def __init__(self, tmp_path, data, piece=None):
        Feed.count += 1
        self.path = str(tmp_path / ("stream_%d.fifo" % Feed.count))
        os.mkfifo(self.path)
        self.thread = threading.Thread(target=self.write, args=(bytes(data), piece), daemon=True)
        self.thread.start()

    def write(self, data, piece):
        fd = None
        try:
            fd = os.open(self.path, os.O_WRONLY)
            view, step = memoryview(data), piece or max(1, len(data))
            at = 0
            while at < len(view):
                at += os.write(fd, view[at:at + step])
        except BrokenPipeError:
            pass
        finally:
            if fd is not None:
                os.close(fd)

    def done(self):
        """after the reader's call.  A reader that failed before it opened the FIFO has left the writer in its open: a non-blocking
        open lets it go (it then meets a closed pipe), and nothing here waits for anything but the thread's own end."""
        if self.thread.is_alive():
            os.close(os.open(self.path, os.O_RDONLY | os.O_NONBLOCK))
        self.thread.join(timeout=30)
        assert not self.thread.is_alive()


def from_stream(tmp_path, data, *args, piece=None, **kw):
    """_io.prep_sites on `data` from a FIFO -> (arrays, the handle's counters); an M6AIOError carries the FIFO's path as stream_path"""
    feed = Feed(tmp_path, data, piece)
    try:
        with _io.prep_sites(feed.path, *args, **kw) as p:
            return host_arrays(p), dict(n_windows=p.n_windows, window_bytes=p.window_bytes, stream_bytes=p.stream_bytes, n_streams=p.n_streams,
                                        d2h=p.times()[1], read_names=p.read_names, read_ids=p.read_ids.copy(), n_sites=p.n_sites)
    except _io.M6AIOError as e:
        e.stream_path = feed.path
        raise
    finally:
        feed.done()


def from_file(path, *args, **kw):
    with _io.prep_sites(path, *args, **kw) as p:
        return host_arrays(p), dict(n_windows=p.n_windows, window_bytes=p.window_bytes, stream_bytes=p.stream_bytes, n_streams=p.n_streams,
                                    d2h=p.times()[1], read_names=p.read_names, read_ids=p.read_ids.copy(), n_sites=p.n_sites)


def same(a, b, tag):
    assert sorted(a) == sorted(b), tag
    for k in a:
        assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), (tag, k)


def stream_is_the_file(tmp_path, data, *args, tag="", piece=None, name="ev.txt", **kw):
    """the stream's arrays and windows are the file's, and the windows are the statement's; or both raise the same code and the same
    text with the path replaced.  Returns (the stream's counters, the file's), or None after an error."""
    ev = tmp_path / name
    ev.write_bytes(data)
    try:
        want, cw = from_file(str(ev), *args, **kw)
    except _io.M6AIOError as whole:
        with pytest.raises(_io.M6AIOError) as e:
            from_stream(tmp_path, data, *args, piece=piece, **kw)
        assert e.value.code == whole.code and str(e.value).replace(e.value.stream_path, str(ev)) == str(whole), (tag, str(e.value), str(whole))
        return None
    got, cg = from_stream(tmp_path, data, *args, piece=piece, **kw)
    same(got, want, tag)
    assert (cg["n_windows"], cg["window_bytes"]) == (cw["n_windows"], cw["window_bytes"]) == n_windows_of(data, kw["window_kb"]), tag
    assert (cg["stream_bytes"], cg["n_streams"]) == (len(data), 1) and (cw["stream_bytes"], cw["n_streams"]) == (0, 0), tag
    return cg, cw


# ---- 1. the generated families -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("window_kb", [4, 8, 64])
@pytest.mark.parametrize("family, seed", SITE_CASES)
def test_stream_is_the_windowed_file_on_every_family(tmp_path, family, seed, window_kb):
    c = G.case(family, seed)
    args = (c.kw.get("readcount_min", 1), c.kw.get("readcount_max", 1000), c.kw.get("min_segment_count", 20))
    for norm in (None, hct116()):
        r = stream_is_the_file(tmp_path, c.data, *args, tag=(family, seed, window_kb, norm is not None), norm=norm, n_threads=2, window_kb=window_kb)
        assert (r is None) == (c.error is not None), (family, seed)
        if r is None:
            one_correct_call(tmp_path)


# ---- 2. how the bytes arrive does not matter ----------------------------------------------------------------------------------------------
def test_pieces_of_any_size_give_the_same_arrays(tmp_path):
    """("combine", 1) at 4 KB windows grows a window: the growth appends to what is there, byte by byte if that is how they come"""
    c = G.case("combine", 1)
    for piece in (1, 7, 65537):
        cg, _ = stream_is_the_file(tmp_path, c.data, tag=piece, piece=piece, n_threads=2, window_kb=4)
        assert cg["window_bytes"] >= 32 << 10 and cg["n_sites"] > 0


# ---- 3. every kind of line on a cut ---------------------------------------------------------------------------------------------------------
def test_crafted_cuts_through_a_stream(tmp_path, monkeypatch):
    """a declined run that ends exactly on b + W and a contig change on a cut: the contig names and the declined run's bytes come from
    what the windows saved, the host half reads them from a temporary file, and the file is gone afterwards"""
    W = 8 << 10
    data, declined_read = crafted_cuts(W)
    wins = WS.windows(data, W)
    tmp = tmp_path / "tmpdir"
    tmp.mkdir()
    monkeypatch.setenv("TMPDIR", str(tmp))
    for norm in (None, hct116()):
        cg, _ = stream_is_the_file(tmp_path, data, 1, 24, 20, tag=("cuts", norm is not None), norm=norm, n_threads=2, window_kb=8)
        assert cg["n_windows"] == len(wins) >= 6 and declined_read in cg["read_ids"]
        assert os.listdir(str(tmp)) == []
    names, runs = S.index(data)
    (dec,) = [r for r in runs if r["read"] == declined_read]
    assert S.declines(data, dec) and any(w["e"] == w["b"] + W == dec["end"] for w in wins)
    prev, change = None, False                                # a contig change on a cut
    for w in wins:
        if w["runs"]:
            change = change or (prev is not None and w["names"][w["runs"][0]["tx"]] != prev)
            prev = w["names"][w["runs"][-1]["tx"]]
    assert change


# ---- 4. the last window ----------------------------------------------------------------------------------------------------------------------
def test_a_stream_that_ends_on_the_window_ends_there(tmp_path):
    """b + size == len(data): no byte follows, so the window is the last; one more byte and it is not.  The reader's one byte of
    lookahead decides it."""
    W = 8 << 10
    base, pad = G.case("plain", 1).data, 0
    assert base.endswith(b"\n")
    for _ in range(8):                                       # the last window's b stays where it is while the padding fills its size
        data = base + b"x" * pad + b"\n"
        wins = WS.windows(data, W)
        short = wins[-1]["b"] + wins[-1]["size"] - len(data)
        if short == 0:
            break
        pad += short
    assert short == 0 and b"\t" not in data[len(base):]
    more = data + b"x"
    n_exact, n_more = n_windows_of(data, 8), n_windows_of(more, 8)
    assert n_more != n_exact, (n_exact, n_more)              # the statement: that window is no longer the last, so it is cut or grows
    for name, d in (("exact", data), ("more", more)):
        cg, _ = stream_is_the_file(tmp_path, d, tag=name, n_threads=2, window_kb=8, name=name + ".txt")
        assert cg["n_sites"] > 0


# ---- 5. edges -------------------------------------------------------------------------------------------------------------------------------
def no_kept_run(W):
    """a run longer than 2 W between short ones (its window grows to 4 W), and more than W bytes of lines without a tab (a window
    that keeps no run and hands on at its last newline)"""
    rng = np.random.default_rng(5)
    f = G.File(rng)
    tx, long = G.Tx(rng, "EDGE", 12, (3,)), G.Tx(rng, "LONG", 12, ())
    for _ in range(3):                                       # window 0 is the header and lines without a tab
        f.raw(b"x" * (W // 2) + b"\n")
    G.site_reads(f, tx, 3, range(12), mismatch=0)
    start = f.size
    while f.size - start <= 2 * W + 512:
        f.line(long.name, 2, long.kmer(2), 500)
    G.site_reads(f, tx, 3, range(12, 26), mismatch=0)
    return f.bytes()


def test_edges(tmp_path):
    W = 4 << 10
    plain = G.case("plain", 1).data
    data = no_kept_run(W)
    wins = WS.windows(data, W)
    assert any(not w["runs"] for w in wins[:-1]) and max(w["size"] for w in wins) >= 4 * W
    for name, d, sites in (("header_only", G.HEADER, False), ("nothing", b"", None), ("no_newline_at_the_end", plain[:-1], True),
                           ("no_kept_run", data, True)):
        r = stream_is_the_file(tmp_path, d, tag=name, n_threads=2, window_kb=4, name=name + ".txt")
        assert (r is None) == (sites is None), name
        if r is not None:
            assert (r[0]["n_sites"] > 0) == sites, name
    with pytest.raises(_io.M6AIOError) as e:
        from_stream(tmp_path, b"", n_threads=2, window_kb=4)
    assert e.value.code == -4 and str(e.value).endswith(e.value.stream_path + ": no header line")
    one_correct_call(tmp_path)


# ---- 6. read names ------------------------------------------------------------------------------------------------------------------------
def test_read_names_from_a_stream(tmp_path):
    c = NG.case("windows")
    named, _ = c.write(tmp_path)
    want, cw = from_file(named, n_threads=2, window_kb=8, read_names=True)
    got, cg = from_stream(tmp_path, c.named, n_threads=2, window_kb=8, read_names=True, piece=4097)
    same(got, want, "names")
    assert cg["n_sites"] > 0 and cg["n_windows"] == cw["n_windows"] > 1
    for a, b in zip(cg["read_names"], cw["read_names"]):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    assert len(cg["read_names"][0]) == len(c.names)


# ---- 7. replicates that mix files and streams ----------------------------------------------------------------------------------------------
def test_replicates_of_files_and_streams(tmp_path):
    files = F.write(tmp_path, "three")
    norm = hct116()
    want, cw = from_file(files, 1, 1000, 1, norm=norm, n_threads=2, window_kb=64)
    feeds = [Feed(tmp_path, open(files[k], "rb").read(), piece=65537) for k in (0, 2)]
    try:
        with _io.prep_sites([feeds[0].path, files[1], feeds[1].path], 1, 1000, 1, norm=norm, n_threads=2, window_kb=64) as p:
            got = host_arrays(p)
            assert p.n_streams == 2 and p.stream_bytes == os.path.getsize(files[0]) + os.path.getsize(files[2]) and p.n_replicates == 3
            assert (p.n_windows, p.window_bytes) == (cw["n_windows"], cw["window_bytes"]) and p.n_sites > 0
    finally:
        for f in feeds:
            f.done()
    same(got, want, "three")
    assert cw["n_streams"] == 0


# ---- 8. the command --------------------------------------------------------------------------------------------------------------------------
def command(args, stdin=None, check=True):
    r = subprocess.run([sys.executable, "-m", "m6anet_amd", "eventalign_inference"] + args, cwd=REPO, timeout=600, input=stdin,
                       env=dict(os.environ, M6A_EVENTALIGN_TIMES="1"), stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert (r.returncode == 0) == check, r.stderr.decode()[-2000:]
    return r


def times_of(r):
    (line,) = [l for l in r.stdout.decode().splitlines() if l.startswith("M6A_TIMES ")]
    return json.loads(line[len("M6A_TIMES "):])


@pytest.fixture(scope="module")
def bundled(tmp_path_factory):
    d = tmp_path_factory.mktemp("pipe_cli")
    ev = unpack(d, "ref_tests_data")
    return d, ev, open(ev, "rb").read()


@pytest.mark.parametrize("csv", ["host", "device"])
def test_the_command_reads_its_standard_input(bundled, csv):
    d, ev, data = bundled
    flags = ["--n_processes", "4", "--num_iterations", "100", "--csv", csv, "--window_mb", "1"]
    whole, piped = str(d / ("file_" + csv)), str(d / ("stdin_" + csv))
    t_file = times_of(command(["--eventalign", ev, "--out_dir", whole] + flags))
    t = times_of(command(["--eventalign", "-", "--out_dir", piped] + flags, stdin=data))
    for fn in CSVS:
        a, b = open(os.path.join(whole, fn), "rb").read(), open(os.path.join(piped, fn), "rb").read()
        assert len(a) > 1000 and a == b, fn
    assert t["stream_bytes"] == len(data) and t["n_streams"] == 1 and (t_file["stream_bytes"], t_file["n_streams"]) == (0, 0)
    assert (t["n_windows"], t["window_bytes"]) == (t_file["n_windows"], t_file["window_bytes"]) and t["n_windows"] > 1


def test_the_command_compresses_what_it_read_from_its_standard_input(bundled):
    d, ev, data = bundled
    flags = ["--n_processes", "4", "--num_iterations", "100", "--csv", "device", "--window_mb", "1"]
    plain, packed = str(d / "file_plain"), str(d / "stdin_gz")
    command(["--eventalign", ev, "--out_dir", plain] + flags)
    t = times_of(command(["--eventalign", "-", "--out_dir", packed, "--compress"] + flags, stdin=data))
    assert t["n_streams"] == 1 and t["csv_writer"] == "device"
    for fn in CSVS:
        assert not os.path.exists(os.path.join(packed, fn))
        text, _ = BS.inflate_file(open(os.path.join(packed, fn + ".gz"), "rb").read())
        assert text == open(os.path.join(plain, fn), "rb").read(), fn


# ---- 9. refusals --------------------------------------------------------------------------------------------------------------------------
def test_refusals(tmp_path, bundled):
    with pytest.raises(_io.M6AIOError) as e:                  # gzip from a stream
        from_stream(tmp_path, b"\x1f\x8b\x08\x04" + bytes(200000), n_threads=2)
    assert e.value.code == -1 and "bgzip -dc" in str(e.value) and e.value.stream_path in str(e.value)
    one_correct_call(tmp_path)
    d, ev, data = bundled                                     # `-` twice: before anything is opened, so nothing reads the input
    out = str(tmp_path / "twice")
    r = command(["--eventalign", "-", "-", "--out_dir", out], stdin=data[:4096], check=False)
    assert b"`-`" in r.stderr and b"twice" in r.stderr and not any(os.path.exists(os.path.join(out, fn)) for fn in CSVS)
    one_correct_call(tmp_path)
    path = str(tmp_path / "never_opened.fifo")                # dataprep --device gpu: refused by what the path is, never opened
    os.mkfifo(path)
    for index in (None, str(tmp_path / "eventalign.index")):
        with pytest.raises(_io.M6AIOError) as e:
            _io.prep_on_device(path, 1, index_path=index)
        assert e.value.code == -1 and "is a stream" in str(e.value) and path in str(e.value)
    one_correct_call(tmp_path)


# ---- 10. traffic and budget ---------------------------------------------------------------------------------------------------------------
def test_a_stream_brings_back_its_segment_names_and_little_else(tmp_path):
    c = G.case("plain", 1)
    cg, cw = stream_is_the_file(tmp_path, c.data, tag="traffic", n_threads=2, window_kb=8)
    names = 0                                                 # the contig bytes of every segment: a window's first run, and each change
    for w in WS.windows(c.data, 8 << 10):
        for k, r in enumerate(w["runs"]):
            if k == 0 or r["tx"] != w["runs"][k - 1]["tx"]:
                names += len(w["names"][r["tx"]])
    print("d2h: stream %d B, windowed file %d B, segment names %d B, %d windows" % (cg["d2h"], cw["d2h"], names, cg["n_windows"]))
    assert cg["n_windows"] > 2 and names > 0
    assert cg["d2h"] <= cw["d2h"] + names + 4096


def test_a_stream_over_the_budget_is_out_of_memory(tmp_path, monkeypatch):
    data = G.case("plain", 1).data
    header, body = data[:data.find(b"\n") + 1], data[data.find(b"\n") + 1:]
    big = header + body * (2400000 // len(body) + 1)
    assert len(big) >= 2400000
    monkeypatch.setenv("M6A_PREP_BUDGET_MB", "1")
    with pytest.raises(_io.M6AIOError) as e:
        from_stream(tmp_path, big, n_threads=2, window_kb=1024)
    assert e.value.code == -2 and "--window_mb" in str(e.value)
    monkeypatch.delenv("M6A_PREP_BUDGET_MB")
    one_correct_call(tmp_path)
