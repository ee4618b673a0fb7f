"""The front half in windows (include/m6a.h: m6a_prep_sites_build_windows; M6A_PREP_WINDOW_KB, `eventalign_inference --window_mb`)
held to what the whole-file mode is held to: on every generated family, three seeds and windows of 4, 8, 12 and 64 KB the table
and the sites are the statement's bit for bit, the device cuts where tests/window_statement.py cuts, errors keep their code, text
and byte offset, a crafted file puts every kind of line on a cut, replicates pool to the same arrays, the command writes the same
bytes, a file over the whole-file budget goes through, and a window costs the host link a fixed handful of bytes."""
import filecmp
import os

import numpy as np
import pytest

import eventalign_gen as G
import eventalign_statement as S
import replicate_fixtures as F
import window_statement as WS
from m6anet_amd import _io
from test_eventalign_statement import assert_sites_are_the_statement, assert_table_is_the_statement, hct116, message
from test_gpu_eventalign_inference import CSVS, arrays_equal_the_loader, run, unpack
from test_gpu_prep_edges import CASES, SITE_CASES, one_correct_call

pytestmark = pytest.mark.gpu
WINDOWS_KB = [4, 8, 12, 64]


def n_windows_of(data, window_kb):
    wins = WS.windows(data, window_kb << 10)
    return len(wins), max(w["size"] for w in wins)


@pytest.mark.parametrize("window_kb", WINDOWS_KB)
@pytest.mark.parametrize("family, seed", [(f, s) for f, s in CASES if f != "midline"])
def test_device_table_is_the_statement_in_windows(tmp_path, monkeypatch, family, seed, window_kb):
    c, spec = G.case(family, seed), G.FAMILIES[family]
    ev, _ = c.write(tmp_path)
    if "error" in spec:                                       # the same code and the same byte offset as the whole file's
        with pytest.raises(_io.M6AIOError) as whole:
            _io.prep_on_device(ev, c.nn)
        monkeypatch.setenv("M6A_PREP_WINDOW_KB", str(window_kb))
        with pytest.raises(_io.M6AIOError) as e:
            _io.prep_on_device(ev, c.nn)
        assert e.value.code == whole.value.code == spec["error"][0] and message(e) == message(whole) == c.error[1]
        monkeypatch.delenv("M6A_PREP_WINDOW_KB")
        one_correct_call(tmp_path)
        return
    monkeypatch.setenv("M6A_PREP_WINDOW_KB", str(window_kb))
    with _io.prep_on_device(ev, c.nn) as t:
        a = _io.table_arrays(t.contents)
    status = assert_table_is_the_statement(a, c, (family, seed, window_kb))
    assert [bool(s) for s in status] == [S.declines(c.data, r) for r in c.runs], (family, seed, window_kb)


@pytest.mark.parametrize("window_kb", WINDOWS_KB)
@pytest.mark.parametrize("family, seed", SITE_CASES)
def test_device_sites_are_the_statement_in_windows(tmp_path, family, seed, window_kb):
    c = G.case(family, seed)
    ev, _ = c.write(tmp_path)
    args = (c.kw.get("readcount_min", 1), c.kw.get("readcount_max", 1000), c.kw.get("min_segment_count", 20))
    if c.error is not None:                                   # the host's code and text, then one correct call
        with pytest.raises(_io.M6AIOError) as host:
            _io.dataprep(ev, str(tmp_path / "host"), n_threads=2, **c.kw)
        with pytest.raises(_io.M6AIOError) as e:
            _io.prep_sites(ev, *args, norm=None, n_threads=2, window_kb=window_kb)
        assert e.value.code == host.value.code == c.error[0] and message(e) == message(host) and message(e).startswith(c.error[1])
        one_correct_call(tmp_path)
        return
    for norm in (None, hct116()):
        want = c.sites if norm is None else S.sites(c.names, c.runs, norm=norm, **c.kw)
        with _io.prep_sites(ev, *args, norm=norm, n_threads=2, window_kb=window_kb) as p:
            X, km, off = p.inputs()
            tag = (family, seed, window_kb, norm is not None)
            assert p.n_sites == len(want["tx_pos"]) and p.n_reads == len(want["read_ids"]), tag
            assert_sites_are_the_statement(X, km, off, p.tx_pos, p.read_ids, [p.names[t] for t in p.site_tx],
                                           [bytes(k[1:6]).decode() for k in p.kmer7], want, tag)
            assert np.array_equal(p.off, want["off"]) and [bytes(k).decode() for k in p.kmer7] == want["kmer7"], tag
            assert (p.n_windows, p.window_bytes) == n_windows_of(c.data, window_kb), tag       # the device cuts where the rule cuts


def test_some_window_grows(tmp_path):
    """a run longer than the window: the window is taken again at twice the size, and the sizes say so"""
    c = G.case("combine", 1)
    ev, _ = c.write(tmp_path)
    with _io.prep_sites(ev, window_kb=4) as p:
        assert p.window_bytes >= 32 << 10 and (p.n_windows, p.window_bytes) == n_windows_of(c.data, 4)
    with _io.prep_sites(ev) as p:                             # the whole file: one window, of no set size
        assert (p.n_windows, p.window_bytes) == (1, 0)
    with _io.prep_sites(ev, window_kb=0) as p:
        assert (p.n_windows, p.window_bytes) == (1, 0)


# ---- every kind of line on a cut ---------------------------------------------------------------------------------------------------
def crafted_cuts(W):
    """One file for windows of W = 8 KB, readcount_max = 24:
      CUTA   140 runs of three lines, about 33 KB: they straddle at least four windows and the 25 counted runs lie in the first
      CUTB   runs of about 480 B; read 3 comes again more than W bytes behind its first run, so in a later window
      CUTC   24 runs around a site; one is declined (a signed float) and ends exactly at b + W of its window, a line without a tab
             and an empty line follow it, the runs behind them end their lines with CR LF, and the file ends without a newline
    Returns (bytes, the declined run's read index)."""
    rng = np.random.default_rng(7)
    f = G.File(rng)
    a, b, c, fill = (G.Tx(rng, n, 12, (3,)) for n in ("CUTA", "CUTB", "CUTC", "FILL"))
    G.site_reads(f, a, 3, range(140), mismatch=0, events=(1, 2))
    G.site_reads(f, b, 3, range(20), mismatch=0, events=(2, 3))
    G.site_reads(f, b, 3, [3, 20, 21], mismatch=0, events=(2, 3))
    filler = G.File(rng)
    G.site_reads(filler, fill, 3, range(60), mismatch=0)
    filler = b"".join(filler.parts[1:])
    declined = f.text(c.name, 2, c.kmer(2), 900) + f.text(c.name, 3, c.kmer(3), 900, mean="+95.31") + f.text(c.name, 4, c.kmer(4), 900)
    pad_tail = b"\t".join(G.b(x) for x in ("", 7, "CCCCC", 1, "t", 1, "80.00", "1.000", "0.00100", "NNNNN", "80.00", "1.00", "0.00", 1, 2)) + b"\n"
    n_before = 0
    while True:                                               # reads of CUTC until the window the file has reached is a settled one
        G.site_reads(f, c, 3, [n_before], mismatch=0)
        n_before += 1
        wins = WS.windows(f.bytes() + filler, W)
        settled = [k for k, w in enumerate(wins[:-1]) if w["b"] + W <= f.size]        # their cuts lie in what is written
        if n_before < 3 or not settled:
            continue
        room = wins[settled[-1] + 1]["b"] + W - f.size - len(b"PADC") - len(pad_tail) - len(declined)
        if room >= 0:
            break
        assert n_before < 20
    f.raw(b"PADC" + b"x" * room + pad_tail)
    f.raw(declined)
    f.raw(b"no tab in this line\n")
    f.raw(b"\n")
    G.site_reads(f, c, 3, range(n_before, 22), mismatch=0, eol=b"\r\n")
    f.raw(f.text(c.name, 2, c.kmer(2), 22) + f.text(c.name, 3, c.kmer(3), 22) + f.text(c.name, 4, c.kmer(4), 22, eol=b""))
    return f.bytes(), 900


def test_crafted_cuts(tmp_path, monkeypatch):
    W = 8 << 10
    data, declined_read = crafted_cuts(W)
    wins = WS.windows(data, W)
    names, runs = S.index(data)
    of = [[r for r in w["runs"] if w["names"][r["tx"]] == b"CUTA"] for w in wins]
    assert sum(bool(x) for x in of) >= 3 and len(of[0]) > 25                       # CUTA: at least 3 windows, the cut-off in the first
    first, again = [k for k, w in enumerate(wins) for r in w["runs"] if w["names"][r["tx"]] == b"CUTB" and r["read"] == 3]
    assert again > first
    (dec,) = [r for r in runs if r["read"] == declined_read]
    assert S.declines(data, dec) and any(w["e"] == w["b"] + W == dec["end"] for w in wins)
    assert data[dec["end"]:].startswith(b"no tab in this line\n\n") and b"\r\n" in data and not data.endswith(b"\n")
    ev = tmp_path / "cuts.txt"
    ev.write_bytes(data)
    kw = dict(readcount_max=24)
    monkeypatch.setenv("M6A_PREP_WINDOW_KB", "8")
    for norm in (None, hct116()):
        got = arrays_equal_the_loader(str(ev), str(tmp_path / ("cuts_%d" % (norm is not None))), kw, norm, "cuts")
        assert got is not None and {3, 20} <= got["CUTB"] and declined_read in got["CUTC"] and max(got["CUTA"]) == 24
    with _io.prep_sites(str(ev), 1, 24, 20, n_threads=2) as p:
        assert (p.n_windows, p.window_bytes) == (len(wins), W) and p.n_windows >= 6
    with _io.prep_on_device(str(ev), 1) as t:                                      # the table, too: every run, its bytes and its rows
        a = _io.table_arrays(t.contents)
    monkeypatch.delenv("M6A_PREP_WINDOW_KB")
    with _io.prep_on_device(str(ev), 1) as t:
        whole = _io.table_arrays(t.contents)
    assert a["names"] == whole["names"] and sorted(a) == sorted(whole)
    for k in a:
        if k != "names":
            assert np.array_equal(np.ascontiguousarray(a[k]).view(np.uint8), np.ascontiguousarray(whole[k]).view(np.uint8)), k


# ---- replicates ------------------------------------------------------------------------------------------------------------------
def host_arrays(p):
    X, km, off = p.inputs()
    return dict(X=X.view(np.uint32), km=km, off=off, off_host=p.off, site_tx=p.site_tx, tx_pos=p.tx_pos, kmer7=p.kmer7,
                read_ids=p.read_ids.view(np.uint64), read_rep=p.read_rep, tx_off=p.tx_off, blob=np.frombuffer(p.tx_blob, np.uint8))


@pytest.mark.parametrize("fixture", ["three", "gap", "twice"])
def test_replicates_pool_to_the_same_arrays(tmp_path, fixture):
    files = F.write(tmp_path, fixture)
    norm = hct116()
    with _io.prep_sites(files, 1, 1000, 1, norm=norm, n_threads=2) as p:
        whole, n_whole = host_arrays(p), p.n_windows
    assert n_whole == len(files)
    for window_kb in (64, 1024):
        with _io.prep_sites(files, 1, 1000, 1, norm=norm, n_threads=2, window_kb=window_kb) as p:
            cut = host_arrays(p)
            want = [n_windows_of(open(f, "rb").read(), window_kb) for f in files]
            assert p.n_windows == sum(n for n, _ in want) and p.window_bytes == max(s for _, s in want)
            assert p.n_replicates == len(files)
        for k in whole:
            assert np.array_equal(whole[k], cut[k]), (fixture, window_kb, k)


# ---- the 200 MB file ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def big(tmp_path_factory):
    """~100 copies of the bundled file, distinct transcript ids per copy (as test_gpu_eventalign_inference.test_200mb_file builds it)"""
    d = tmp_path_factory.mktemp("big")
    text = open(unpack(d, "ref_tests_data")).read()
    header, body = text.split("\n", 1)
    ev = str(d / "big.txt")
    with open(ev, "w", buffering=16 << 20) as f:
        f.write(header + "\n")
        for k in range(100):
            f.write(body.replace("ENST", "C%dENST" % k) if k else body)
    assert os.path.getsize(ev) > 200e6
    return d, ev


@pytest.mark.parametrize("csv", ["host", "device"])
def test_the_command_writes_the_same_bytes_in_windows(big, csv):
    d, ev = big
    flags = ["--eventalign", ev, "--n_processes", "8", "--num_iterations", "100", "--csv", csv]
    whole, cut = str(d / ("whole_" + csv)), str(d / ("cut_" + csv))
    run(["eventalign_inference", "--out_dir", whole] + flags)
    r = run(["eventalign_inference", "--out_dir", cut, "--window_mb", "8"] + flags, env=dict(os.environ, M6A_EVENTALIGN_TIMES="1"))
    for fn in CSVS:
        assert os.path.getsize(os.path.join(cut, fn)) > 1000 and filecmp.cmp(os.path.join(whole, fn), os.path.join(cut, fn), shallow=False), fn
    import json
    (line,) = [l for l in r.stdout.decode().splitlines() if l.startswith("M6A_TIMES ")]
    t = json.loads(line[len("M6A_TIMES "):])
    assert t["n_windows"] >= os.path.getsize(ev) // (8 << 20) and t["window_bytes"] == 8 << 20 and t["peak_bytes"] > 0


def test_a_file_over_the_whole_file_budget_goes_through_in_windows(big, monkeypatch):
    """The ceiling moves: with the budget set to the whole-file peak less half the file's size, whole-file mode is out of memory and
    8 MB windows are not, with the same arrays and a peak under that budget.  (This needs the front half, not the back half, to set
    the whole-file peak on this file; the windowed peak is asserted to lie under the budget so that the test cannot pass for nothing.)
    And the traffic: a window costs the link at most 512 B."""
    _, ev = big
    size = os.path.getsize(ev)
    norm = hct116()
    with _io.prep_sites(ev, norm=norm, n_threads=8) as p:
        whole, p0, d2h0 = host_arrays(p), p.peak_bytes, p.times()[1]
    budget_mb = (p0 - size // 2) >> 20
    print("whole file: peak %d B, d2h %d B; budget %d MB" % (p0, d2h0, budget_mb))
    monkeypatch.setenv("M6A_PREP_BUDGET_MB", str(budget_mb))
    with pytest.raises(_io.M6AIOError) as e:
        _io.prep_sites(ev, norm=norm, n_threads=8)
    assert e.value.code == -2 and "two-step path" in str(e.value)
    with _io.prep_sites(ev, norm=norm, n_threads=8, window_kb=8192) as p:
        cut, p1, d2h1, n = host_arrays(p), p.peak_bytes, p.times()[1], p.n_windows
    print("8 MB windows: %d windows, peak %d B, d2h %d B" % (n, p1, d2h1))
    assert p1 < budget_mb << 20 and p1 < p0 - size // 2
    for k in whole:
        assert np.array_equal(whole[k], cut[k]), k
    assert n >= size // (8 << 20) and d2h1 <= d2h0 + 512 * n
