"""The window cut (tests/window_statement.py) against the index of the whole file: on every generated family that indexes, three
seeds and windows of 4, 8, 12 and 64 KB, the runs found window by window are the file's runs -- byte range, read and name -- and
the windows tile the file; the file that does not index is refused with the same text at the same offset.  And the parser of
`eventalign_inference` takes --window_mb.  tests/test_gpu_prep_windows.py holds the device to these cuts."""
import pytest

import eventalign_gen as G
import eventalign_statement as S
import window_statement as WS
from m6anet_amd.scripts import eventalign_inference

WINDOWS_KB = [4, 8, 12, 64]
INDEXED = [f for f in G.FAMILIES if "error" not in G.FAMILIES[f]]


def longest_run(data):
    return max(r["end"] - r["start"] for r in S.index(data)[1])


def test_the_generated_files_are_cut_where_the_sweep_needs_it():
    """What the sweep below relies on, so that a change to the generators cannot quietly turn it into one-window cases: the sizes
    of seed 1, the long runs that make a 4 KB window grow, and at least two windows at 8 KB."""
    sizes = {f: len(G.case(f, 1).data) for f in G.FAMILIES}
    assert min(sizes.values()) >= 1700 and max(sizes.values()) <= 2 << 20 and sizes["short_in_run"] < 2048
    long_runs = {f: longest_run(G.case(f, 1).data) for f in INDEXED}
    assert long_runs["combine"] > 28 << 10
    for f in ("plain", "newlines_0", "newlines_1", "newlines_2"):
        assert 4096 < long_runs[f] < 8192, f
    for f in INDEXED:
        if f not in ("combine", "plain", "newlines_0", "newlines_1", "newlines_2"):
            assert 250 <= long_runs[f] <= 2500, f
    for f in INDEXED:
        n = len(WS.windows(G.case(f, 1).data, 8 << 10))
        assert (n >= 2) == (f != "short_in_run"), (f, n)
    grown = [f for f in INDEXED if any(w["size"] > 4096 for w in WS.windows(G.case(f, 1).data, 4096))]
    assert {"combine", "plain", "newlines_0", "newlines_1", "newlines_2"} <= set(grown)


@pytest.mark.parametrize("window_kb", WINDOWS_KB)
@pytest.mark.parametrize("family, seed", [(f, s) for f in INDEXED for s in G.SEEDS])
def test_windows_find_the_runs_of_the_file(family, seed, window_kb):
    data = G.generate(family, seed)
    W = window_kb << 10
    wins = WS.windows(data, W)
    names, runs = S.index(data)
    got_names, got = WS.runs_of_windows(wins)
    assert got_names == names
    assert got == [dict(tx=r["tx"], read=r["read"], start=r["start"], end=r["end"]) for r in runs]
    # the windows tile the file: each starts inside or at the end of the one before, at a line's first byte, and no run is lost
    # or comes twice (the list above is the file's, in order)
    assert wins[0]["b"] == 0 and wins[-1]["e"] == len(data)
    for a, z in zip(wins, wins[1:]):
        assert a["b"] < z["b"] <= a["e"] and data[z["b"] - 1:z["b"]] == b"\n"
        assert a["e"] - a["b"] <= a["size"] and a["size"] % W == 0
        assert not a["runs"] or a["runs"][-1]["end"] <= z["b"]
    for w in wins:
        assert all(w["b"] <= r["start"] and r["end"] <= w["e"] for r in w["runs"])


@pytest.mark.parametrize("window_kb", WINDOWS_KB)
@pytest.mark.parametrize("seed", G.SEEDS)
def test_a_short_line_is_reported_at_the_offset_in_the_file(seed, window_kb):
    data = G.generate("short_line", seed)
    with pytest.raises(S.StatementError) as whole:
        S.index(data)
    with pytest.raises(S.StatementError) as cut:
        WS.windows(data, window_kb << 10)
    assert (cut.value.code, cut.value.text) == (whole.value.code, whole.value.text)


def test_no_header_line_is_the_first_windows():
    for data in (b"", b"no newline at all"):
        with pytest.raises(S.StatementError, match="no header line"):
            WS.windows(data, 4096)
    body = b"c\t1\tAAAAA\t5\tt\n" * 3
    wins = WS.windows(b"x" * 10000 + b"\n" + body, 4096)           # a header longer than the window: the window grows
    assert wins[0]["size"] == 16384 and WS.runs_of_windows(wins)[1] == S.index(b"x" * 10000 + b"\n" + body)[1]


def test_parser_takes_window_mb():
    args = ["--eventalign", "e.txt", "--out_dir", "o"]
    p = eventalign_inference.cli_parser()
    assert p.parse_args(args).window_mb == 0 and p.parse_args(args).csv == "host"
    assert p.parse_args(args + ["--window_mb", "256"]).window_mb == 256
    with pytest.raises(SystemExit):
        p.parse_args(args + ["--window_mb", "half"])
    plain = eventalign_inference.argparser().parse_args(args)        # the shared flags alone still build, without either flag
    assert not hasattr(plain, "window_mb") and not hasattr(plain, "csv")
