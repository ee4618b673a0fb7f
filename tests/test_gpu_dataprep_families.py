"""`dataprep --device gpu --writer device` and `--writer host` (m6a_prep_dataprep_write, m6a_prep_eventalign; include/m6a.h) held to the
plain statement, not to each other or to the host: on every generated family of tests/eventalign_gen.py and tests/dataprep_gen.py with
n_neighbors = 1 (but `midline`: --skip_index conflicts with --device gpu --writer device), every seed, --compress off and on, either
route writes the four files the statements give from the bytes of eventalign.txt (tests/dataprep_gen.py: expected), the device
writer declines exactly the statement's count of values and then leaves the files to the host writer, and it takes exactly the cases of
TAKES below -- so a device writer that declined everything cannot pass.  At seed 1 the same at 4 KB upload chunks and in 8 KB windows
(either route), and in 4 KB rounds of text (the device writer's).  The error families keep the statement's code and words, leave no
file, and one correct call follows.
(What bytes cannot show: a row that exactly fills csv_emit's tile is written the same through the tile or straight to global memory, so
`<` for `<=` in that comparison changes no file; an advance, a sign or a length that is off by one does.)"""
import pytest

import dataprep_gen as DG
import eventalign_gen as G
from m6anet_amd import _io
from test_dataprep_files_statement import assert_files, message, no_files

pytestmark = pytest.mark.gpu

FAMILIES = [f for f in DG.ALL if DG.ALL[f].get("nn", 1) == 1 and f != "midline"]
ERRORS = [f for f in FAMILIES if any(k in DG.ALL[f] for k in ("error", "rows_error", "site_error"))]
GOOD = [f for f in FAMILIES if f not in ERRORS]
# what the device writer takes, decided on the CPU from the statement alone (test_the_device_writer_takes_what_the_statement_says
# checks the table against the statement; every case below checks stats["writer"] against the table)
TAKES_BOTH = ["plain", "radix_4095", "radix_4096", "radix_4097", "radix_8192", "newlines_0", "newlines_1", "newlines_2", "filters_20",
              "filters_25", "long_names", "big_site", "index_wide", "big_positions", "values_taken"]
TAKES_NONE = ["split_runs", "split_rows", "radix_ties", "numbers_ok", "atoll", "combine", "declined"]
TAKES_PLAIN = ["values_rounding"]
LINE = "dataprep: --writer device declined %d values; writing on the host\n"


def takes(family, compress):
    return family in TAKES_BOTH or (family in TAKES_PLAIN and not compress)


def test_the_device_writer_takes_what_the_statement_says():
    assert sorted(TAKES_BOTH + TAKES_NONE + TAKES_PLAIN) == sorted(GOOD) and sorted(ERRORS) == ["disagree", "short_in_run", "short_line"]
    for family in GOOD:
        for seed in DG.SEEDS:
            for compress in (False, True):
                assert (DG.expected(family, seed, compress)[1] == 0) == takes(family, compress), (family, seed, compress)
    old = [f for f in TAKES_BOTH if f in G.FAMILIES]
    assert len(old) * len(DG.SEEDS) == 30 and len([f for f in GOOD if f in G.FAMILIES]) * len(DG.SEEDS) == 51


def device_writer(c, tmp_path, capfd, want, nd, compress, tag):
    """--writer device into <tmp>/dev: the statement's files, and the statement's account of who wrote them.  Returns the statistics."""
    ev, _ = c.write(tmp_path)
    dev, st = str(tmp_path / "dev"), {}
    capfd.readouterr()
    _io.dataprep(ev, dev, n_threads=2, compress=compress, device="gpu", writer="device", stats=st, **c.kw)
    err = capfd.readouterr().err
    print(tag, "statement declines", nd, "device", st["n_declined"], st["writer"], "rounds", st["n_rounds"])
    assert_files(dev, want, tag + ("device",))
    assert st["n_declined"] == nd and st["writer"] == ("device" if nd == 0 else "host") == ("device" if takes(c.family, compress) else "host"), (tag, st)
    assert err.count("declined") == (nd > 0) and err.count(LINE % nd) == (nd > 0), (tag, err)
    assert st["index_bytes"] == len(want["eventalign.index"]) and st["n_runs"] == len(c.runs), (tag, st)
    if nd == 0:
        assert st["json_bytes"] == len(want["data.json"]) and st["n_sites"] == want["data.info"].count(b"\n") - 1, (tag, st)
    return st


@pytest.mark.parametrize("compress", [False, True])
@pytest.mark.parametrize("family, seed", [(f, s) for f in GOOD for s in DG.SEEDS])
def test_both_routes_write_the_statements_files(tmp_path, capfd, family, seed, compress):
    c = DG.case(family, seed)
    want, nd = DG.expected(family, seed, compress)
    tag = (family, seed, compress)
    device_writer(c, tmp_path, capfd, want, nd, compress, tag)
    ev, _ = c.write(tmp_path)
    host = str(tmp_path / "host")
    _io.dataprep(ev, host, n_threads=2, compress=compress, device="gpu", writer="host", **c.kw)
    assert_files(host, want, tag + ("host",))


# M6A_PREP_WINDOW_KB: a window that holds no whole run is taken again at twice the size (include/m6a.h), so there is no smallest window
# relative to the longest line; 8 KB is below long_names' lines of 12 KB
UNITS = [("M6A_PREP_CHUNK_KB", "4"), ("M6A_PREP_WINDOW_KB", "8"), ("M6A_JSON_ROUND_KB", "4")]


@pytest.mark.parametrize("compress", [False, True])
@pytest.mark.parametrize("variable, value", UNITS)
@pytest.mark.parametrize("family", GOOD)
def test_small_units(tmp_path, capfd, monkeypatch, family, variable, value, compress):
    c = DG.case(family, 1)
    want, nd = DG.expected(family, 1, compress)
    whole = None
    if variable == "M6A_JSON_ROUND_KB" and family in ("big_site", "long_names"):
        (tmp_path / "whole").mkdir()
        whole = device_writer(c, tmp_path / "whole", capfd, want, nd, compress, (family, 1, compress, "default"))
    monkeypatch.setenv(variable, value)
    st = device_writer(c, tmp_path, capfd, want, nd, compress, (family, 1, compress, variable))
    if variable != "M6A_JSON_ROUND_KB":                 # the front half reads chunks and windows for either writer; rounds are the device writer's
        ev, _ = c.write(tmp_path)
        host = str(tmp_path / "host")
        _io.dataprep(ev, host, n_threads=2, compress=compress, device="gpu", writer="host", **c.kw)
        assert_files(host, want, (family, 1, compress, variable, "host"))
    if whole is not None:
        # at 32 MB either file is one round.  At 4 KB each of long_names' 14 records of over 8 KB is a round of its own, and big_site's
        # 3 000 index rows of about 28 bytes leave in blocks of 64 rows, two blocks to a round: over 20 rounds
        assert whole["n_rounds"] == 2 and st["n_rounds"] > whole["n_rounds"] and st["n_rounds"] >= 14, (whole, st)


@pytest.mark.parametrize("family, seed", [(f, s) for f in ERRORS for s in DG.SEEDS])
def test_errors_are_the_statements(tmp_path, family, seed):
    c = DG.case(family, seed)
    ev, _ = c.write(tmp_path)
    dev = str(tmp_path / "dev")
    with pytest.raises(_io.M6AIOError) as e:
        _io.dataprep(ev, dev, n_threads=2, device="gpu", writer="device", **c.kw)
    assert e.value.code == c.error[0] and message(e).startswith(c.error[1]), (family, seed, str(e.value))
    assert no_files(dev)
    good = DG.case("plain", 1)
    ev, _ = good.write(tmp_path)
    after, st = str(tmp_path / "after"), {}
    _io.dataprep(ev, after, n_threads=2, device="gpu", writer="device", stats=st)
    assert_files(after, DG.expected("plain", 1, False)[0], (family, seed, "after"))
    assert st["writer"] == "device"
