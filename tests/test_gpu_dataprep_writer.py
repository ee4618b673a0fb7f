"""`dataprep --device gpu --writer device` (m6a_prep_dataprep_write, m6a_repr_format; include/m6a.h): the number printer on the
device gives the host core's bytes on the shared generator (tests/repr_inputs.py), and the four files are byte-identical to
`--device cpu`'s on every fixture of tests/test_dataprep_rows.py with n_neighbors = 1 -- at the default upload chunk and at 4 KB
chunks, in many small rounds, in windows, on the crafted file whose runs go through the host half, where the printer declines a
value, on files with no site, and after every error."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import dataprep_json_statement as S
import repr_inputs
from m6anet_amd import _io
from test_dataprep_json_statement import parse_json
from test_dataprep_rows import FILES, cases, crafted, edge_files, ref_lines, same_files, unpack

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. the number printer -----------------------------------------------------------------------------------------------------------
def host_core(v, round3):
    L, buf, out, off = _io.load(), C.create_string_buffer(40), [], [0]
    n_declined = 0
    for x in v.tolist():
        n = L.m6a_io_repr_core(x, 1 if round3 else 0, buf)
        n_declined += n < 0
        out.append(buf.value)
        off.append(off[-1] + len(buf.value))
    return b"".join(out), np.array(off, np.int64), n_declined


@pytest.fixture(scope="module")
def generator_and_host_text():
    v, ok = repr_inputs.all_values()
    return v, ok, {r: host_core(v, r) for r in (False, True)}


@pytest.mark.parametrize("round3", [False, True])
def test_repr_format_is_the_host_core(generator_and_host_text, round3):
    v, ok, host = generator_and_host_text
    text, off, nd = host[round3]
    want = repr_inputs.expected(v, round3)
    assert nd == sum(w is None for w in want) and (round3 or nd == int((~ok).sum()))      # the statement's count
    got_text, got_off, got_nd = _io.repr_format(v, round3)
    assert got_nd == nd and np.array_equal(got_off, off) and got_text == text
    first_declined = int(np.flatnonzero(~ok)[0])
    for a, n in ((0, 0), (0, 1), (0, 63), (0, 64), (0, 65), (first_declined - 30, 63), (first_declined - 40, 65), (first_declined, 1)):
        t, o, d = _io.repr_format(v[a:a + n], round3)               # the wave edges, with and without a declined value inside
        assert t == text[off[a]:off[a + n]] and np.array_equal(o, off[a:a + n + 1] - off[a]), (a, n)
        assert d == sum(w is None for w in want[a:a + n]), (a, n)


# ---- 2. the files, on every fixture ------------------------------------------------------------------------------------------------------
def both(ev, tmp_path, name, **kw):
    """--device cpu into <name>_cpu, --device gpu --writer device into <name>_dev; the directories and the statistics."""
    cpu, dev, st = str(tmp_path / (name + "_cpu")), str(tmp_path / (name + "_dev")), {}
    _io.dataprep(ev, cpu, n_threads=4, device="cpu", **kw)
    _io.dataprep(ev, dev, n_threads=4, device="gpu", writer="device", stats=st, **kw)
    same_files(cpu, dev)
    return cpu, dev, st


@pytest.mark.parametrize("chunk_kb", [None, 4])
def test_files_equal_the_cpu_path(tmp_path, monkeypatch, chunk_kb):
    if chunk_kb:
        monkeypatch.setenv("M6A_PREP_CHUNK_KB", str(chunk_kb))
    seen = 0
    for name, ev, kw in cases(tmp_path):
        if kw.get("n_neighbors", 1) != 1:
            continue
        cpu, dev, st = both(ev, tmp_path, name, **kw)
        seen += 1
        if not name.startswith("crafted"):
            assert st["writer"] == "device" and st["n_declined"] == 0, (name, st)
            assert st["json_bytes"] == os.path.getsize(os.path.join(dev, "data.json")), name
            assert st["index_bytes"] == os.path.getsize(os.path.join(dev, "eventalign.index")), name
            assert st["n_sites"] == len(open(os.path.join(dev, "data.info")).readlines()) - 1, name
    assert seen == 9


# ---- 3. rounds and windows -----------------------------------------------------------------------------------------------------------------
def test_many_rounds(tmp_path, monkeypatch):
    ev = unpack(tmp_path, "ref_tests_data")
    _, dev, one = both(ev, tmp_path, "one", min_segment_count=1)
    monkeypatch.setenv("M6A_JSON_ROUND_KB", "4")
    _, dev, st = both(ev, tmp_path, "many", min_segment_count=1)
    sizes = [len(l) for l in open(os.path.join(dev, "data.json"), "rb")]
    index_kb = os.path.getsize(os.path.join(dev, "eventalign.index")) >> 10
    assert max(sizes) > 4096 and min(sizes) < 2048                  # sites larger than a round, and rounds of several sites
    assert one["n_rounds"] == 2 and st["n_rounds"] > sum(s > 4096 for s in sizes) + index_kb / 4 > 20
    assert st["json_bytes"] == sum(sizes) and st["n_declined"] == 0


def test_windows(tmp_path, monkeypatch):
    ev = unpack(tmp_path, "ref_tests_data")
    monkeypatch.setenv("M6A_PREP_WINDOW_KB", "8")
    _, _, st = both(ev, tmp_path, "win", min_segment_count=1)
    assert st["writer"] == "device"


# ---- 4. the crafted file ---------------------------------------------------------------------------------------------------------------------
def statement_declined(ev, tmp_path, compress, **kw):
    d = str(tmp_path / "plain_for_statement")
    _io.dataprep(ev, d, device="cpu", **kw)
    return S.n_declined(parse_json(os.path.join(d, "data.json")), compress)


def test_crafted_runs_go_through_the_host_half(tmp_path, capfd):
    ev = crafted(tmp_path)
    kw = dict(min_segment_count=1, readcount_max=3)
    assert statement_declined(ev, tmp_path, True, **kw) == 0
    with _io.prep_on_device(ev, 1) as t:
        assert (_io.table_arrays(t.contents)["run_status"] != 0).sum() >= 4       # runs the front half declines
    _, _, st = both(ev, tmp_path, "rc3", compress=True, **kw)
    assert st["writer"] == "device" and st["n_declined"] == 0 and "declined" not in capfd.readouterr().err


def test_a_declined_value_goes_to_the_host_writer(tmp_path, capfd):
    ev = crafted(tmp_path)                                           # its signed mean reaches a site: repr would write a minus sign
    for compress in (False, True):
        want = statement_declined(ev, tmp_path, compress, min_segment_count=1)
        assert want > 0
        capfd.readouterr()
        _, dev, st = both(ev, tmp_path, "declined_%d" % compress, min_segment_count=1, compress=compress)
        err = capfd.readouterr().err
        assert err.count("dataprep: --writer device declined %d values; writing on the host\n" % want) == 1 and err.count("declined") == 1
        assert st["writer"] == "host" and st["n_declined"] == want
        assert "-" in open(os.path.join(dev, "data.json")).read()


# ---- 5. errors, each followed by one correct call in the same process --------------------------------------------------------------------------
def runs_of(rows):
    out = []
    for i, r in enumerate(rows):
        if not out or out[-1][0] != r[0] or out[-1][1] != r[3]:
            out.append([r[0], r[3], i, i])
        out[-1][3] = i + 1
    return out


def disagreeing(tmp_path):
    """ref_tests_data with the first 5-mer of one read's DRACH window replaced, where another read covers the same window."""
    header, lines = ref_lines()
    rows = [l.split("\t") for l in lines]
    drach = re.compile("[AGT][GA]AC[ACT]")
    covered = {}
    runs = runs_of(rows)
    for tx, read, a, b in runs:
        pos = {int(rows[i][1]): rows[i][2] for i in range(a, b)}
        for p in pos:
            if p + 1 in pos and p + 2 in pos and drach.fullmatch(pos[p + 1]):
                if (tx, p) in covered and covered[(tx, p)] != read:
                    for i in range(a, b):
                        if int(rows[i][1]) == p:
                            rows[i][2] = rows[i][9] = "TTTTT"
                    path = tmp_path / "disagree.txt"
                    path.write_text(header + "\n" + "\n".join("\t".join(r) for r in rows) + "\n")
                    return str(path), tx, p + 3
                covered.setdefault((tx, p), read)
    raise AssertionError("no window shared by two reads")


def no_files(d):
    return not any(os.path.exists(os.path.join(d, f)) for f in FILES)


def test_errors_are_the_cpu_paths(tmp_path, monkeypatch):
    good = unpack(tmp_path, "ref_tests_data")
    ev, tx, pos = disagreeing(tmp_path)
    with pytest.raises(_io.M6AIOError) as host:
        _io.dataprep(ev, str(tmp_path / "dis_cpu"), min_segment_count=1, device="cpu")
    with pytest.raises(_io.M6AIOError) as dev:
        _io.dataprep(ev, str(tmp_path / "dis_dev"), min_segment_count=1, device="gpu", writer="device")
    h, g = str(host.value).split(": ", 1)[1], str(dev.value).split(": ", 1)[1]
    assert h == "reads disagree on the sequence at %s:%d" % (tx, pos) and g == h and dev.value.code == host.value.code == -4
    assert no_files(str(tmp_path / "dis_dev"))
    both(good, tmp_path, "after_disagree", min_segment_count=20)

    monkeypatch.setenv("M6A_PREP_BUDGET_MB", "1")
    with pytest.raises(_io.M6AIOError) as e:
        _io.dataprep(good, str(tmp_path / "budget"), device="gpu", writer="device")
    assert "--device cpu" in str(e.value) and e.value.code == -2 and no_files(str(tmp_path / "budget"))
    monkeypatch.delenv("M6A_PREP_BUDGET_MB")
    both(good, tmp_path, "after_budget", min_segment_count=20)

    header, lines = ref_lines()
    p = tmp_path / "short.txt"
    p.write_text(header + "\n" + "\n".join(lines[:50]) + "\nctg\t1\n")
    with pytest.raises(_io.M6AIOError) as e1:
        _io.dataprep(str(p), str(tmp_path / "short_cpu"))
    with pytest.raises(_io.M6AIOError) as e2:
        _io.dataprep(str(p), str(tmp_path / "short_dev"), device="gpu", writer="device")
    assert e1.value.code == e2.value.code == -4 and str(e1.value).split(": ", 1)[1] == str(e2.value).split(": ", 1)[1]
    assert no_files(str(tmp_path / "short_dev"))
    with pytest.raises(_io.M6AIOError) as e3:
        _io.dataprep(str(tmp_path / "missing.txt"), str(tmp_path / "missing_dev"), device="gpu", writer="device")
    assert e3.value.code == -3 and no_files(str(tmp_path / "missing_dev"))
    both(good, tmp_path, "after_short", min_segment_count=20)


# ---- 6. no site at all -----------------------------------------------------------------------------------------------------------------------
def test_no_site_and_header_only(tmp_path):
    ev = unpack(tmp_path, "ref_tests_data")
    cpu, dev, st = both(ev, tmp_path, "nosite", min_segment_count=100000)
    assert os.path.getsize(os.path.join(dev, "data.json")) == 0 and st["n_sites"] == 0 and st["json_bytes"] == 0
    assert open(os.path.join(dev, "data.info")).read() == S.INFO_HEADER and os.path.getsize(os.path.join(dev, "data.log")) > 0
    cpu, dev, st = both(ev, tmp_path, "nowanted", readcount_min=100000)
    assert os.path.getsize(os.path.join(dev, "data.log")) == 0 and st["n_runs"] > 0
    cpu, dev, st = both(edge_files(tmp_path)["header_only"], tmp_path, "header_only")
    assert open(os.path.join(dev, "eventalign.index")).read() == S.INDEX_HEADER and st["n_runs"] == 0
    assert open(os.path.join(dev, "data.info")).read() == S.INFO_HEADER


# ---- 7. the command --------------------------------------------------------------------------------------------------------------------------
def test_command(tmp_path):
    ev = unpack(tmp_path, "ref_tests_data")
    cpu, dev = str(tmp_path / "cpu"), str(tmp_path / "dev")
    _io.dataprep(ev, cpu, min_segment_count=20, compress=True)
    r = subprocess.run([sys.executable, "-m", "m6anet_amd", "dataprep", "--eventalign", ev, "--out_dir", dev, "--device", "gpu", "--writer", "device",
                        "--compress", "--n_processes", "4"], cwd=REPO, timeout=600, env=dict(os.environ, M6A_DATAPREP_TIMES="1"),
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    same_files(cpu, dev)
    lines = [l for l in r.stderr.splitlines() if l.startswith("M6A_TIMES ")]
    assert len(lines) == 1
    st = json.loads(lines[0][len("M6A_TIMES "):])
    assert st["writer"] == "device" and st["n_declined"] == 0 and st["n_rounds"] == 2
    assert st["json_bytes"] == os.path.getsize(os.path.join(dev, "data.json")) and st["n_sites"] == 101
    assert st["d2h_bytes"] < 2 * (st["json_bytes"] + st["index_bytes"]) and st["peak_bytes"] > 0
    assert all(st[k] >= 0 for k in ("ms_front", "ms_back", "ms_format", "ms_copy", "ms_write"))
