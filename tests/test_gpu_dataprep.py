"""`dataprep --device gpu` (m6a_prep_eventalign, include/m6a.h): the device's table equals m6a_io_dataprep_rows's -- integers,
k-mers and byte ranges equal, features bit-equal -- and the four files it leads to are byte-identical to `--device cpu`'s, on
every fixture of tests/test_dataprep_rows.py, at the default upload chunk and at 4 KB chunks (lines, runs and positions cross
chunk boundaries), on a crafted file whose runs the device hands to the host, and on a ~200 MB file."""
import os
import subprocess
import sys

import numpy as np
import pytest

from m6anet_amd import _io
from test_dataprep_rows import FILES, GOLD, cases, crafted, ref_lines, same_files, unpack

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def device_table(ev, nn=1, index_path=None):
    with _io.prep_on_device(ev, nn, index_path) as t:
        return _io.table_arrays(t.contents)


def host_table(ev, nn=1, index_path=None):
    with _io.host_rows(ev, nn, index_path) as t:
        return _io.table_arrays(t.contents)


def assert_tables_equal(d, h):
    """Every run the device did not hand to the host has the host's npos and rows, features bit for bit."""
    assert d["names"] == h["names"]
    for k in ("run_tx", "run_read", "run_start", "run_end"):
        assert np.array_equal(d[k], h[k]), k
    ok = d["run_status"] == 0
    assert np.array_equal(d["run_npos"][ok], h["run_npos"][ok])
    for r in np.flatnonzero(ok):
        a0, a1, b0, b1 = d["row_off"][r], d["row_off"][r + 1], h["row_off"][r], h["row_off"][r + 1]
        assert a1 - a0 == b1 - b0, r
        assert np.array_equal(d["row_pos"][a0:a1], h["row_pos"][b0:b1])
        assert np.array_equal(d["row_kmer"][a0:a1], h["row_kmer"][b0:b1])
        assert np.array_equal(d["row_feat"][a0:a1].view(np.uint64), h["row_feat"][b0:b1].view(np.uint64))
    return int((~ok).sum())


@pytest.mark.parametrize("chunk_kb", [None, 4])
def test_device_table_and_files_equal_the_host(tmp_path, monkeypatch, chunk_kb):
    if chunk_kb:
        monkeypatch.setenv("M6A_PREP_CHUNK_KB", str(chunk_kb))
    for name, ev, kw in cases(tmp_path):
        nn = kw.get("n_neighbors", 1)
        declined = assert_tables_equal(device_table(ev, nn), host_table(ev, nn))
        if not name.startswith("crafted"):
            assert declined == 0, name
        cpu, gpu = str(tmp_path / (name + "_cpu")), str(tmp_path / (name + "_gpu"))
        _io.dataprep(ev, cpu, n_threads=4, device="cpu", **kw)
        _io.dataprep(ev, gpu, n_threads=4, device="gpu", **kw)
        same_files(cpu, gpu)


def test_crafted_runs_go_to_the_host(tmp_path):
    ev = crafted(tmp_path)
    d = device_table(ev)
    declined = assert_tables_equal(d, host_table(ev))
    assert declined >= 4                  # exponent, sign, 16 digits, 12.0, out of key order (each on a matching line)
    for kw in (dict(min_segment_count=1), dict(min_segment_count=1, readcount_max=3), dict(min_segment_count=2, compress=True)):
        cpu, gpu = str(tmp_path / "cpu"), str(tmp_path / "gpu")
        _io.dataprep(ev, cpu, device="cpu", **kw)
        _io.dataprep(ev, gpu, device="gpu", **kw)
        same_files(cpu, gpu)


def test_skip_index_and_errors(tmp_path):
    ev = unpack(tmp_path, "ref_tests_data")
    cpu, gpu = str(tmp_path / "cpu"), str(tmp_path / "gpu")
    _io.dataprep(ev, cpu, min_segment_count=1)
    os.makedirs(gpu)
    open(os.path.join(gpu, "eventalign.index"), "wb").write(open(os.path.join(cpu, "eventalign.index"), "rb").read())
    idx = os.path.join(gpu, "eventalign.index")
    assert assert_tables_equal(device_table(ev, 1, idx), host_table(ev, 1, idx)) == 0
    _io.dataprep(ev, cpu, min_segment_count=1, skip_index=True)
    _io.dataprep(ev, gpu, min_segment_count=1, skip_index=True, device="gpu")
    same_files(cpu, gpu)
    with pytest.raises(_io.M6AIOError) as e:
        _io.dataprep(ev, str(tmp_path / "fresh"), skip_index=True, device="gpu")
    assert e.value.code == -3
    header, lines = ref_lines()
    p = tmp_path / "short.txt"
    p.write_text(header + "\n" + "\n".join(lines[:50]) + "\nctg\t1\n")
    with pytest.raises(_io.M6AIOError) as e1:
        _io.dataprep(str(p), str(tmp_path / "a"))
    with pytest.raises(_io.M6AIOError) as e2:
        _io.dataprep(str(p), str(tmp_path / "b"), device="gpu")
    assert e1.value.code == e2.value.code == -4
    assert str(e1.value).split(": ", 1)[1] == str(e2.value).split(": ", 1)[1]


def test_over_the_budget_is_an_error_not_a_partial_output(tmp_path, monkeypatch):
    ev = unpack(tmp_path, "ref_tests_data")
    monkeypatch.setenv("M6A_PREP_BUDGET_MB", "1")
    out = str(tmp_path / "o")
    with pytest.raises(_io.M6AIOError) as e:
        _io.dataprep(ev, out, device="gpu")
    assert "--device cpu" in str(e.value) and e.value.code == -2
    assert not any(os.path.exists(os.path.join(out, f)) for f in FILES)


def test_cli_device_gpu(tmp_path):
    ev = unpack(tmp_path, "dataprep_synthetic")
    outs = {}
    for dev in ("cpu", "gpu"):
        outs[dev] = str(tmp_path / dev)
        subprocess.check_call([sys.executable, "-m", "m6anet_amd", "dataprep", "--eventalign", ev, "--out_dir", outs[dev],
                               "--min_segment_count", "5", "--n_neighbors", "2", "--device", dev], cwd=REPO, timeout=300)
    same_files(outs["cpu"], outs["gpu"])


def test_200mb_file(tmp_path):
    """~100 copies of the bundled file, distinct transcript ids per copy (as tools/measure_dataprep.py builds its large file)."""
    text = open(unpack(tmp_path, "ref_tests_data")).read()
    header, body = text.split("\n", 1)
    ev = str(tmp_path / "big.txt")
    with open(ev, "w", buffering=16 << 20) as f:
        f.write(header + "\n")
        for k in range(100):
            f.write(body.replace("ENST", "C%dENST" % k) if k else body)
    assert os.path.getsize(ev) > 200e6
    cpu, gpu = str(tmp_path / "cpu"), str(tmp_path / "gpu")
    _io.dataprep(ev, cpu, min_segment_count=20, device="cpu")
    _io.dataprep(ev, gpu, min_segment_count=20, device="gpu")
    same_files(cpu, gpu)
    a, b = _io.NativeSites([cpu], min_reads=20), _io.NativeSites([gpu], min_reads=20)
    assert a.X.shape[0] > 0 and np.array_equal(a.X, b.X) and np.array_equal(a.off, b.off) and np.array_equal(a.tx_pos, b.tx_pos)
    assert np.array_equal(a.site_kmers, b.site_kmers) and np.array_equal(a.read_id_values, b.read_id_values)
    assert [a.tx_id(i) for i in range(0, len(a.tx_pos), 97)] == [b.tx_id(i) for i in range(0, len(b.tx_pos), 97)]
    a.close()
    b.close()
