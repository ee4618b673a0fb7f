"""The two halves of native dataprep (include/m6a_io.h): m6a_io_dataprep_rows (the index runs and every run's candidate rows)
followed by m6a_io_dataprep_write (the readcount cut, one run per read, the sort, min_segment_count and the text) write the same
four files, byte for byte, as m6a_io_dataprep -- the path `dataprep --device gpu` takes with a device-made table."""
import gzip
import os

import numpy as np
import pytest

from m6anet_amd import _io

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FILES = ("eventalign.index", "data.json", "data.info", "data.log")


def unpack(tmp_path, sub, name="eventalign.txt"):
    p = tmp_path / (sub + "_" + name)
    p.write_bytes(gzip.open(os.path.join(GOLD, sub, "eventalign.txt.gz"), "rb").read())
    return str(p)


def ref_lines():
    text = gzip.open(os.path.join(GOLD, "ref_tests_data", "eventalign.txt.gz"), "rt").read()
    header, body = text.split("\n", 1)
    return header, body.rstrip("\n").split("\n")


def crafted(tmp_path):
    """Every case a fast path declines, on lines of the bundled file: a float in exponent form, a signed float, a 16-digit float,
    an integer field written as 12.0, a run out of key order, NNNNN model k-mers, a read of one position, a read index that comes
    back later in the same transcript."""
    header, lines = ref_lines()
    rows = [l.split("\t") for l in lines[:3000]]
    reads = []
    for i, r in enumerate(rows):
        if not reads or reads[-1][1] != r[3]:
            reads.append([i, r[3]])
    starts = [i for i, _ in reads]

    def first_line_of(k):
        return starts[k]
    rows[first_line_of(3)][6] = "%.4e" % float(rows[first_line_of(3)][6])                 # exponent form
    rows[first_line_of(5)][6] = "-" + rows[first_line_of(5)][6]                           # signed
    rows[first_line_of(7)][7] = rows[first_line_of(7)][7] + "0" * (16 - len(rows[first_line_of(7)][7].replace(".", "")))  # 16 digits
    rows[first_line_of(9)][13] = rows[first_line_of(9)][13] + ".0"                        # integer field as 12.0
    a = first_line_of(11)
    rows[a], rows[a + 1] = rows[a + 1], rows[a]                                           # out of key order
    for k in range(first_line_of(13), first_line_of(14)):
        rows[k][9] = "NNNNN"                                                              # model k-mer NNNNN
    for k in range(first_line_of(15), first_line_of(16)):
        rows[k][1] = rows[first_line_of(15)][1]                                           # one position only
        rows[k][2] = rows[k][9] = rows[first_line_of(15)][2]
    # read 17 again after read 18, same transcript: a repeated read index
    b0, b1, b2 = first_line_of(17), first_line_of(18), first_line_of(19)
    if rows[b0][0] == rows[b1][0]:
        rows[b1:b2] = rows[b1:b2] + [list(r) for r in rows[b0:b1]]
    p = tmp_path / "crafted.txt"
    p.write_text(header + "\n" + "\n".join("\t".join(r) for r in rows) + "\n")
    return str(p)


def edge_files(tmp_path):
    header, lines = ref_lines()
    base = header + "\n" + "\n".join(lines[:600])
    out = {}
    for tag, txt in (("header_only", header + "\n"), ("nonl", base), ("crlf", (base + "\n").replace("\n", "\r\n"))):
        p = tmp_path / (tag + ".txt")
        p.write_bytes(txt.encode())
        out[tag] = str(p)
    return out


def cases(tmp_path):
    """(name, eventalign, kwargs) for every fixture the two paths are compared on."""
    ref = unpack(tmp_path, "ref_tests_data")
    out = [("ref_msc1", ref, dict(min_segment_count=1)), ("ref_msc20_compress", ref, dict(min_segment_count=20, compress=True))]
    syn = unpack(tmp_path, "dataprep_synthetic")
    out += [("synthetic_nn%d" % nn, syn, dict(min_segment_count=5, n_neighbors=nn)) for nn in (1, 2, 3)]
    out.append(("noncontiguous", unpack(tmp_path, "dataprep_noncontiguous"), dict(min_segment_count=1)))
    out += [(tag, p, dict(min_segment_count=1)) for tag, p in edge_files(tmp_path).items()]
    cr = crafted(tmp_path)
    out += [("crafted", cr, dict(min_segment_count=1)), ("crafted_rc3", cr, dict(min_segment_count=1, readcount_max=3))]
    return out


def write_both(ev, tmp_path, name, threads=4, **kw):
    """m6a_io_dataprep into <name>_host, rows + write into <name>_rows; returns both directories."""
    host, rows = str(tmp_path / (name + "_host")), str(tmp_path / (name + "_rows"))
    nn = kw.pop("n_neighbors", 1)
    _io.dataprep(ev, host, n_threads=threads, n_neighbors=nn, **kw)
    with _io.host_rows(ev, nn, n_threads=threads) as t:
        _io.write_table(ev, rows, t, n_threads=threads, **kw)
    return host, rows


def same_files(a, b, names=FILES):
    for fn in names:
        assert open(os.path.join(a, fn), "rb").read() == open(os.path.join(b, fn), "rb").read(), fn


@pytest.mark.parametrize("threads", [1, 4])
def test_rows_then_write_is_dataprep(tmp_path, threads):
    for name, ev, kw in cases(tmp_path):
        host, rows = write_both(ev, tmp_path, "%s_t%d" % (name, threads), threads=threads, **kw)
        same_files(host, rows)


def test_crafted_file_exercises_what_it_says(tmp_path):
    ev = crafted(tmp_path)
    blob = open(ev).read()
    assert "e+0" in blob and "\t-" in blob and ".0\t" in blob and "NNNNN" in blob
    host, _ = write_both(ev, tmp_path, "c", min_segment_count=1)
    assert os.path.getsize(os.path.join(host, "data.json")) > 1000
    with _io.host_rows(ev, 1) as t:
        a = _io.table_arrays(t.contents)
    assert (a["run_npos"] == 1).any()                                        # a read of a single position
    keys = list(zip(a["run_tx"].tolist(), a["run_read"].tolist()))
    assert len(set(keys)) < len(keys)                                         # a read index twice in one transcript


def test_table_layout(tmp_path):
    ev = unpack(tmp_path, "dataprep_synthetic")
    with _io.host_rows(ev, 2) as t:
        a = _io.table_arrays(t.contents)
    nr = len(a["run_read"])
    assert nr > 10 and a["row_off"][0] == 0 and a["row_off"][-1] == len(a["row_pos"]) and np.all(np.diff(a["row_off"]) >= 0)
    assert a["row_kmer"].shape[1] == 9 and a["row_feat"].shape[1] == 15 and (a["run_status"] == 0).all()
    idx = open(os.path.join(GOLD, "dataprep_synthetic", "eventalign.index")).read().splitlines()[1:]
    assert [(a["names"][t], str(r), str(s), str(e)) for t, r, s, e in zip(a["run_tx"], a["run_read"], a["run_start"], a["run_end"])] \
        == [tuple(l.split(",")) for l in idx]
    for r in range(nr):                                                       # rows in position order inside a run
        assert np.all(np.diff(a["row_pos"][a["row_off"][r]:a["row_off"][r + 1]]) > 0)


def test_skip_index(tmp_path):
    ev = unpack(tmp_path, "ref_tests_data")
    host = str(tmp_path / "host")
    _io.dataprep(ev, host, min_segment_count=1)
    rows = str(tmp_path / "rows")
    os.makedirs(rows)
    idx_text = open(os.path.join(host, "eventalign.index"), "rb").read()
    open(os.path.join(rows, "eventalign.index"), "wb").write(idx_text)
    _io.dataprep(ev, host, min_segment_count=1, skip_index=True)
    with _io.host_rows(ev, 1, index_path=os.path.join(rows, "eventalign.index")) as t:
        _io.write_table(ev, rows, t, min_segment_count=1, write_index=False)
    same_files(host, rows)
    assert open(os.path.join(rows, "eventalign.index"), "rb").read() == idx_text
    with pytest.raises(_io.M6AIOError):
        _io.host_rows(ev, 1, index_path=str(tmp_path / "missing.index"))


def test_errors_are_the_host_paths(tmp_path):
    header, lines = ref_lines()
    p = tmp_path / "short.txt"
    p.write_text(header + "\n" + "\n".join(lines[:50]) + "\nctg\t1\n")
    with pytest.raises(_io.M6AIOError) as e1:
        _io.dataprep(str(p), str(tmp_path / "a"))
    with pytest.raises(_io.M6AIOError) as e2:
        _io.host_rows(str(p), 1)
    assert e1.value.code == e2.value.code == -4 and str(e1.value).split(": ", 1)[1] == str(e2.value).split(": ", 1)[1]
