"""Read names on the host side: an m6a_sites built from host arrays plus a table of names (m6a_io_sites_set_read_names) writes the
statement's CSV text -- data.site_proba.csv untouched, the UUID in column 3 of data.indiv_proba.csv -- for one and for three
replicates, whole and cut at 7 sites, through write_csv and through the shard writers; a read id outside its table is refused;
without the call the bytes are what they are today; and `eventalign_inference` has the flag while the flags it shares have not moved."""
import os

import numpy as np
import pytest

import csv_statement as ST
import read_names_statement as RS
from m6anet_amd import _io
from m6anet_amd.scripts import dataprep, eventalign_inference, inference

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CSVS = ("data.site_proba.csv", "data.indiv_proba.csv")


@pytest.fixture(scope="module")
def golden():
    """the arrays of the bundled sites as from_arrays takes them, three outputs, and per n_rep the replicate of each read and the
    tables of names: read ids are made indices into their replicate's table, in a shuffled order"""
    nat = _io.NativeSites([os.path.join(GOLD, "ref_tests_data")], 20, None, 2)
    S, R = len(nat.tx_pos), int(nat.off[-1])
    names = sorted({nat.tx_id(i) for i in range(S)})
    a = dict(off=np.array(nat.off), tx_pos=np.array(nat.tx_pos), tx_blob="".join(names).encode(),
             tx_off=np.cumsum([0] + [len(n) for n in names]), site_tx=np.array([names.index(nat.tx_id(i)) for i in range(S)], np.uint32),
             kmer5=np.frombuffer("".join(nat.kmer5(i) for i in range(S)).encode(), np.uint8).reshape(S, 5))
    nat.close()
    rng = np.random.default_rng(11)
    a.update(read_prob=rng.random(R, np.float32), site_prob=rng.random(S, np.float32), mod_ratio=rng.random(S))
    by_rep = {}
    for n_rep in (1, 3):
        rep = rng.integers(0, n_rep, R).astype(np.int32)
        sizes = [int((rep == k).sum()) // 2 + 3 for k in range(n_rep)]              # reads share names, as the reads of one molecule do
        ids = np.array([rng.integers(0, sizes[k]) for k in rep], np.float64)
        tables = [[int.from_bytes(rng.bytes(16), "big") for _ in range(n)] for n in sizes]
        by_rep[n_rep] = dict(read_ids=ids, read_rep=rep if n_rep > 1 else None, n_rep=n_rep, tables=tables,
                             names16=np.concatenate([RS.table(t) for t in tables]), name_off=np.cumsum([0] + sizes))
    return a, by_rep


def build(a, r, named=True):
    s = _io.NativeSites.from_arrays(a["off"], a["tx_pos"], a["tx_blob"], a["tx_off"], a["site_tx"], a["kmer5"], r["read_ids"], r["read_rep"], r["n_rep"])
    if named:
        s.set_read_names(r["names16"], r["name_off"])
    return s


def statement(a, r, limit):
    site, indiv = ST.texts(a["off"], a["tx_pos"], a["tx_blob"], a["tx_off"], a["site_tx"], a["kmer5"], r["read_ids"], a["read_prob"], a["site_prob"],
                           a["mod_ratio"], r["read_rep"], r["n_rep"], site_end=limit)
    return ST.SITE_HEADER + site, ST.INDIV_HEADER + indiv


def written(d):
    return tuple(open(os.path.join(str(d), f), "rb").read() for f in CSVS)


@pytest.mark.parametrize("limit", [None, 7])
@pytest.mark.parametrize("n_rep", [1, 3])
def test_writers_print_the_names(tmp_path, golden, n_rep, limit):
    a, r = golden[0], golden[1][n_rep]
    site, indiv = statement(a, r, limit)
    want = (site, RS.indiv(indiv, r["tables"]))
    assert want[1] != indiv and want[1].count(b"-") >= 4 * (len(indiv.splitlines()) - 1)
    s = build(a, r)
    s.write_csv(str(tmp_path), a["read_prob"], a["site_prob"], a["mod_ratio"], write_header=True, n_threads=3, n_sites=limit)
    assert written(tmp_path) == want
    # the shard writers: two ranks, the first writes the headers
    S = len(a["tx_pos"]) if limit is None else limit
    mid, out = S // 2, tmp_path / "shards"
    out.mkdir()
    sizes = []
    for lo, hi in ((0, mid), (mid, S)):
        r0, r1 = int(a["off"][lo]), int(a["off"][hi])
        sizes.append(s.csv_shard_size(lo, hi, a["read_prob"][r0:r1], a["site_prob"][lo:hi], a["mod_ratio"][lo:hi]))
    hs, hi_ = s.csv_header_bytes()
    totals = (hs + sizes[0][0] + sizes[1][0], hi_ + sizes[0][1] + sizes[1][1])
    for k, (lo, hi) in enumerate(((0, mid), (mid, S))):
        r0, r1 = int(a["off"][lo]), int(a["off"][hi])
        s.csv_shard_write(str(out), lo, hi, a["read_prob"][r0:r1], a["site_prob"][lo:hi], a["mod_ratio"][lo:hi],
                          hs + (sizes[0][0] if k else 0), hi_ + (sizes[0][1] if k else 0), totals if k == 0 else None)
    assert written(out) == want
    s.close()


@pytest.mark.parametrize("n_rep", [1, 3])
def test_without_the_call_the_bytes_are_todays(tmp_path, golden, n_rep):
    a, r = golden[0], golden[1][n_rep]
    s = build(a, r, named=False)
    s.write_csv(str(tmp_path), a["read_prob"], a["site_prob"], a["mod_ratio"], write_header=True, n_threads=3)
    assert written(tmp_path) == statement(a, r, None)
    s.close()


@pytest.mark.parametrize("n_rep", [1, 3])
def test_a_read_id_outside_its_table_is_refused(tmp_path, golden, n_rep):
    a, r = golden[0], golden[1][n_rep]
    k = int(r["read_rep"][5]) if n_rep > 1 else 0
    size = int(r["name_off"][k + 1] - r["name_off"][k])
    for bad in (float(size), -1.0, 0.5, float("nan"), -0.0, 1e18):
        ids = r["read_ids"].copy()
        ids[5] = bad
        s = build(a, dict(r, read_ids=ids), named=False)
        with pytest.raises(_io.M6AIOError) as e:
            s.set_read_names(r["names16"], r["name_off"])
        assert e.value.code == -1 and "read 5" in str(e.value), bad
        s.write_csv(str(tmp_path), a["read_prob"], a["site_prob"], a["mod_ratio"], write_header=True, n_sites=0)     # nothing was set
        s.close()
    s = build(a, r, named=False)
    with pytest.raises(_io.M6AIOError) as e:                                     # one table too few
        _io._chk(s._L.m6a_io_sites_set_read_names(s._h, r["names16"].ctypes.data, r["name_off"].ctypes.data, n_rep + 1))
    assert e.value.code == -1
    ids = r["read_ids"].copy()
    ids[5] = size - 1                                                              # the last row of its table is inside
    s2 = build(a, dict(r, read_ids=ids))
    s2.close()
    s.close()
    loaded = _io.NativeSites([os.path.join(GOLD, "ref_tests_data")], 20, None, 2)   # loaded sites take no names
    with pytest.raises(_io.M6AIOError) as e:
        loaded.set_read_names(np.zeros((1, 16), np.uint8), np.array([0, 1]))
    assert e.value.code == -1
    loaded.close()


def flags(parser):
    return {a.dest: (a.default, a.required, tuple(a.option_strings)) for a in parser._actions}


def test_the_command_has_the_flag_and_the_shared_flags_have_not_moved():
    shared, cli = flags(eventalign_inference.argparser()), flags(eventalign_inference.cli_parser())
    assert set(shared) == {"eventalign", "out_dir", "readcount_min", "readcount_max", "min_segment_count", "n_processes", "pretrained_model",
                           "model_state_dict", "model_config", "norm_path", "batch_size", "save_per_batch", "num_iterations", "device", "seed",
                           "read_proba_threshold", "encoder", "drop_unflushed_tail"}
    assert set(cli) - set(shared) == {"csv", "window_mb", "compress", "compress_level", "read_names"}
    assert all(cli[k] == shared[k] for k in shared)
    assert cli["read_names"] == (False, False, ("--read_names",))
    p = eventalign_inference.cli_parser()
    assert p.parse_args(["--eventalign", "e", "--out_dir", "o"]).read_names is False
    assert p.parse_args(["--eventalign", "e", "--out_dir", "o", "--read_names"]).read_names is True
    (action,) = [a for a in p._actions if a.dest == "read_names"]
    assert "data.json" in action.help and "UUID" in action.help
    assert "read_names" not in flags(dataprep.argparser()) and "read_names" not in flags(inference.argparser())
