"""`eventalign_inference` on the host side: its parser takes dataprep's site flags and inference's flags with their defaults and
refuses what `inference` refuses, `inference`'s own parser is untouched, and an m6a_sites built from host arrays
(m6a_io_sites_from_arrays) writes the CSVs byte for byte as the loaded sites it was built from."""
import os

import numpy as np
import pytest

from m6anet_amd import _io
from m6anet_amd.scripts import dataprep, eventalign_inference, inference

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def defaults(parser):
    return {a.dest: a.default for a in parser._actions}


def test_parser_defaults_are_dataprep_and_inference_defaults():
    p, d, i = defaults(eventalign_inference.argparser()), defaults(dataprep.argparser()), defaults(inference.argparser())
    for flag in ("readcount_min", "readcount_max", "min_segment_count", "n_processes"):
        assert p[flag] == d[flag], flag
    for flag in ("pretrained_model", "model_state_dict", "model_config", "norm_path", "batch_size", "save_per_batch", "num_iterations",
                 "device", "seed", "read_proba_threshold", "encoder", "drop_unflushed_tail"):
        assert p[flag] == i[flag], flag
    assert set(p) == {"eventalign", "out_dir", "readcount_min", "readcount_max", "min_segment_count", "n_processes", "pretrained_model",
                      "model_state_dict", "model_config", "norm_path", "batch_size", "save_per_batch", "num_iterations", "device", "seed",
                      "read_proba_threshold", "encoder", "drop_unflushed_tail"}
    a = eventalign_inference.argparser().parse_args(["--eventalign", "e.txt", "--out_dir", "o"])
    assert (a.eventalign, a.out_dir, a.n_processes, a.min_segment_count, a.device) == ("e.txt", "o", 1, 20, "cuda:0")


def test_parser_refuses_what_inference_refuses(tmp_path):
    with pytest.raises(SystemExit):
        eventalign_inference.argparser().parse_args(["--eventalign", "e", "--out_dir", "o", "--encoder", "bogus"])
    with pytest.raises(SystemExit):
        eventalign_inference.argparser().parse_args(["--out_dir", "o"])
    args = eventalign_inference.argparser().parse_args(["--eventalign", str(tmp_path / "missing.txt"), "--out_dir", str(tmp_path / "o"),
                                                        "--device", "cpu"])
    with pytest.raises(ValueError, match="--device cpu"):
        eventalign_inference.main(args)
    assert not os.path.exists(tmp_path / "o")


def test_inference_parser_is_unchanged():
    p = inference.argparser()
    req = {a.dest: a.required for a in p._actions}
    assert req["input_dir"] and req["out_dir"]
    assert sorted(defaults(p)) == sorted(["input_dir", "out_dir", "pretrained_model", "model_config", "model_state_dict", "norm_path",
                                          "batch_size", "save_per_batch", "n_processes", "num_iterations", "device", "seed",
                                          "read_proba_threshold", "gpus", "encoder", "drop_unflushed_tail"])
    assert defaults(p)["n_processes"] == 25 and defaults(p)["gpus"] == 1


@pytest.mark.parametrize("limit", [None, 7])
def test_sites_from_arrays_write_the_same_bytes(tmp_path, limit):
    nat = _io.NativeSites([os.path.join(GOLD, "ref_tests_data")], 20, None, 2)
    S, R = len(nat.tx_pos), int(nat.off[-1])
    names = sorted({nat.tx_id(i) for i in range(S)}, reverse=True)          # any name table: the sites index it
    blob = "".join(names).encode()
    tx_off = np.cumsum([0] + [len(n.encode()) for n in names])
    site_tx = np.array([names.index(nat.tx_id(i)) for i in range(S)], np.uint32)
    k5 = np.frombuffer("".join(nat.kmer5(i) for i in range(S)).encode(), np.uint8).reshape(S, 5)
    built = _io.NativeSites.from_arrays(nat.off, nat.tx_pos, blob, tx_off, site_tx, k5, nat.read_id_values)
    assert built.X is None and np.array_equal(built.off, nat.off) and [built.tx_id(i) for i in range(S)] == [nat.tx_id(i) for i in range(S)]
    rng = np.random.default_rng(3)
    rp, sp, mr = rng.random(R, np.float32), rng.random(S, np.float32), rng.random(S)
    a, b = tmp_path / "a", tmp_path / "b"
    a.mkdir()
    b.mkdir()
    nat.write_csv(str(a), rp, sp, mr, write_header=True, n_sites=limit)
    built.write_csv(str(b), rp, sp, mr, write_header=True, n_sites=limit)
    for fn in ("data.site_proba.csv", "data.indiv_proba.csv"):
        assert (a / fn).read_bytes() == (b / fn).read_bytes(), fn
    assert len((a / "data.site_proba.csv").read_bytes().splitlines()) == 1 + (S if limit is None else limit)
    built.close()
    nat.close()


def test_runs_rows_are_the_rows_of_those_runs(tmp_path):
    ev = os.path.join(tmp_path, "ev.txt")
    import gzip
    open(ev, "wb").write(gzip.open(os.path.join(GOLD, "ref_tests_data", "eventalign.txt.gz"), "rb").read())
    with _io.host_rows(ev, 1) as t:
        full = _io.table_arrays(t.contents)
    pick = np.arange(0, len(full["run_start"]), 3)
    import ctypes as C
    L = _io.load()
    h = C.c_void_p()
    st, en, rd = (np.ascontiguousarray(full[k][pick]) for k in ("run_start", "run_end", "run_read"))
    assert L.m6a_io_runs_rows(ev.encode(), len(pick), st.ctypes.data, en.ctypes.data, rd.ctypes.data, 1, 2, C.byref(h)) == 0
    part = _io.table_arrays(L.m6a_io_rows_table(h).contents)
    L.m6a_io_rows_free(h)
    assert np.array_equal(part["run_npos"], full["run_npos"][pick])
    for j, r in enumerate(pick):
        a0, a1, b0, b1 = part["row_off"][j], part["row_off"][j + 1], full["row_off"][r], full["row_off"][r + 1]
        assert np.array_equal(part["row_pos"][a0:a1], full["row_pos"][b0:b1])
        assert np.array_equal(part["row_kmer"][a0:a1], full["row_kmer"][b0:b1])
        assert np.array_equal(part["row_feat"][a0:a1].view(np.uint64), full["row_feat"][b0:b1].view(np.uint64))


def test_sites_from_arrays_without_sites_write_the_headers(tmp_path):
    built = _io.NativeSites.from_arrays(np.zeros(1, np.int64), np.zeros(0, np.int64), b"", np.zeros(1, np.int64), np.zeros(0, np.uint32),
                                        np.zeros((0, 5), np.uint8), np.zeros(0))
    built.write_csv(str(tmp_path), [], [], [], write_header=True)
    assert (tmp_path / "data.site_proba.csv").read_text().splitlines() == [
        "transcript_id,transcript_position,n_reads,probability_modified,kmer,mod_ratio"]
    assert (tmp_path / "data.indiv_proba.csv").read_text().splitlines() == ["transcript_id,transcript_position,read_index,probability_modified"]
    built.close()


def test_sites_from_arrays_are_not_a_store(tmp_path):
    built = _io.NativeSites.from_arrays(np.array([0, 2], np.int64), np.array([7], np.int64), b"tx", np.array([0, 2], np.int64),
                                        np.zeros(1, np.uint32), np.frombuffer(b"GGACT", np.uint8).reshape(1, 5), np.array([1.0, 2.0]))
    with pytest.raises(_io.M6AIOError, match="no features"):
        built.save_store(str(tmp_path / "x.m6astore"))
    assert not os.path.exists(tmp_path / "x.m6astore")
    built.close()
