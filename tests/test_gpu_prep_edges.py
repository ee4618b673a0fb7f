"""The prep kernels (m6anet_amd/csrc/m6a_prep.hip) against the plain statement of the operation (tests/eventalign_statement.py),
not through the host: on every generated family of tests/eventalign_gen.py and three seeds, at the default upload chunk and at
chunks of 4 KB and 12 KB, the front half's table and the back half's arrays equal the statement's bit for bit, and a run is
handed to the host exactly where the statement's `declines` says it may be."""
import os

import numpy as np
import pytest

import eventalign_gen as G
import eventalign_statement as S
from m6anet_amd import _io
from test_eventalign_statement import CASES, assert_sites_are_the_statement, assert_table_is_the_statement, hct116, message
from test_gpu_eventalign_inference import two_step_and_fused

pytestmark = pytest.mark.gpu
CHUNKS_KB = [None, 4, 12]          # the library rounds a chunk up to whole 4 KB blocks; 12 puts the chunk edges on other lines than 4


def set_chunk(monkeypatch, chunk_kb):
    if chunk_kb:
        monkeypatch.setenv("M6A_PREP_CHUNK_KB", str(chunk_kb))
    else:
        monkeypatch.delenv("M6A_PREP_CHUNK_KB", raising=False)


def one_correct_call(tmp_path):
    """after an error: the same process still computes the plain family"""
    c = G.case("plain", 1)
    ev, _ = c.write(tmp_path)
    with _io.prep_on_device(ev, 1) as t:
        assert (assert_table_is_the_statement(_io.table_arrays(t.contents), c) == 0).all()


@pytest.mark.parametrize("chunk_kb", CHUNKS_KB)
@pytest.mark.parametrize("family, seed", CASES)
def test_device_table_is_the_statement(tmp_path, monkeypatch, family, seed, chunk_kb):
    set_chunk(monkeypatch, chunk_kb)
    c, spec = G.case(family, seed), G.FAMILIES[family]
    ev, idx = c.write(tmp_path)
    if "error" in spec:
        with pytest.raises(_io.M6AIOError) as e:
            _io.prep_on_device(ev, c.nn, idx)
        assert e.value.code == spec["error"][0] and message(e).startswith(spec["error"][1])
        one_correct_call(tmp_path)
        return
    with _io.prep_on_device(ev, c.nn, idx) as t:
        a = _io.table_arrays(t.contents)
    status = assert_table_is_the_statement(a, c, (family, seed, chunk_kb))
    # handed to the host exactly where the statement allows it: a device that declined everything would pass every row comparison
    assert [bool(s) for s in status] == [S.declines(c.data, r) for r in c.runs], (family, seed, chunk_kb)


SITE_CASES = [(f, s) for f, s in CASES if G.FAMILIES[f].get("nn", 1) == 1 and f != "midline"]      # the back half builds its own index


@pytest.mark.parametrize("chunk_kb", CHUNKS_KB)
@pytest.mark.parametrize("family, seed", SITE_CASES)
def test_device_sites_are_the_statement(tmp_path, monkeypatch, family, seed, chunk_kb):
    set_chunk(monkeypatch, chunk_kb)
    c = G.case(family, seed)
    ev, _ = c.write(tmp_path)
    args = (c.kw.get("readcount_min", 1), c.kw.get("readcount_max", 1000), c.kw.get("min_segment_count", 20))
    if c.error is not None:                                   # the host's code and text, then one correct call
        with pytest.raises(_io.M6AIOError) as host:
            _io.dataprep(ev, str(tmp_path / "host"), n_threads=2, **c.kw)
        with pytest.raises(_io.M6AIOError) as e:
            _io.prep_sites(ev, *args, norm=None, n_threads=2)
        assert e.value.code == host.value.code == c.error[0] and message(e) == message(host) and message(e).startswith(c.error[1])
        one_correct_call(tmp_path)
        return
    for norm in (None, hct116()):
        want = c.sites if norm is None else S.sites(c.names, c.runs, norm=norm, **c.kw)
        with _io.prep_sites(ev, *args, norm=norm, n_threads=2) as p:
            X, km, off = p.inputs()
            tag = (family, seed, chunk_kb, norm is not None)
            assert p.n_sites == len(want["tx_pos"]) and p.n_reads == len(want["read_ids"]), tag
            assert_sites_are_the_statement(X, km, off, p.tx_pos, p.read_ids, [p.names[t] for t in p.site_tx],
                                           [bytes(k[1:6]).decode() for k in p.kmer7], want, tag)
            assert np.array_equal(p.off, want["off"]) and [bytes(k).decode() for k in p.kmer7] == want["kmer7"], tag


@pytest.mark.parametrize("family", ["split_runs", "split_rows"])
def test_split_sorts_end_to_end(tmp_path, family):
    """`eventalign_inference`'s two CSVs equal `dataprep` + `inference`'s, byte for byte, where the sorts take more than one key"""
    ev, _ = G.case(family, 1).write(tmp_path)
    two_step_and_fused(tmp_path, ev, family)


@pytest.mark.parametrize("seed", G.SEEDS)
def test_skip_index_with_rows_that_end_inside_a_line(tmp_path, seed):
    """`dataprep --device gpu --skip_index` on an index whose rows end mid-line: the device hands those runs to the host, and the
    files lead to the statement's arrays (the run is its byte range, cut where the index says)"""
    c = G.case("midline", seed)
    ev, _ = c.write(tmp_path)
    out = str(tmp_path / "gpu")
    os.makedirs(out)
    open(os.path.join(out, "eventalign.index"), "w").write(c.index)
    _io.dataprep(ev, out, n_threads=2, skip_index=True, device="gpu")
    assert open(os.path.join(out, "eventalign.index")).read() == c.index
    nat = _io.NativeSites([out], 20, None, 2)
    n = len(nat.tx_pos)
    assert_sites_are_the_statement(nat.X, nat.site_kmers, nat.off, nat.tx_pos, nat.read_id_values, [nat.tx_id(i) for i in range(n)],
                                   [nat.kmer5(i) for i in range(n)], c.sites, seed)
    nat.close()
