"""tests/csv_statement.py pinned to the bytes the product writes today: the HOST writer (NativeSites.from_arrays(...).write_csv,
m6a_io.cpp format_rows) equals the statement on the seeded edge arrays of tests/csv_edges.py, before the device writer is held to
the same statement (tests/test_gpu_csv_device.py)."""
import os

import numpy as np
import pytest

import csv_edges as E
import csv_statement as ST
from m6anet_amd import _io

CSVS = ("data.site_proba.csv", "data.indiv_proba.csv")


def host_texts(tmp_path, a, n_sites=None):
    sites = _io.NativeSites.from_arrays(a["off"], a["tx_pos"], a["tx_blob"], a["tx_off"], a["site_tx"], a["kmer5"], a["read_ids"],
                                        a.get("read_rep"), a.get("n_rep", 1))
    out = str(tmp_path)
    sites.write_csv(out, a["read_prob"], a["site_prob"], a["mod_ratio"], write_header=True, n_threads=3, n_sites=n_sites)
    sites.close()
    s, i = (open(os.path.join(out, f), "rb").read() for f in CSVS)
    assert s.startswith(ST.SITE_HEADER) and i.startswith(ST.INDIV_HEADER)
    return s[len(ST.SITE_HEADER):], i[len(ST.INDIV_HEADER):]


def statement_texts(a, **kw):
    return ST.texts(a["off"], a["tx_pos"], a["tx_blob"], a["tx_off"], a["site_tx"], a["kmer5"], a["read_ids"], a["read_prob"], a["site_prob"],
                    a["mod_ratio"], a.get("read_rep"), a.get("n_rep", 1), **kw)


def test_the_edge_arrays_hold_the_edges():
    c = E.cases()
    a = c["main"]
    assert {len(str(int(x))) for x in a["read_ids"]} >= set(range(1, 16)) and a["read_ids"].max() == 10 ** 15 - 1
    assert {len(str(int(x))) for x in a["tx_pos"] if x >= 0} == set(range(1, 20)) and a["tx_pos"].max() == 2 ** 63 - 1
    bags = set(np.diff(a["off"]).tolist())
    assert {20, 99, 100} <= bags and max(bags) > 1000
    assert {int(n) for n in np.diff(a["tx_off"])} >= {1, 2, 3, 4, 255, 4096}
    assert set(c["rep"]["read_rep"].tolist()) == {0, 9, 10}
    for arr in (a["read_prob"], a["site_prob"], a["mod_ratio"]):
        nan = arr[np.isnan(arr)]
        assert len(nan) >= 2 and {bool(np.signbit(x)) for x in nan} == {False, True}
    assert ST.declines(a["off"], a["read_ids"], a["read_prob"], a["site_prob"], a["mod_ratio"]) == 0
    # the ties are ties: the exact decimal expansion of m / 2^17 ends in 5 at the 17th decimal
    from fractions import Fraction
    for m in E.TIES_EVEN + E.TIES_UP:
        assert (Fraction(m, 2 ** 17) * 10 ** 17) % 10 == 5 and (Fraction(m, 2 ** 17) * 10 ** 17).denominator == 1
        down = int(Fraction(m, 2 ** 17) * 10 ** 16)
        assert ST.f16(m / 2.0 ** 17) == "0.%016d" % (down if m in E.TIES_EVEN else down + 1) and (down % 2 == 0) == (m in E.TIES_EVEN)


def test_statement_spells_the_special_values():
    assert ST.f16(np.float32(1)) == "1.0000000000000000" and ST.f16(0.0) == "0.0000000000000000"
    assert ST.f16(np.nextafter(np.float32(1), np.float32(0))) == "0.9999999403953552"
    assert ST.f16(E.f32_bits(1)) == "0.0000000000000000" and ST.f16(2.0 ** -55) == "0.0000000000000000"
    from fractions import Fraction
    half = Fraction(1, 2 * 10 ** 16)                         # 5e-17 as a double lies on one side of half a unit of the 16th decimal
    assert Fraction(5e-17) != half and ST.f16(5e-17) == ("0.0000000000000001" if Fraction(5e-17) > half else "0.0000000000000000")
    assert ST.f16(6e-17) == "0.0000000000000001" and ST.f16(4e-17) == "0.0000000000000000"
    assert ST.f16(1.9999999999999998) == "1.9999999999999998"
    assert ST.f16(E.f32_bits(0xffc00000)) == "-nan" and ST.f16(E.f64_bits(0x7ff8000000000000)) == "nan"
    assert [ST.value_declined(v) for v in (0.0, -0.0, 1.9999999999999998, 2.0, -1e-300, float("nan"), float("inf"), -float("inf"))] == \
        [False, True, False, True, True, False, False, False]
    assert [ST.id_declined(v) for v in (0.0, -0.0, 10.0 ** 15 - 1, 1e15, 2.5, -1.0, float("nan"), float("inf"))] == \
        [False, True, False, True, True, True, True, True]
    for name, (a, n) in E.declined_cases().items():
        assert ST.declines(a["off"], a["read_ids"], a["read_prob"], a["site_prob"], a["mod_ratio"]) == n == 1, name


@pytest.mark.parametrize("name", ["main", "rep", "empty", "one", "wide"])
def test_host_writer_equals_the_statement(tmp_path, name):
    a = E.cases()[name]
    want = statement_texts(a)
    got = host_texts(tmp_path, a)
    assert got[0] == want[0], name
    assert got[1] == want[1], name
    S = len(a["tx_pos"])
    if S > 2:                                                # the first sites only (--drop_unflushed_tail): a prefix of the same texts
        part = host_texts(tmp_path, a, n_sites=S // 2)
        assert part == statement_texts(a, site_end=S // 2) and want[0].startswith(part[0]) and want[1].startswith(part[1])
