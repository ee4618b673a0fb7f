"""m6a_ks_exact on the CPU (m6anet_amd/csrc/m6a_ks_exact.h): libm6a_io.so's m6a_io_ks_exact gives the bits tests/ks_exact_statement.py
states on every item tests/test_gpu_ks_exact.py holds the kernel to (tests/ks_exact_cases.py: the crossed sizes, the named items, the
distinct items of the mixed launch); the bags swapped give the same bits; argument errors leave p alone; and
tests/ks_exact_core_main.cpp, a program of its own built here with ASan and UBSan, runs the core against the recurrence over the whole
table and returns 0."""
import os
import subprocess

import numpy as np
import pytest

import ks_exact_cases as KE
from m6anet_amd import _io, ranksum

HERE = os.path.dirname(os.path.abspath(__file__))
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
M6A_IO_EINVAL = -1
LISTS = {"crossed sizes": KE.cross, "named items": lambda: list(KE.SPECIAL.values()), "mixed launch": lambda: KE.distinct(KE.mixed(4096))}


@pytest.mark.parametrize("name", LISTS)
def test_host_core_gives_the_statement(name):
    items = LISTS[name]()
    n, m, h = KE.arrays(items)
    p = np.full(len(items) + 2, 7.0)                             # a sentinel on either side
    assert _io.load().m6a_io_ks_exact(n.ctypes.data, m.ctypes.data, h.ctypes.data, len(items), p.ctypes.data + 8) == 0
    assert p[0] == 7.0 and p[-1] == 7.0
    want = np.array([KE.statement(it) for it in items])
    bad = [(it, g, w) for it, g, w in zip(items, p[1:-1], want) if not KE.same_bits([g], [w])]
    assert not bad, (name, len(bad), bad[:5])
    assert KE.same_bits(_io.ks_exact(n, m, h), want) and KE.same_bits(KE.host(items), want)
    assert KE.same_bits(_io.ks_exact(m, n, h), want)             # the bags swapped: the same bits


def test_named_items_are_what_their_names_say():
    p = dict(zip(KE.SPECIAL, KE.host(list(KE.SPECIAL.values()))))
    assert sorted(k for k, v in p.items() if np.isnan(v)) == sorted(KE.NAN)
    assert p["a band narrower than one cell"] == 1.0 and p["a band that covers the grid"] == 0.0 and p["an h far beyond the grid"] == 0.0
    assert 0.0 < p["a subnormal result"] < 2.0 ** -1022 and p["a zero result"] == 0.0
    assert all(0.01 < p[k] < 0.99 for k in ("the short cap", "the short cap, longer bag", "the cell cap"))
    assert KE.same_bits([p["the cell cap"]], [p["the cell cap, swapped"]])
    n, m, h = KE.arrays(KE.cross())
    got = _io.ks_exact(n, m, h)
    assert np.isnan(got[h < 0]).all() and (got[h == 0] == 1.0).all() and (got[h > n * m] == 0.0).all()
    assert not np.isnan(got[h >= 0]).any() and ((got[h >= 0] >= 0) & (got[h >= 0] <= 1)).all()


def test_shapes_and_ks_h():
    d_pos, d_neg = np.array([[3, -1], [0, 9]]), np.array([[5, -1], [0, 2]])
    h = ranksum.ks_h(d_pos, d_neg)
    assert h.dtype == np.int64 and h.tolist() == [[5, -1], [0, 9]]
    p = _io.ks_exact(np.full((2, 2), 4), np.full((2, 2), 5), h)
    assert p.shape == (2, 2) and np.isnan(p[0, 1]) and p[1, 0] == 1.0 and KE.same_bits([p[0, 0]], [KE.statement((4, 5, 5))])
    with pytest.raises(ValueError):
        _io.ks_exact([1, 2], [1], [1, 2])


def test_argument_errors_leave_the_output_alone():
    f = _io.load().m6a_io_ks_exact
    n, m, h = KE.arrays([(20, 20, 100), (5, 7, 3)])
    p = np.full(2, 7.0)
    ptr = lambda x: x.ctypes.data                                # noqa: E731
    for args in ((None, ptr(m), ptr(h), 2, ptr(p)), (ptr(n), None, ptr(h), 2, ptr(p)), (ptr(n), ptr(m), None, 2, ptr(p)),
                 (ptr(n), ptr(m), ptr(h), -1, ptr(p))):
        assert f(*args) == M6A_IO_EINVAL and (p == 7.0).all()
    assert f(ptr(n), ptr(m), ptr(h), 2, None) == M6A_IO_EINVAL
    assert f(None, None, None, 0, None) == 0 and f(ptr(n), ptr(m), ptr(h), 0, ptr(p)) == 0 and (p == 7.0).all()   # no items: nothing to do


def test_text_with_exact_p_values():
    """the p_method column, the fallback for an item m6a_ks_exact leaves undefined, and the text without p_exact as it was"""
    tx, pos, kmer, n_a, n_b = ["T1", "T1", "T2"], [5, 9, 2], ["AAACA", "GGACT", "TGACC"], [20, 3000, 4], [20, 3000, 0]
    d_pos, d_neg, med = [160, 900000, -1], [40, 100, -1], [0.5, 0.25, float("nan")]
    plain = ranksum.ks_text(tx, pos, kmer, n_a, n_b, d_pos, d_neg, med, med)
    assert plain.splitlines()[0] == ranksum.KS_HEADER and all(ln.count(",") == 11 for ln in plain.splitlines())
    p_exact = _io.ks_exact(n_a, n_b, ranksum.ks_h(d_pos, d_neg))
    assert not np.isnan(p_exact[0]) and np.isnan(p_exact[1:]).all()              # 3000 > 2047 reads; an undefined pair
    text = ranksum.ks_text(tx, pos, kmer, n_a, n_b, d_pos, d_neg, med, med, p_exact=p_exact)
    rows, old = [ln.split(",") for ln in text.splitlines()], [ln.split(",") for ln in plain.splitlines()]
    assert rows[0] == old[0] + ["p_method"] and [r[:10] for r in rows] == [r[:10] for r in old]
    assert [r[12] for r in rows[1:]] == ["exact", "asymptotic", "asymptotic"]
    assert rows[1][10] == repr(float(p_exact[0])) and rows[2][10] == old[2][10] and rows[3][10] == rows[3][11] == "nan"
    p = np.array([float(r[10]) for r in rows[1:]])
    assert [r[11] for r in rows[1:]] == ["nan" if np.isnan(q) else repr(float(q)) for q in ranksum.bh(p)]
    nine = lambda x: np.repeat(np.asarray(x)[:, None], 9, axis=1)                # noqa: E731
    signal = ranksum.signal_ks_text(tx, pos, kmer, n_a, n_b, nine(d_pos), nine(d_neg), nine(med), nine(med), p_exact=nine(p_exact))
    lines = signal.splitlines()
    assert lines[0] == ranksum.SIGNAL_KS_HEADER + ",p_method" and len(lines) == 28
    assert [ln.split(",")[14] for ln in lines[1:]] == ["exact"] * 9 + ["asymptotic"] * 18


def test_core_program_under_sanitizers(tmp_path):
    exe = str(tmp_path / "ks_exact_core")
    subprocess.run(["g++", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g", "-O1", "-std=c++17",
                    "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(HERE, "..", "m6anet_amd", "csrc"),
                    os.path.join(HERE, "ks_exact_core_main.cpp"), "-o", exe], check=True, timeout=300)
    r = subprocess.run([exe], env=ENV, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stdout[-2000:], r.stderr[-3000:])
    assert r.stdout.splitlines()[-1] == "0 failures"
