"""The rank-sum core on the CPU (m6anet_amd/csrc/m6a_ranksum.h): libm6a_io.so's m6a_io_site_ranksum gives the integers and the bits of z
that tests/ranksum_statement.py states, on the shapes tests/test_gpu_ranksum.py holds the kernel to (tests/ranksum_cases.py); its
argument errors leave the outputs alone; and tests/ranksum_core_main.cpp, a program of its own built here with ASan and UBSan, runs
the core on heap bags of exactly their sizes and returns 0."""
import os
import subprocess

import numpy as np
import pytest

import ranksum_cases as RC
from m6anet_amd import _io

HERE = os.path.dirname(os.path.abspath(__file__))
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
M6A_IO_EINVAL = -1


def call(pa, oa, pb, ob, ia, ib, P, optional=True, n_threads=0, fill=7):
    gt, eq, tie = (np.full(P + 2, fill, np.int64) for _ in range(3))      # a sentinel on either side of every output
    z = np.full(P + 2, float(fill), np.float64)
    ptr = lambda x, skip=0: None if x is None else x.ctypes.data + skip    # noqa: E731
    rc = _io.load().m6a_io_site_ranksum(ptr(pa), ptr(oa), oa.size - 1, ptr(pb), ptr(ob), ob.size - 1, ptr(ia), ptr(ib), P,
                                        ptr(gt, 8) if optional else None, ptr(eq, 8) if optional else None,
                                        ptr(tie, 8) if optional else None, ptr(z, 8), n_threads)
    for x in (gt, eq, tie, z):
        assert x[0] == fill and x[-1] == fill
    return rc, gt[1:-1], eq[1:-1], tie[1:-1], z[1:-1]


@pytest.mark.parametrize("name", ["crossed and special", "backwards", "0 drawn", "1 drawn", "65 drawn", "4097 drawn", "identity"])
def test_host_core_gives_the_statement(name):
    pa, oa, pb, ob, _ = RC.sets()
    ia, ib = (None, None) if name == "identity" else RC.pair_lists()[name]
    P = RC.n_sites() if ia is None else ia.size
    want = RC.want(ia, ib)
    for n_threads in (1, 5):
        rc, *got = call(pa, oa, pb, ob, ia, ib, P, n_threads=n_threads)
        assert rc == 0
        for g, w, what in zip(got, want, ("gt", "eq", "tie", "z")):
            assert RC.same_bits(g, w), (name, what)
    rc, gt, eq, tie, z = call(pa, oa, pb, ob, ia, ib, P, optional=False)   # the three counts left out
    assert rc == 0 and RC.same_bits(z, want[3]) and (gt == 7).all() and (eq == 7).all() and (tie == 7).all()


def test_the_cases_hold_what_they_are_named_for():
    """a NaN, an empty bag: undefined; everything else defined; all pooled values equal: z = 0"""
    _, oa, _, ob, names = RC.sets()
    gt, eq, tie, z = RC.want()
    K = len(RC.SIZES)
    for k, name in enumerate(names):
        undefined = name.startswith(("empty", "both empty", "nan"))
        assert (gt[K + k] == -1 and eq[K + k] == -1 and tie[K + k] == -1 and np.isnan(z[K + k])) == undefined, name
    k = K + names.index("all equal")
    assert (gt[k], eq[k], tie[k]) == (0, 70 * 33, 103 ** 3 - 103) and z[k] == 0 and not np.signbit(z[k])
    k = K + names.index("signed zeros")
    assert (gt[k], eq[k]) == (2, 6)                             # three zeros of a equal two of b, whatever their signs; 0.25 is above both
    k = K + names.index("complete separation")
    assert (gt[k], eq[k], tie[k]) == (30 * 25, 0, 0) and z[k] > 6


def test_argument_errors_leave_the_outputs_alone():
    pa, oa, pb, ob, _ = RC.sets()
    S = RC.n_sites()
    good = np.zeros(3, np.int64)
    for ia, ib, P, why in ((np.array([0, S, 1]), good, 3, "an index one past the set"), (good, np.array([0, -1, 1]), 3, "a negative index"),
                           (None, None, S - 1, "the identity with another number of pairs"), (good, None, 3, "one index array alone")):
        rc, gt, eq, tie, z = call(pa, oa, pb, ob, None if ia is None else ia.astype(np.int64), None if ib is None else ib.astype(np.int64), P)
        assert rc == M6A_IO_EINVAL and (gt == 7).all() and (eq == 7).all() and (tie == 7).all() and (z == 7).all(), why
    for bad in (np.array([1, 2, 3], np.int64), np.array([0, 2, 1], np.int64)):     # offsets that do not start at 0, that decrease
        rc, gt, _, _, z = call(pa, bad, pb, bad, None, None, 2)
        assert rc == M6A_IO_EINVAL and (gt == 7).all() and (z == 7).all()
    assert _io.load().m6a_io_site_ranksum(pa.ctypes.data, oa.ctypes.data, S, pb.ctypes.data, ob.ctypes.data, S, None, None, S, None, None, None,
                                          None, 0) == M6A_IO_EINVAL                # z is required
    assert _io.load().m6a_io_site_ranksum(None, None, 0, None, None, 0, None, None, 0, None, None, None, None, 0) == 0   # no pairs: nothing to do


def test_core_program_under_sanitizers(tmp_path):
    exe = str(tmp_path / "ranksum_core")
    subprocess.run(["g++", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g", "-O1", "-std=c++17",
                    "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(HERE, "..", "m6anet_amd", "csrc"),
                    os.path.join(HERE, "ranksum_core_main.cpp"), "-o", exe], check=True, timeout=300)
    r = subprocess.run([exe], env=ENV, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stdout[-2000:], r.stderr[-3000:])
    assert r.stdout.splitlines()[-1] == "0 failures"
