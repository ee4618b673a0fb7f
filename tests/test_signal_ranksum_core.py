"""m6a_site_signal_ranksum on the CPU: libm6a_io.so's m6a_io_site_signal_ranksum gives the integers and the bits of z that
tests/signal_ranksum_statement.py states, on the shapes tests/test_gpu_signal_ranksum.py holds the kernel to
(tests/signal_ranksum_cases.py), at 1 and at 4 threads; its optional outputs may be left out and its argument errors leave the outputs
alone; and tests/signal_ranksum_core_main.cpp, a program of its own built here with ASan and UBSan, runs the gather and the count on
heap rows of exactly their sizes and returns 0."""
import os
import subprocess

import numpy as np
import pytest

import signal_ranksum_cases as SC
from m6anet_amd import _io

HERE = os.path.dirname(os.path.abspath(__file__))
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
M6A_IO_EINVAL = -1


def call(Xa, oa, Xb, ob, ia, ib, P, optional=True, n_threads=0, fill=7):
    gt, eq, tie = (np.full(9 * P + 2, fill, np.int64) for _ in range(3))  # a sentinel on either side of every output
    z = np.full(9 * P + 2, float(fill), np.float64)
    ptr = lambda x, skip=0: None if x is None else x.ctypes.data + skip    # noqa: E731
    rc = _io.load().m6a_io_site_signal_ranksum(ptr(Xa), ptr(oa), oa.size - 1, ptr(Xb), ptr(ob), ob.size - 1, ptr(ia), ptr(ib), P,
                                               ptr(gt, 8) if optional else None, ptr(eq, 8) if optional else None,
                                               ptr(tie, 8) if optional else None, ptr(z, 8), n_threads)
    for x in (gt, eq, tie, z):
        assert x[0] == fill and x[-1] == fill
    return (rc,) + tuple(x[1:-1].reshape(P, 9) for x in (gt, eq, tie, z))


@pytest.mark.parametrize("name", SC.LISTS)
def test_host_core_gives_the_statement(name):
    Xa, oa, Xb, ob, _ = SC.sets()
    ia, ib = (None, None) if name == "identity" else SC.pair_lists()[name]
    P = SC.n_sites() if ia is None else ia.size
    want = SC.want(ia, ib)
    for n_threads in (1, 4):
        rc, *got = call(Xa, oa, Xb, ob, ia, ib, P, n_threads=n_threads)
        assert rc == 0
        for g, w, what in zip(got, want, ("gt", "eq", "tie", "z")):
            assert SC.same_bits(g, w), (name, what)
    rc, gt, eq, tie, z = call(Xa, oa, Xb, ob, ia, ib, P, optional=False)   # the three counts left out
    assert rc == 0 and SC.same_bits(z, want[3]) and (gt == 7).all() and (eq == 7).all() and (tie == 7).all()


def test_argument_errors_leave_the_outputs_alone():
    Xa, oa, Xb, ob, _ = SC.sets()
    S = SC.n_sites()
    good = np.zeros(3, np.int64)
    for ia, ib, P, why in ((np.array([0, S, 1]), good, 3, "an index one past the set"), (good, np.array([0, -1, 1]), 3, "a negative index"),
                           (None, None, S - 1, "the identity with another number of pairs"), (good, None, 3, "one index array alone")):
        rc, gt, eq, tie, z = call(Xa, oa, Xb, ob, None if ia is None else ia.astype(np.int64), None if ib is None else ib.astype(np.int64), P)
        assert rc == M6A_IO_EINVAL and (gt == 7).all() and (eq == 7).all() and (tie == 7).all() and (z == 7).all(), why
    for bad in (np.array([1, 2, 3], np.int64), np.array([0, 2, 1], np.int64)):     # offsets that do not start at 0, that decrease
        rc, gt, _, _, z = call(Xa, bad, Xb, bad, None, None, 2)
        assert rc == M6A_IO_EINVAL and (gt == 7).all() and (z == 7).all()
    L = _io.load()
    assert L.m6a_io_site_signal_ranksum(Xa.ctypes.data, oa.ctypes.data, S, Xb.ctypes.data, ob.ctypes.data, S, None, None, S, None, None, None,
                                        None, 0) == M6A_IO_EINVAL                  # z is required
    assert L.m6a_io_site_signal_ranksum(None, None, 0, None, None, 0, None, None, 0, None, None, None, None, 0) == 0   # no pairs: nothing to do


def test_core_program_under_sanitizers(tmp_path):
    exe = str(tmp_path / "signal_ranksum_core")
    subprocess.run(["g++", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g", "-O1", "-std=c++17",
                    "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(HERE, "..", "m6anet_amd", "csrc"),
                    os.path.join(HERE, "signal_ranksum_core_main.cpp"), "-o", exe], check=True, timeout=300)
    r = subprocess.run([exe], env=ENV, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stdout[-2000:], r.stderr[-3000:])
    assert r.stdout.splitlines()[-1] == "0 failures"
