"""m6a_site_ks and m6a_site_signal_ks on the CPU (m6anet_amd/csrc/m6a_ks.h): libm6a_io.so's m6a_io_site_ks and m6a_io_site_signal_ks give
the integers and the medians' bits that tests/ks_statement.py states, on the shapes tests/test_gpu_ks.py and tests/test_gpu_signal_ks.py
hold the kernels to (tests/ks_cases.py), at 1 and at 4 threads; the two medians may be left out; argument errors leave the outputs alone;
and tests/ks_core_main.cpp, a program of its own built here with ASan and UBSan, runs the core on heap bags of exactly their sizes and
returns 0."""
import os
import subprocess

import numpy as np
import pytest

import ks_cases as KC
from m6anet_amd import _io

HERE = os.path.dirname(os.path.abspath(__file__))
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
M6A_IO_EINVAL = -1
CALLS = {"scalar": (KC.scalar, "m6a_io_site_ks"), "signal": (KC.signal, "m6a_io_site_signal_ks")}


def call(which, va, oa, vb, ob, ia, ib, P, optional=True, n_threads=0, fill=7):
    cases, symbol = CALLS[which]
    W = cases.columns
    d_pos, d_neg = (np.full(W * P + 2, fill, np.int64) for _ in range(2))       # a sentinel on either side of every output
    med_a, med_b = (np.full(W * P + 2, float(fill), np.float64) for _ in range(2))
    ptr = lambda x, skip=0: None if x is None else x.ctypes.data + skip    # noqa: E731
    rc = getattr(_io.load(), symbol)(ptr(va), ptr(oa), oa.size - 1, ptr(vb), ptr(ob), ob.size - 1, ptr(ia), ptr(ib), P, ptr(d_pos, 8), ptr(d_neg, 8),
                                     ptr(med_a, 8) if optional else None, ptr(med_b, 8) if optional else None, n_threads)
    for x in (d_pos, d_neg, med_a, med_b):
        assert x[0] == fill and x[-1] == fill
    shape = (P,) if W == 1 else (P, W)
    return (rc,) + tuple(x[1:-1].reshape(shape) for x in (d_pos, d_neg, med_a, med_b))


@pytest.mark.parametrize("name", KC.LISTS)
@pytest.mark.parametrize("which", ["scalar", "signal"])
def test_host_core_gives_the_statement(which, name):
    cases = CALLS[which][0]
    va, oa, vb, ob, _ = cases.sets()
    ia, ib, P = cases.pairs(name)
    want = cases.want(ia, ib)
    for n_threads in (1, 4):
        rc, *got = call(which, va, oa, vb, ob, ia, ib, P, n_threads=n_threads)
        assert rc == 0
        for g, w, what in zip(got, want, ("d_pos", "d_neg", "med_a", "med_b")):
            assert KC.same_bits(g, w), (name, what, np.argwhere(g != w)[:5])
    rc, d_pos, d_neg, med_a, med_b = call(which, va, oa, vb, ob, ia, ib, P, optional=False)   # the two medians left out
    assert rc == 0 and KC.same_bits(d_pos, want[0]) and KC.same_bits(d_neg, want[1]) and (med_a == 7).all() and (med_b == 7).all()


@pytest.mark.parametrize("which", ["scalar", "signal"])
def test_argument_errors_leave_the_outputs_alone(which):
    cases, symbol = CALLS[which]
    va, oa, vb, ob, _ = cases.sets()
    S = cases.n_sites()
    good = np.zeros(3, np.int64)
    for ia, ib, P, why in ((np.array([0, S, 1]), good, 3, "an index one past the set"), (good, np.array([0, -1, 1]), 3, "a negative index"),
                           (None, None, S - 1, "the identity with another number of pairs"), (good, None, 3, "one index array alone")):
        rc, *out = call(which, va, oa, vb, ob, None if ia is None else ia.astype(np.int64), None if ib is None else ib.astype(np.int64), P)
        assert rc == M6A_IO_EINVAL and all((o == 7).all() for o in out), why
    for bad in (np.array([1, 2, 3], np.int64), np.array([0, 2, 1], np.int64)):     # offsets that do not start at 0, that decrease
        rc, *out = call(which, va, bad, vb, bad, None, None, 2)
        assert rc == M6A_IO_EINVAL and all((o == 7).all() for o in out)
    f = getattr(_io.load(), symbol)
    med = np.full(cases.columns * S, 7.0)
    for d_pos, d_neg in ((None, med.ctypes.data), (med.ctypes.data, None)):          # d_pos and d_neg are required
        assert f(va.ctypes.data, oa.ctypes.data, S, vb.ctypes.data, ob.ctypes.data, S, None, None, S, d_pos, d_neg, None, None, 0) == M6A_IO_EINVAL
    assert (med == 7).all()
    assert f(None, None, 0, None, None, 0, None, None, 0, None, None, None, None, 0) == 0   # no pairs: nothing to do


def test_core_program_under_sanitizers(tmp_path):
    exe = str(tmp_path / "ks_core")
    subprocess.run(["g++", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g", "-O1", "-std=c++17",
                    "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(HERE, "..", "m6anet_amd", "csrc"),
                    os.path.join(HERE, "ks_core_main.cpp"), "-o", exe], check=True, timeout=300)
    r = subprocess.run([exe], env=ENV, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stdout[-2000:], r.stderr[-3000:])
    assert r.stdout.splitlines()[-1] == "0 failures"
