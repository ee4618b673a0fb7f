"""The read draw of the training step (m6anet_amd/csrc/m6a_train_draw.h, the text the HIP kernel compiles) on the CPU: as
tests/train_draw_main.cpp, a program of its own built here with ASan and UBSan and run directly, held to tests/train_statement.py."""
import os
import subprocess

import numpy as np
import pytest

import train_statement as TS

HERE = os.path.dirname(os.path.abspath(__file__))
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")


@pytest.fixture(scope="module")
def core(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("train_draw") / "train_draw")
    subprocess.run(["g++", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g", "-O1", "-std=c++17",
                    "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(HERE, "..", "m6anet_amd", "csrc"), os.path.join(HERE, "train_draw_main.cpp"),
                    "-o", exe], check=True, timeout=300)

    def run(*args):
        r = subprocess.run([exe] + [str(a) for a in args], env=ENV, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and not r.stderr, (r.returncode, r.stdout[-300:], r.stderr[-3000:])
        return r.stdout.splitlines()
    return run


def cases():
    out = []
    for n in list(range(20, 201)) + [1000, 5000, 2 ** 31 - 1]:
        for bag in (1, 20, 64):
            if bag <= n:
                out += [(seed, i, n, bag) for seed, i in ((0, 0), (25, n % 7), (2 ** 64 - 1, 2 ** 40 + n), (12345678901234567, 99999))]
    out += [(3, i, 64, 64) for i in range(50)] + [(3, i, 20, 20) for i in range(50)] + [(3, 0, 1, 1), (3, 1, 2, 1), (3, 2, 2, 2)]
    return out


def test_core_equals_the_statement_and_draws_distinct_reads_in_range(core, tmp_path):
    cs = cases()
    (tmp_path / "cases").write_text("".join("%d %d %d %d\n" % c for c in cs))
    out = core("draws", tmp_path / "cases")
    assert len(out) == len(cs)
    for (seed, i, n, bag), line in zip(cs, out):
        got = [int(t) for t in line.split()]
        assert got == TS.draw(seed, i, n, bag), (seed, i, n, bag)
        assert len(got) == bag == len(set(got)) and min(got) >= 0 and max(got) < n
    full = [sorted(int(t) for t in line.split()) for c, line in zip(cs, out) if c[2] == c[3]]
    assert full and all(f == list(range(len(f))) for f in full)            # bag = n: a permutation


def test_every_draw_is_uniform(core):
    """n = 23, 200 000 positions: draw j of a position is one of the 23 reads, independently from position to position, so each
    draw's histogram has a chi-square of 22 degrees of freedom; 48.268 is its 0.999 quantile.  Draw 0 of bag 1, and the first and
    the last draw of bag 20."""
    n, count = 23, 200000
    for bag, which in ((1, (0,)), (20, (0, 19))):
        rows = [np.array(line.split(), np.int64) for line in core("hist", 7, n, bag, count)]
        assert len(rows) == bag
        for j in which:
            assert rows[j].sum() == count
            chi2 = float(((rows[j] - count / n) ** 2 / (count / n)).sum())
            print("bag %d draw %d: chi-square %.2f" % (bag, j, chi2))
            assert chi2 < 48.268, (bag, j, chi2)
    # and the same positions through the statement, a prefix of them
    want = np.zeros(n, np.int64)
    for i in range(3000):
        want[TS.draw(7, i, n, 1)[0]] += 1
    got = np.array(core("hist", 7, n, 1, 3000)[0].split(), np.int64)
    assert np.array_equal(got, want)


def test_library_sample_equals_the_statement():
    from m6anet_amd.engine import train_sample
    g = np.random.Generator(np.random.PCG64(2))
    off = np.concatenate([[0], np.cumsum(g.integers(20, 400, 300))]).astype(np.int64)
    order = g.integers(0, 300, 1000).astype(np.int64)
    for bag, seed in ((20, 0), (1, 25), (13, 2 ** 63 + 5)):
        assert np.array_equal(train_sample(off, order, bag, seed), TS.sample(off, order, bag, seed))
    with pytest.raises(Exception):
        train_sample(off, order, 65, 0)
    with pytest.raises(Exception):
        train_sample(np.array([0, 5], np.int64), [0], 20, 0)
    with pytest.raises(ValueError):
        train_sample(off, [300], 20, 0)
