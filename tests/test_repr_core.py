"""The number core of the device data.json writer (m6anet_amd/csrc/m6a_repr.h) against Python's repr, without a GPU: as a program
of its own under ASan and UBSan (tests/repr_core_main.cpp), and as libm6a_io.so exports it (m6a_io_repr_core)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import repr_inputs
from m6anet_amd import _io

HERE = os.path.dirname(os.path.abspath(__file__))
INTS = [0, 1, 9, 10, 99, 100, 12345, 2 ** 31 - 1, 2 ** 31, 2 ** 32, 10 ** 15 - 1, 10 ** 15, 2 ** 53 - 1, 2 ** 53, 2 ** 53 + 1, 2 ** 63 - 1,
        -1, -10, -2 ** 31, -2 ** 53, -2 ** 63] + [10 ** k for k in range(19)] + [10 ** k - 1 for k in range(1, 19)]


@pytest.fixture(scope="module")
def program_output(tmp_path_factory):
    d = tmp_path_factory.mktemp("repr_core")
    exe = str(d / "repr_core")
    subprocess.run(["g++", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g", "-O1", "-std=c++17",
                    "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(HERE, "..", "m6anet_amd", "csrc"), os.path.join(HERE, "repr_core_main.cpp"),
                    "-o", exe], check=True, timeout=300)
    v, ok = repr_inputs.all_values()
    v.tofile(str(d / "doubles.bin"))
    np.array(INTS, np.int64).tofile(str(d / "ints.bin"))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, str(d / "doubles.bin"), str(d / "ints.bin")], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stdout[-300:], r.stderr[-3000:])
    lines = r.stdout.split("\n")
    assert lines[-1] == "" and len(lines) == v.size + len(INTS) + 1
    return v, ok, [l.split("\t") for l in lines[:v.size]], [l.split("\t") for l in lines[v.size:-1]]


def test_generator_covers_what_it_says():
    v, ok = repr_inputs.all_values()
    t = repr_inputs.taken()
    assert t.size > 200000 and ok.sum() == t.size and (~ok).sum() >= len(repr_inputs.declined()) + 4
    assert t.min() == 1e-4 and t.max() == np.nextafter(1e16, 0) and np.isnan(v).sum() == 1 and np.isinf(v).sum() == 2
    assert len(repr_inputs.golden_features()) == 63000 and all(1e-4 <= x < 1e16 for x in repr_inputs.golden_features())
    assert any("e" in repr(x) for x in v[~ok] if np.isfinite(x))          # what repr writes with an exponent is in the declined set


def test_program_gives_pythons_repr(program_output):
    v, ok, rows, _ = program_output
    want, want3 = repr_inputs.expected(v), repr_inputs.expected(v, round3=True)
    buf = C.create_string_buffer(40)
    L = _io.load()
    for i, (n, text, n3, text3) in enumerate(rows):
        x = float(v[i])
        if ok[i]:
            assert text == want[i] and int(n) == len(text) <= 24, (x.hex(), text, want[i])
            assert L.m6a_io_py_repr(x, buf) == int(n) and buf.value.decode() == text        # the host writer's own printer
        else:
            assert int(n) == -1 and text == "" and want[i] is None, (x, n, text)
        if want3[i] is None:                                         # rounded to 0.0, or out of range, or never finite
            assert int(n3) == -1 and text3 == "", (x, n3, text3)
        else:
            assert text3 == want3[i] and int(n3) == len(text3) <= 24, (x.hex(), text3, want3[i])
    assert sum(w is None for w in want) == int((~ok).sum()) and sum(w is None for w in want3) > int((~ok).sum())


def test_program_prints_integers_and_read_ids(program_output):
    rows = program_output[3]
    for k, (text, rid) in zip(INTS, rows):
        assert text == str(k)
        assert rid == (repr(float(k)) if 0 <= k < 2 ** 53 else "-"), (k, rid)
    assert repr(float(2 ** 53 - 1)) == "9007199254740991.0"


@pytest.mark.parametrize("round3", [False, True])
def test_exported_core_is_the_same(round3):
    v, ok = repr_inputs.all_values()
    want = repr_inputs.expected(v, round3)
    L = _io.load()
    buf = C.create_string_buffer(40)
    for x, w in zip(v.tolist(), want):
        n = L.m6a_io_repr_core(x, 1 if round3 else 0, buf)
        if w is None:
            assert n == -1 and buf.value == b"", (x, n)
        else:
            assert n == len(w) and buf.value.decode() == w, (x.hex(), buf.value, w)
