"""`eventalign_inference --read_representation` and --representation_dtype where no GPU is needed: the bytes of the .npy header and the
round rule (tests/repr_file_statement.py against NumPy, and m6anet_amd/csrc/m6a_npy.h as a program under ASan and UBSan against the
statement), the bindings' declarations, NULL arguments, and the argument errors of both commands."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import repr_file_statement as stmt
from m6anet_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
DATA = os.path.join(REPO, "tests", "golden", "ref_tests_data")
N_ROWS = [0, 1, 9, 10, 99999, 100000]       # the dictionary grows by a digit at 10 and at 100 000: the room behind it shrinks
DTYPES = ["float32", "float16"]

# off[] of the round tests: single reads, a large site in the middle, a large site last, empty sites
OFFS = {
    "ones": list(range(0, 41)),
    "mixed": [0, 20, 45, 345, 365, 390, 400, 1000],
    "big_last": [0, 3, 6, 600],
    "empty_sites": [0, 0, 5, 5, 5, 9, 9],
    "one_site": [0, 7],
}
ROUND_BYTES = [1, 128, 1024, 2560, 4096, 38400, 1 << 20]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n_rows", N_ROWS)
def test_statement_is_open_memmaps_header(tmp_path, n_rows, dtype):
    path = str(tmp_path / "a.npy")
    if n_rows:
        m = np.lib.format.open_memmap(path, mode="w+", dtype=np.dtype(dtype), shape=(n_rows, 32))
        del m
    else:                                                            # an empty file cannot be mapped; np.save writes the same header
        np.save(path, np.empty((0, 32), np.dtype(dtype)))
    want = stmt.header_bytes(n_rows, dtype)
    with open(path, "rb") as f:
        got = f.read(len(want) + 1)
    assert got[:len(want)] == want and len(want) == 128
    assert os.path.getsize(path) == stmt.row_offset(n_rows, dtype, n_rows)
    a = np.load(path, mmap_mode="r") if n_rows else np.load(path)
    assert a.shape == (n_rows, 32) and a.dtype == np.dtype(dtype) and a.flags.c_contiguous


@pytest.fixture(scope="module")
def npy_core(tmp_path_factory):
    d = tmp_path_factory.mktemp("npy_core")
    exe = str(d / "npy_core")
    subprocess.run(["g++", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g", "-O1", "-std=c++17",
                    "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(REPO, "m6anet_amd", "csrc"), os.path.join(HERE, "npy_core_main.cpp"),
                    "-o", exe], check=True, timeout=300)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")

    def run(*args):
        r = subprocess.run([exe] + [str(a) for a in args], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
        assert r.returncode == 0 and not r.stderr, (args, r.returncode, r.stdout[-300:], r.stderr[-3000:])
        return [l.split("\t") for l in r.stdout.splitlines()]
    return d, run


def test_program_writes_the_statements_header(npy_core):
    _, run = npy_core
    rows = run("header", *(N_ROWS + [2 ** 31, 61800000, 10 ** 18]))
    assert len(rows) == 2 * (len(N_ROWS) + 3)
    for n, dt, hexed in rows:
        assert bytes.fromhex(hexed) == stmt.header_bytes(int(n), DTYPES[int(dt)]), (n, dt)
    for (dt, at), name in zip(run("offset", 100000, 99999), DTYPES):
        assert int(at) == stmt.row_offset(100000, name, 99999) == 128 + 99999 * 32 * stmt.ITEMSIZE[name]


@pytest.mark.parametrize("name", sorted(OFFS))
def test_program_cuts_the_statements_rounds(npy_core, name):
    d, run = npy_core
    off = OFFS[name]
    np.array(off, np.int64).tofile(str(d / (name + ".bin")))
    for rb in ROUND_BYTES:
        rows = run("rounds", d / (name + ".bin"), rb)
        for (dt, widest, cuts), dtype in zip(rows, DTYPES):
            cut = [int(x) for x in cuts.split()]
            per = max(1, rb // (32 * stmt.ITEMSIZE[dtype]))
            # the statement's rule takes kilobytes; below one, state the rule here
            want = [0]
            while want[-1] < len(off) - 1:
                a = want[-1]
                b = a + 1
                while b < len(off) - 1 and off[b + 1] - off[a] <= per:
                    b += 1
                want.append(b)
            assert cut == want, (name, rb, dtype)
            if rb % 1024 == 0:
                assert cut == stmt.cut_rounds(off, len(off) - 1, rb // 1024, dtype)
            assert int(widest) == max(off[b] - off[a] for a, b in zip(cut, cut[1:]))
            assert cut[0] == 0 and cut[-1] == len(off) - 1 and all(b > a for a, b in zip(cut, cut[1:]))
            for a, b in zip(cut, cut[1:]):                           # whole sites; over the bound only as one site; and no round could take one more
                assert off[b] - off[a] <= per or b == a + 1
                assert b == len(off) - 1 or off[b + 1] - off[a] > per


def test_statement_round_edges():
    off = OFFS["mixed"]                                              # rows per site: 20 25 300 20 25 10 600
    assert stmt.cut_rounds(off, 7, 1, "float32") == [0, 1, 2, 3, 4, 5, 6, 7]                  # 8 rows: every site a round of its own
    assert stmt.cut_rounds(off, 7, 6, "float32") == [0, 2, 3, 5, 6, 7]                        # 48 rows: 20 + 25 fit, 20 + 25 + 10 do not
    assert stmt.cut_rounds(off, 7, 6, "float16") == [0, 2, 3, 6, 7]                           # 96 rows: 300 and 600 still alone
    assert stmt.cut_rounds(off, 7, 1 << 17, "float32") == [0, 7] and stmt.n_rounds(off, 7) == 1
    assert stmt.cut_rounds(off, 3, 6, "float32") == [0, 2, 3]                                 # n_sites_limit
    assert stmt.n_rounds([0, 0, 0], 2) == 0 and stmt.cut_rounds(off, 0) == [0]


def test_bindings_declare_the_header_signatures():
    h = open(os.path.join(REPO, "include", "m6a.h")).read()
    assert re.search(r"#define\s+M6A_REPR_F32\s+0\b", h) and re.search(r"#define\s+M6A_REPR_F16\s+1\b", h)
    m = re.search(r"\bint\s+m6a_read_representation_dtype\s*\(([^)]*)\)\s*;", h)
    assert m, "include/m6a.h does not declare m6a_read_representation_dtype"
    assert [re.sub(r"\s+", " ", p).strip() for p in m.group(1).split(",")] == [
        "m6a_ctx *ctx", "const float *X", "const uint8_t *site_kmers", "const int64_t *off", "int64_t n_sites", "void *repr", "int dtype",
        "float *read_prob"]
    m = re.search(r"\bint\s+m6a_prep_sites_write_read_representation\s*\(([^)]*)\)\s*;", h)
    assert m, "include/m6a.h does not declare m6a_prep_sites_write_read_representation"
    assert [re.sub(r"\s+", " ", p).strip() for p in m.group(1).split(",")] == [
        "m6a_prep_sites *p", "m6a_ctx *ctx", "const char *path", "int dtype", "int64_t n_sites_limit", "m6a_repr_write_stats *stats"]
    fields = re.search(r"typedef struct m6a_repr_write_stats \{(.*?)\} m6a_repr_write_stats;", h, re.S).group(1)
    fields = re.sub(r"/\*.*?\*/", "", fields, flags=re.S)
    names = [n.strip() for decl in fields.split(";") if decl.strip() for n in decl.strip().split(None, 1)[1].split(",")]
    assert names == [n for n, _ in _lib.ReprWriteStats._fields_]
    assert "M6A_REPR_ROUND_KB" in h and "open_memmap" in h
    L = _lib.load()
    for name in ("m6a_read_representation_dtype", "m6a_prep_sites_write_read_representation"):
        assert name in _lib.SYMBOLS and getattr(L, name).restype is C.c_int
    vp = C.c_void_p
    assert L.m6a_read_representation_dtype.argtypes == [vp, vp, vp, vp, C.c_int64, vp, C.c_int, vp]
    assert L.m6a_prep_sites_write_read_representation.argtypes == [vp, vp, C.c_char_p, C.c_int, C.c_int64, C.POINTER(_lib.ReprWriteStats)]
    assert _lib.REPR_DTYPES == {"float32": 0, "float16": 1}


def test_null_context_and_null_handle_fail(tmp_path):
    L = _lib.load()
    X, km, off = np.zeros((1, 9), np.float32), np.zeros((1, 3), np.uint8), np.array([0, 1], np.int64)
    for dtype, out in ((0, np.zeros((1, 32), np.float32)), (1, np.zeros((1, 32), np.float16)), (2, np.zeros((1, 32), np.float32))):
        assert L.m6a_read_representation_dtype(None, X.ctypes.data, km.ctypes.data, off.ctypes.data, 1, out.ctypes.data, dtype, None) == -1
        assert not out.any()
    path = tmp_path / "x.npy"
    st = _lib.ReprWriteStats()
    st.n_rounds = 7
    assert L.m6a_prep_sites_write_read_representation(None, None, os.fsencode(str(path)), 0, -1, C.byref(st)) == -1      # M6A_EINVAL
    assert not path.exists() and st.n_rounds == 0 and st.bytes == 0                # stats are filled on every return
    assert b"null" in L.m6a_prep_last_error()
    assert L.m6a_prep_sites_write_read_representation(None, None, None, 1, -1, None) == -1


def run_cli(command, args):
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, "-m", "m6anet_amd", command] + args, capture_output=True, text=True, cwd=REPO, env=env)


@pytest.mark.parametrize("value", ["float16", "float32"])
def test_dtype_without_the_flag_is_an_argument_error(tmp_path, value):
    out = tmp_path / "out"
    ea = os.path.join(REPO, "tests", "golden", "ref_tests_data", "eventalign.txt")      # never opened: the error comes first
    for command, head in (("inference", ["--input_dir", DATA]), ("eventalign_inference", ["--eventalign", ea])):
        for extra in (["--representation_dtype", value], ["--representation_dtype=" + value], ["--repr", value]):
            r = run_cli(command, head + ["--out_dir", str(out)] + extra)
            assert r.returncode == 2, (command, extra, r.returncode, r.stderr[-2000:])
            assert "--representation_dtype" in r.stderr and "--read_representation" in r.stderr
            assert not out.exists()
    r = run_cli("inference", ["--input_dir", DATA, "--out_dir", str(out), "--gpus", "2", "--representation_dtype", value])
    assert r.returncode == 2 and "--read_representation" in r.stderr and not out.exists()        # no rank was started either
    r = run_cli("inference", ["--input_dir", DATA, "--out_dir", str(out), "--read_representation", "--representation_dtype", "bfloat16"])
    assert r.returncode == 2 and "invalid choice" in r.stderr and not out.exists()


def test_read_repr_still_resolves_to_read_representation():
    from m6anet_amd.scripts import eventalign_inference, inference
    a = inference.full_parser().parse_args(["--input_dir", "x", "--out_dir", "y", "--read_repr"])
    assert a.read_representation is True and not hasattr(a, "representation_dtype")
    a = eventalign_inference.full_parser().parse_args(["--eventalign", "x", "--out_dir", "y", "--read_repr", "--representation_dtype", "float16"])
    assert a.read_representation is True and a.representation_dtype == "float16"
    a = eventalign_inference.full_parser().parse_args(["--eventalign", "x", "--out_dir", "y"])
    assert a.read_representation is False and not hasattr(a, "representation_dtype")
    flags = lambda p: {o for act in p._actions for o in act.option_strings}               # noqa: E731
    for mod in (inference, eventalign_inference):                   # the shared parsers are as they were: the flags live in full_parser()
        assert flags(mod.full_parser()) - flags(mod.command_parser()) == {"--read_representation", "--representation_dtype"}


@pytest.mark.parametrize("command", ["inference", "eventalign_inference"])
def test_help_names_the_flags(command):
    r = run_cli(command, ["--help"])
    assert r.returncode == 0
    text = re.sub(r"\s+", " ", r.stdout)
    assert "--read_representation" in text and "--representation_dtype {float32,float16}" in text
    assert "data.read_representation.npy" in text and "binary16" in text
