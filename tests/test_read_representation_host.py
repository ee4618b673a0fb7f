"""m6a_read_representation and `inference --read_representation` where no GPU is needed: the binding's declaration, the NULL context, and
the argument errors of the command (which must come before anything is written or a device is touched)."""
import ctypes as C
import os
import re
import subprocess
import sys

from m6anet_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATA = os.path.join(REPO, "tests", "golden", "ref_tests_data")


def test_binding_declares_the_header_signature():
    """include/m6a.h: int m6a_read_representation(ctx, X, site_kmers, off, int64 n_sites, repr, read_prob)."""
    h = open(os.path.join(REPO, "include", "m6a.h")).read()
    m = re.search(r"\bint\s+m6a_read_representation\s*\(([^)]*)\)\s*;", h)
    assert m, "include/m6a.h does not declare m6a_read_representation"
    params = [re.sub(r"\s+", " ", p).strip() for p in m.group(1).split(",")]
    assert params == ["m6a_ctx *ctx", "const float *X", "const uint8_t *site_kmers", "const int64_t *off", "int64_t n_sites",
                      "float *repr", "float *read_prob"]
    assert re.search(r"#define\s+M6A_N_REPR\s+32\b", h)
    assert "m6a_read_representation" in _lib.SYMBOLS
    fn = _lib.load().m6a_read_representation
    assert fn.argtypes == [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    assert fn.restype is C.c_int


def test_null_context_is_einval():
    import numpy as np
    X, km, off = np.zeros((1, 9), np.float32), np.zeros((1, 3), np.uint8), np.array([0, 1], np.int64)
    out = np.zeros((1, 32), np.float32)
    rc = _lib.load().m6a_read_representation(None, X.ctypes.data, km.ctypes.data, off.ctypes.data, 1, out.ctypes.data, None)
    assert rc == -1                                                   # M6A_EINVAL
    assert not out.any()


def run_cli(args):
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, "-m", "m6anet_amd", "inference"] + args, capture_output=True, text=True, cwd=REPO, env=env)


def test_flag_with_two_gpus_is_an_argument_error(tmp_path):
    out = tmp_path / "out"
    r = run_cli(["--input_dir", DATA, "--out_dir", str(out), "--read_representation", "--gpus", "2"])
    assert r.returncode == 2, (r.returncode, r.stderr[-2000:])
    assert "--read_representation" in r.stderr
    assert not out.exists()
    r = run_cli(["--gpus=2", "--read_repr", "--input_dir", DATA, "--out_dir", str(out)])     # argparse's abbreviation, --flag=value
    assert r.returncode == 2 and "--read_representation" in r.stderr and not out.exists()


def test_help_lists_the_flag():
    r = run_cli(["--help"])
    assert r.returncode == 0
    text = re.sub(r"\s+", " ", r.stdout)
    assert "--read_representation" in text and "data.read_representation.npy" in text and "get_read_representation" in text
