"""The stream reader core (m6anet_amd/csrc/m6a_stream.h) on the CPU: tests/stream_core_main.cpp, a program of its own built here with
ASan and UBSan and run directly.  A 200 KB seeded buffer goes through a real pipe() in pieces of 1, 2, 7, 4095, 4096, 4097 and
65 537 bytes and in random pieces, the reader fills requests of 1, 4096, 65 536 and 100 000 bytes, and every combination gives the
buffer back byte for byte with at_eof() false until the last byte is consumed and true exactly then -- 200 KB is a whole number of
1-byte and of 4096-byte requests, so the stream also ends on a request's last byte.  An empty pipe is at its end at once, and a
closed descriptor is the error path with the text `cannot read <path>`.  The read-ahead ring over the reader (two buffers filled by
a thread of its own) is held to the same: buffers of 4096 and 65 536 bytes against the same pieces and requests, so that requests
end inside a buffer, on its last byte and behind it; the same program built with ThreadSanitizer runs three of those cases; and a
ring that is left while the writer still writes ends without waiting for the rest.  tests/test_gpu_pipe_input.py holds the stream front half
that reads through this core to the windowed file path."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
N = 200 << 10
PIECES = [1, 2, 7, 4095, 4096, 4097, 65537, 0]                # 0: random pieces
REQUESTS = [1, 4096, 65536, 100000]


def build(d, name, sanitizers):
    exe = str(d / name)
    subprocess.run(["g++"] + sanitizers + ["-fno-omit-frame-pointer", "-g", "-O1", "-std=c++17",
                    "-Wall", "-Wextra", "-Werror", "-pthread", "-I" + os.path.join(HERE, "..", "m6anet_amd", "csrc"),
                    os.path.join(HERE, "stream_core_main.cpp"), "-o", exe], check=True, timeout=300)

    def run(*args):
        r = subprocess.run([exe, "11", str(N)] + [str(a) for a in args], env=ENV, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and not r.stderr, (args, r.returncode, r.stdout[-300:], r.stderr[-3000:])
        return r.stdout.strip()
    return run


@pytest.fixture(scope="module")
def core(tmp_path_factory):
    return build(tmp_path_factory.mktemp("stream_core"), "stream_core", ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])


@pytest.fixture(scope="module")
def core_tsan(tmp_path_factory):
    return build(tmp_path_factory.mktemp("stream_core_tsan"), "stream_core_tsan", ["-fsanitize=thread"])


@pytest.mark.parametrize("request_bytes", REQUESTS)
@pytest.mark.parametrize("piece", PIECES)
def test_the_buffer_comes_back_whatever_the_pieces(core, piece, request_bytes):
    assert N % 4096 == 0 and N % 65536 != 0 and N % 100000 != 0    # requests that end on the last byte, and requests that end short
    assert core("pieces", piece, request_bytes) == "ok %d" % N


def test_an_empty_pipe_is_at_its_end_at_once(core):
    assert core("empty") == "ok 0"


def test_a_closed_descriptor_is_the_error_path(core):
    assert core("closed") == "ok 0"


@pytest.mark.parametrize("buffer_bytes", [4096, 65536])
@pytest.mark.parametrize("request_bytes", REQUESTS)
@pytest.mark.parametrize("piece", PIECES)
def test_the_ring_hands_out_the_same_bytes(core, piece, request_bytes, buffer_bytes):
    assert N % buffer_bytes == 0 or buffer_bytes == 65536       # the stream ends on a buffer's last byte, and inside one
    assert core("ring", piece, request_bytes, buffer_bytes) == "ok %d" % N


@pytest.mark.parametrize("piece, request_bytes, buffer_bytes", [(7, 100000, 4096), (4097, 4096, 4096), (0, 1, 65536)])
def test_the_ring_under_thread_sanitizer(core_tsan, piece, request_bytes, buffer_bytes):
    assert core_tsan("ring", piece, request_bytes, buffer_bytes) == "ok %d" % N
    assert core_tsan("abandon", piece, buffer_bytes) == "ok %d" % N


@pytest.mark.parametrize("piece", [1, 4096, 0])
def test_a_ring_that_is_left_does_not_wait_for_the_rest(core, piece):
    assert core("abandon", piece, 4096) == "ok %d" % N
