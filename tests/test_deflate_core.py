"""The BGZF deflate core the HIP kernels compile (m6anet_amd/csrc/m6a_deflate.h), on the CPU: through libm6a_io.so's
m6a_io_bgzf_deflate, where the 64 parts of a block are a loop, and through tests/deflate_core_main.cpp, a program of its own built
here with ASan and UBSan.  tests/test_gpu_deflate.py holds the kernels to the bytes checked here.

Every output must be a file that tests/bgzf_statement.py and gzip inflate to the text, of blocks with ISIZE <= 65 280 and at most
65 536 bytes, ended by the 28-byte marker, and the same bytes on a second call."""
import os
import subprocess
import zlib

import deflate_inputs as DI
from m6anet_amd import _io, bgzf

HERE = os.path.dirname(os.path.abspath(__file__))


def test_every_input_round_trips_and_is_the_same_twice():
    texts = DI.texts()
    assert all(any(len(t) == n for t in texts.values()) for n in DI.SIZES)
    stored = 0
    for name, text in texts.items():
        st = {}
        out = _io.bgzf_deflate_host(text, st)
        types = DI.check(name, text, out)
        assert _io.bgzf_deflate_host(text) == out, name
        assert st["n_stored"] == sum(1 for t in types if t == [0]), name
        stored += st["n_stored"]
        if name.startswith("random_"):                       # nothing to find: a block of a part's size or more comes out stored,
            for (_, total, isize), t in zip(DI.blocks_of(out), types):       # 5 + 26 bytes over its text
                assert isize < DI.PART - 1 or (t == [0] and total == isize + 31), (name, isize, total, t)
    assert _io.bgzf_deflate_host(b"") == bgzf.EOF_MARKER
    print("%d texts, %d bytes, %d stored blocks" % (len(texts), sum(map(len, texts.values())), stored))


def test_sizing_call_is_the_issue_bound():
    import ctypes as C
    L, n = _io.load(), C.c_int64()
    for size in (0, 1, DI.BLOCK, DI.BLOCK + 1, 10 * DI.BLOCK):
        assert L.m6a_io_bgzf_deflate(b"x" * size, size, None, 0, C.byref(n), None) == 0
        assert n.value == (size + DI.BLOCK - 1) // DI.BLOCK * 65536 + 28
    buf = C.create_string_buffer(10)
    assert L.m6a_io_bgzf_deflate(b"x", 1, buf, 10, C.byref(n), None) == -1          # M6A_IO_EINVAL: the buffer is below the bound


def test_matches_are_found():
    """runs of one byte cost a match of 258 bytes each; a repeat across a part edge is found on both sides of it; the golden texts
    come to at most 0.45 of their size (zlib's fixed codes over the same parts give 0.35-0.36, literals alone more than 1.0)"""
    texts = DI.texts()
    same = _io.bgzf_deflate_host(texts["same_%d" % DI.BLOCK])
    assert len(same) < 26 + 28 + 64 * (DI.PART // 258 + 3) * 3
    edge, plain = texts["straddles_a_part_edge"], bytearray(texts["straddles_a_part_edge"])
    plain[950:1150] = bytes(255 - b for b in plain[950:1150])                      # the same text without the repeat
    assert len(_io.bgzf_deflate_host(edge)) < len(_io.bgzf_deflate_host(bytes(plain))) - 150
    for name in ("golden_config1", "golden_replicate"):
        ratio = len(_io.bgzf_deflate_host(texts[name])) / len(texts[name])
        print("%s: %.3f of the text" % (name, ratio))
        assert ratio <= 0.45, (name, ratio)


def test_core_as_a_sanitized_program_of_its_own(tmp_path):
    exe = str(tmp_path / "deflate_core")
    subprocess.run(["g++", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g", "-O1", "-std=c++17",
                    "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(HERE, "..", "m6anet_amd", "csrc"), os.path.join(HERE, "deflate_core_main.cpp"),
                    "-o", exe], check=True, timeout=300)
    texts = DI.texts()
    names = sorted(texts, key=lambda n: -len(texts[n]))    # the long ones first, dealt round
    for name in names:
        (tmp_path / name).write_bytes(texts[name])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    parts = [names[k::4] for k in range(4)]
    children = [subprocess.Popen([exe] + part, cwd=str(tmp_path), env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for part in parts]
    for part, child in zip(parts, children):
        out, err = child.communicate(timeout=600)
        assert child.returncode == 0 and not err, (child.returncode, out[-300:], err[-3000:])
        lines = out.splitlines()
        assert len(lines) == len(part)
        for name, line in zip(part, lines):
            st = {}
            want = _io.bgzf_deflate_host(texts[name], st)
            assert line.split("\t") == [name, str(len(want)), "%08x" % zlib.crc32(want), str(st["n_stored"])], (line, len(want))
