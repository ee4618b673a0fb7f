"""The read-name core the HIP kernels compile (m6anet_amd/csrc/m6a_uuid.h) on the CPU: tests/uuid_core_main.cpp, a program of its
own built here with ASan and UBSan and run directly, held to tests/read_names_statement.py on every generated name, every malformed
spelling and every truncation of a good name; libm6a_io.so's exports of the same core; and the generated families themselves --
each is the statement's twin of its named file and gives at least one site.  tests/test_gpu_read_names.py holds the kernels to the
same statement."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import read_names_gen as NG
import read_names_statement as RS
from m6anet_amd import _io

HERE = os.path.dirname(os.path.abspath(__file__))
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")


@pytest.fixture(scope="module")
def core(tmp_path_factory):
    d = tmp_path_factory.mktemp("uuid_core")
    exe = str(d / "uuid_core")
    subprocess.run(["g++", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g", "-O1", "-std=c++17",
                    "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(HERE, "..", "m6anet_amd", "csrc"), os.path.join(HERE, "uuid_core_main.cpp"),
                    "-o", exe], check=True, timeout=300)

    def run(mode, lines):
        p = d / (mode + ".txt")
        p.write_bytes(b"".join(l + b"\n" for l in lines))
        r = subprocess.run([exe, mode, str(p)], env=ENV, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and not r.stderr, (r.returncode, r.stdout[-300:], r.stderr[-3000:])
        out = r.stdout.splitlines()
        assert len(out) == len(lines)
        return out
    return run


def all_names():
    return [v for f in NG.FAMILIES for v in NG.case(f).names]


def test_statement_on_its_own_examples():
    assert RS.parse(NG.GOOD) == 0x3f2a9c1e7b4d4e8a9f105c6d7e8f9a0b and RS.show(RS.parse(NG.GOOD)) == NG.GOOD
    assert RS.parse(b"0" * 8 + b"-0000-0000-0000-" + b"0" * 12) == 0 and RS.show(2 ** 128 - 1) == b"ffffffff-ffff-ffff-ffff-ffffffffffff"
    assert all(RS.parse(s) is None for s in NG.SPELLINGS.values())
    assert RS.table([1, 2 ** 127]).tolist() == [[0] * 15 + [1], [128] + [0] * 15]
    assert RS.indiv(b"h\nT,1,3,5.0,0.5\n", [[7, 8, 9, 10, 11, 12]]) == b"h\nT,1,3," + RS.show(12) + b",0.5\n"
    assert RS.indiv(b"h\nT,1,2_1,0.5\n", [[7], [8, 9, 10]]) == b"h\nT,1," + RS.show(10) + b"_1,0.5\n"


def test_every_family_is_its_twin_and_has_sites():
    for f in NG.FAMILIES:
        c = NG.case(f)
        twin, names = RS.twin(c.named)
        assert twin == c.twin and names == c.names and len(set(names)) == len(names), f
        assert NG.n_sites(c.twin) > 0, f
    assert len(NG.case("radix").names) == NG.radix_tile() + 1 == 4097
    d = NG.case("descending").names
    assert d == sorted(d, reverse=True)
    a = NG.case("again")
    runs = [r["read"] for r in RS.S.index(a.twin)[1]]
    assert runs.count(3) == 2 and runs.count(5) == 2 and runs.index(3) + 1 < len(runs) - 1 - runs[::-1].index(3)    # not adjacent
    for kb in NG.WINDOWS_KB:                                   # a cut between two runs of one name, and a window's end inside a run
        kinds = [k for *_, k in NG.cuts(NG.case("windows").named, kb << 10)]
        assert len(kinds) > 1 and any("same_name" in k for k in kinds) and any("inside" in k for k in kinds), kb


def test_replicate_files_share_names_in_pooled_sites():
    reps = NG.replicates("split")
    for named, twin, names in reps:
        assert RS.twin(named) == (twin, names)
    assert set(reps[0][2]) & set(reps[1][2]) and reps[1][2][0] == reps[0][2][3]          # a shared name has another index in each file
    assert NG.shared_in_pooled_sites(reps)


def test_malformed_files_name_the_lowest_offset():
    for sp in NG.SPELLINGS:
        for place in NG.PLACES:
            data, at = NG.malformed(sp, place)
            with pytest.raises(RS.S.StatementError) as e:
                RS.twin(data)
            assert e.value.code == RS.S.EFORMAT and e.value.text == "read name at byte %d: not a lowercase UUID" % at
            assert data[at:at + len(NG.SPELLINGS[sp])] == NG.SPELLINGS[sp]
    for first in (True, False):
        data, text = NG.short_and_bad(first)
        with pytest.raises(RS.S.StatementError) as e:
            RS.twin(data)
        assert e.value.text == text and text.startswith("short line" if first else "read name")


def test_core_parses_and_formats_as_the_statement(core):
    fields = [RS.show(v) for v in all_names()] + list(NG.SPELLINGS.values()) + [RS.show(0), RS.show(2 ** 128 - 1)]
    for got, f in zip(core("fields", fields), fields):
        v = RS.parse(f)
        assert got == ("refused" if v is None else "%032x %s" % (v, RS.show(v).decode())), f


def test_core_on_every_truncation(core):
    texts = [NG.GOOD + b"0123", NG.GOOD + b"-abc", RS.show(2 ** 128 - 1) + b"\tfff", NG.GOOD.upper() + b"0000"]
    assert all(len(t) == 40 for t in texts)
    for got, t in zip(core("cuts", texts), texts):
        want = "".join("r" if RS.parse(t[:n]) is None else "a" for n in range(41))
        assert got == want and len(got) == 41, t
    assert core("cuts", texts[:1])[0] == "r" * 36 + "a" + "r" * 4


def test_library_exports_the_core():
    L = _io.load()
    out = (C.c_uint8 * 16)()
    text = C.create_string_buffer(36)
    for v in all_names()[:200] + [0, 2 ** 128 - 1]:
        s = RS.show(v)
        assert L.m6a_io_uuid_parse(s, len(s), out) == 1 and bytes(out) == v.to_bytes(16, "big")
        L.m6a_io_uuid_format(out, text)
        assert text.raw == s
    for s in NG.SPELLINGS.values():
        assert L.m6a_io_uuid_parse(s, len(s), out) == 0
    assert np.array_equal(RS.table(all_names()[:3]), np.frombuffer(b"".join(v.to_bytes(16, "big") for v in all_names()[:3]), np.uint8).reshape(3, 16))
