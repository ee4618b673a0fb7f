"""The data.json decode core the HIP kernels compile (m6anet_amd/csrc/m6a_json.h), on the CPU: as tests/json_core_main.cpp, a program
of its own built here with ASan and UBSan and run directly, held to tests/json_statement.py; the host half of the device loader
(m6a_io_info_open / m6a_io_info_rows) against the loader itself; and the `inference --loader` flag with what it refuses.
tests/test_gpu_json_loader.py holds the kernels to the same statement and the same loader."""
import ctypes as C
import gzip
import os
import random
import struct
import subprocess

import numpy as np
import pytest

import json_gen as JG
import json_statement as JS
from m6anet_amd import _io
from m6anet_amd.constants import PRETRAINED_CONFIGS
from m6anet_amd.data_utils import load_norm_factors

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")


@pytest.fixture(scope="module")
def core(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("json_core") / "json_core")
    subprocess.run(["g++", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g", "-O1", "-std=c++17",
                    "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(HERE, "..", "m6anet_amd", "csrc"), os.path.join(HERE, "json_core_main.cpp"),
                    "-o", exe], check=True, timeout=300)

    def run(*args):
        r = subprocess.run([exe] + [str(a) for a in args], env=ENV, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and not r.stderr, (r.returncode, r.stdout[-300:], r.stderr[-3000:])
        return r.stdout.splitlines()
    return run


def hct116():
    return load_norm_factors(PRETRAINED_CONFIGS["HCT116_RNA002"][2])


def norm_file(tmp_path, kmers):
    p = tmp_path / "norm.txt"
    p.write_text("".join(k + "\n" for k in kmers))
    return p


def records_file(path, sites):
    with open(path, "wb") as f:
        for s in sites:
            f.write(("%s\t%d\t%d\t%d\n" % (s.tx, s.pos, s.n_reads, len(s.text))).encode() + s.text + b"\n")
    return path


def generated_sites():
    rng = random.Random(3)
    good = [JG.good_site(rng, "ENST_A", 10 + d, n, JG.OTHER_KMERS[d], dress=d) for d, n in ((0, 3), (1, 1), (2, 2))]
    edge = JG.Site("ENST_E", 7, 2, JG.record("ENST_E", 7, JG.KMER, [JG.numbers()[k::2][:10] for k in (0, 1)], dress=1))
    return good + [edge], JG.declined_valid(rng), list(JG.malformed(rng).values())


def test_statement_on_its_own_examples():
    assert all(JS.accepted(t.encode()) for t in JG.numbers())
    assert not any(JS.accepted(t.encode()) for t in JG.DECLINED_TOKENS)
    assert len(JS.vocabulary()) == 66 and JS.vocabulary() == open(os.path.join(GOLD, "vocab66.txt")).read().split()
    good, valid, bad = generated_sites()
    for s in good:
        assert JS.walk(s.text, s.tx, s.pos, s.n_reads)[0] == "ok", s.text
    for s in valid + bad:
        got = JS.walk(s.text, s.tx, s.pos, s.n_reads)[0]
        assert got != "ok" and (s.reason is None or got == s.reason), (s.name, got)
    # every reason but "range" (a row of data.info, not a record) and "norm" (below) has a record
    assert {JS.walk(s.text, s.tx, s.pos, s.n_reads)[0] for s in valid + bad} >= set(JS.REASONS) - {"ok", "range", "norm", "row"}
    s = good[0]
    assert JS.walk(s.text, s.tx, s.pos, s.n_reads, {"AAAAA"})[0] == "norm"
    assert JS.walk(s.text.replace(b"], [", b"], x[", 1), s.tx, s.pos, s.n_reads)[0] == "row"


def test_every_accepted_token_has_the_bits_of_float(core, tmp_path):
    toks = JG.numbers() + list(JG.DECLINED_TOKENS)
    digits = {(len(t.lstrip("-").replace(".", "").lstrip("0")), len(t.partition(".")[2])) for t in JG.numbers()}
    assert digits >= {(nd, fr) for nd in range(1, 20) for fr in range(28)}
    (tmp_path / "tokens").write_text("".join(t + "\n" for t in toks))
    out = core("numbers", tmp_path / "tokens")
    assert len(out) == len(toks)
    n_ok = 0
    for t, line in zip(toks, out):
        if JS.accepted(t.encode()):
            assert line == "%016x" % struct.unpack("<Q", struct.pack("<d", float(t)))[0], (t, line, float(t).hex())
            n_ok += 1
        else:
            assert line == "declined", (t, line)
    assert n_ok == len(JG.numbers())
    # the same core inside libm6a_io.so: a token in a record
    L = _io.load()
    for t in JG.numbers()[::7]:
        rec = JG.record("T", 1, JG.KMER, [[t] * 10]).encode()
        v = np.zeros(10)
        assert L.m6a_io_json_walk(rec, len(rec), b"T", 1, 1, None, 0, v.ctypes.data, None) == 0
        assert v.tobytes() == np.full(10, float(t)).tobytes(), t


def test_records_carry_the_statements_reason_and_values(core, tmp_path):
    good, valid, bad = generated_sites()
    sites = good + valid + bad
    for norm in (None, sorted(hct116()), ["AAAAA"]):
        out = core("records", records_file(tmp_path / "recs", sites), "-" if norm is None else norm_file(tmp_path, norm))
        assert len(out) == len(sites)
        for s, line in zip(sites, out):
            reason, rows, kmer = JS.walk(s.text, s.tx, s.pos, s.n_reads, None if norm is None else set(norm))
            got = line.split(" ")
            assert got[0] == reason, (s.name, line[:80], reason)
            if reason == "ok":
                assert got[1] == kmer.decode()
                assert got[2:] == ["%016x" % struct.unpack("<Q", struct.pack("<d", v))[0] for r in rows for v in r], s.name
    assert sum(1 for s in good if JS.walk(s.text, s.tx, s.pos, s.n_reads)[0] == "ok") == len(good)


def test_every_cut_of_every_record_is_declined_in_bounds(core, tmp_path):
    good, valid, bad = generated_sites()
    sites = good + valid[:3] + bad
    out = core("cuts", records_file(tmp_path / "recs", sites), "-")
    assert len(out) == len(sites)
    for s, line in zip(sites, out):
        assert len(line) == len(s.text) + 1
        want = "".join(chr(ord("a") + JS.REASONS.index(JS.walk(s.text[:k], s.tx, s.pos, s.n_reads)[0])) for k in range(len(s.text) + 1))
        assert line == want, s.name
        body = len(s.text.rstrip(b" \n\r\t"))
        assert "a" not in line[:body], s.name                      # no proper cut of a record is a regular site


def golden_dir(tmp_path, name):
    if name == "ref_tests_data":
        return os.path.join(GOLD, name)
    d = tmp_path / name.replace("/", "_")
    d.mkdir()
    (d / "data.json").write_bytes(gzip.open(os.path.join(GOLD, name + ".data.json.gz")).read())
    (d / "data.info").write_bytes(open(os.path.join(GOLD, name + ".data.info"), "rb").read())
    return str(d)


@pytest.mark.parametrize("name", ["ref_tests_data", "dataprep_ref_run/msc1", "dataprep_ref_run/msc20_compress", "dataprep_synthetic/nn1"])
def test_no_site_of_the_golden_files_is_declined(core, tmp_path, name):
    d = golden_dir(tmp_path, name)
    for norm in ("-", norm_file(tmp_path, sorted(hct116()))):
        for min_reads in (1, 20):
            out = core("dir", d, norm, min_reads)
            sites, declined = map(int, out[0].split())
            assert sites > 0 or min_reads == 20
            assert declined == 0, out[:11]
    assert int(core("dir", d, "-", 1)[0].split()[0]) == sum(1 for _ in open(os.path.join(d, "data.info"))) - 1


# ---- the host half -------------------------------------------------------------------------------------------------------------

def info_table(d, min_reads):
    L, h = _io.load(), C.c_void_p()
    _io._chk(L.m6a_io_info_open(os.fsencode(d), min_reads, C.byref(h)))
    return h, L.m6a_io_info_get(h).contents


def host_rows(h, t, sites, norm):
    L = _io.load()
    idx = np.ascontiguousarray(sites, np.int64)
    reads = np.ctypeslib.as_array(C.cast(t.site_reads, C.POINTER(C.c_int64)), shape=(t.n_sites,))
    R = int(reads[idx].sum())
    X, ids, km, k7 = np.empty((R, 9), np.float32), np.empty(R), np.empty((len(idx), 3), np.uint8), C.create_string_buffer(7 * len(idx) + 1)
    blob, mean, std, n = _io.norm_arrays(norm)
    _io._chk(L.m6a_io_info_rows(h, idx.ctypes.data, len(idx), blob, None if mean is None else mean.ctypes.data,
                                None if std is None else std.ctypes.data, n, 2, X.ctypes.data, ids.ctypes.data, km.ctypes.data, k7))
    return X, ids, km, k7.raw[:7 * len(idx)]


def test_host_half_returns_the_loaders_rows_and_errors(tmp_path):
    rng = random.Random(5)
    good, valid, bad = generated_sites()
    ok = [s for s in good if s.tx != "ENST_E"] + valid
    JG.write_dir(str(tmp_path / "ok"), ok, junk=b"\n#junk#\n")
    for norm in (None, hct116()):
        ns = _io.NativeSites([str(tmp_path / "ok")], 1, norm, 2)
        h, t = info_table(str(tmp_path / "ok"), 1)
        try:
            assert t.n_sites == len(ok) and t.n_reads == int(ns.off[-1])
            names = C.string_at(t.tx_blob, np.ctypeslib.as_array(C.cast(t.tx_off, C.POINTER(C.c_int64)), shape=(t.n_tx + 1,))[-1])
            assert names == b"ENST_AENST_DV"
            pick = list(range(0, len(ok), 2))
            X, ids, km, k7 = host_rows(h, t, pick, norm)
            rows = np.concatenate([np.arange(ns.off[i], ns.off[i + 1]) for i in pick])
            assert X.view(np.uint32).tobytes() == np.ascontiguousarray(ns.X[rows]).view(np.uint32).tobytes()
            assert ids.tobytes() == np.ascontiguousarray(ns.read_id_values[rows]).tobytes()
            assert np.array_equal(km, ns.site_kmers[pick])
            assert [k7[7 * j + 1:7 * j + 6].decode() for j in range(len(pick))] == [ns.kmer5(i) for i in pick]
        finally:
            _io.load().m6a_io_info_free(h)
            ns.close()
    for name, s in JG.malformed(rng).items():                       # a valid site, the bad one, a second bad one
        d = str(tmp_path / ("bad_" + name.replace(" ", "_")))
        JG.write_dir(d, [valid[0], s, JG.malformed(rng, "ENST_LATER", 9)["not DRACH"]])
        with pytest.raises(_io.M6AIOError) as want:
            _io.NativeSites([d], 1, None, 2)
        h, t = info_table(d, 1)
        try:
            with pytest.raises(_io.M6AIOError) as got:
                host_rows(h, t, [0, 1, 2], None)
            assert (got.value.code, str(got.value)) == (want.value.code, str(want.value)), name
            host_rows(h, t, [0], None)                              # the site before it alone parses
        finally:
            _io.load().m6a_io_info_free(h)


# ---- the flag --------------------------------------------------------------------------------------------------------------------

def test_cli_parser_carries_loader_and_argparser_does_not():
    from m6anet_amd.scripts import inference
    flags = lambda p: {o for a in p._actions for o in a.option_strings}
    assert flags(inference.cli_parser()) - flags(inference.argparser()) == {"--loader"}
    a = inference.cli_parser().parse_args(["--input_dir", "x", "--out_dir", "y"])
    assert a.loader == "host"
    assert inference.cli_parser().parse_args(["--input_dir", "x", "--out_dir", "y", "--loader", "device"]).loader == "device"
    with pytest.raises(SystemExit):
        inference.cli_parser().parse_args(["--input_dir", "x", "--out_dir", "y", "--loader", "gpu"])


@pytest.mark.parametrize("extra,word", [(["--input_dir", "a", "b"], "one --input_dir"), (["--input_dir", "sites.m6astore"], "site store"),
                                        (["--input_dir", "a", "--gpus", "2"], "one GPU")])
def test_loader_device_refusals_come_before_anything_is_written(tmp_path, capsys, monkeypatch, extra, word):
    from m6anet_amd.scripts import inference
    monkeypatch.setenv("HSA_ENABLE_IPC_MODE_LEGACY", os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))     # maybe_start sets a default
    out = tmp_path / "out"
    args = inference.cli_parser().parse_args(extra + ["--out_dir", str(out), "--loader", "device"])
    with pytest.raises(SystemExit) as e:
        inference.main(args)
    assert e.value.code == 2 and word in capsys.readouterr().err
    assert not out.exists()
    from m6anet_amd import _early
    assert _early.state is None
    _early.maybe_start(["inference"] + extra + ["--out_dir", str(out), "--loader", "device", "--gpus", "2"])
    assert _early.state is None and not out.exists()                # no rank was started ahead of the refusal


def test_build_call_refuses_replicates_and_stores_without_a_device(tmp_path):
    for dirs, word in (([str(tmp_path / "a"), str(tmp_path / "b")], "one input directory"), ([str(tmp_path / "x.m6astore")], "site store")):
        with pytest.raises(ValueError) as e:
            _io.json_sites(dirs, 20, None)
        assert word in str(e.value) and "--loader host" in str(e.value)
