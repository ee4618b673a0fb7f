"""tests/dataprep_json_statement.py held to the reference's own files (tests/golden/ref_tests_data) and to the host writer; and the
argument errors of `dataprep --writer device`, which need no GPU."""
import json
import os
import subprocess
import sys

import pytest

import dataprep_json_statement as S
from m6anet_amd import _io
from test_dataprep_rows import GOLD, unpack

REF = os.path.join(GOLD, "ref_tests_data")
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def parse_json(path):
    """[(tx, pos, kmer7, features, reads)] of a data.json, in file order."""
    sites = []
    for line in open(path):
        (tx, by_pos), = json.loads(line).items()
        (pos, by_kmer), = by_pos.items()
        (kmer, reads), = by_kmer.items()
        sites.append((tx, int(pos), kmer, [r[:9] for r in reads], [int(r[9]) for r in reads]))
    return sites


def parse_index(path):
    rows = [l.split(",") for l in open(path).read().splitlines()[1:]]
    return [(t, int(r), int(a), int(b)) for t, r, a, b in rows]


def test_statement_is_the_references_files():
    sites = parse_json(os.path.join(REF, "data.json"))
    runs = parse_index(os.path.join(REF, "eventalign.index"))
    assert len(sites) == 248 and len(runs) > 100
    out = S.files(sites, runs, [])
    for name in ("data.json", "data.info", "eventalign.index"):
        assert out[name] == open(os.path.join(REF, name)).read(), name
    assert S.n_declined(sites) == 0 and sum(len(s[3]) for s in sites) * 10 == 70000


def test_statement_is_the_host_writer(tmp_path):
    ev = unpack(tmp_path, "ref_tests_data")
    plain, rounded = str(tmp_path / "plain"), str(tmp_path / "rounded")
    _io.dataprep(ev, plain, min_segment_count=1)
    _io.dataprep(ev, rounded, min_segment_count=1, compress=True)
    sites = parse_json(os.path.join(plain, "data.json"))
    runs = parse_index(os.path.join(plain, "eventalign.index"))
    logged = [l.split(":")[0] for l in open(os.path.join(plain, "data.log"))]
    assert logged and set(logged) >= {s[0] for s in sites}
    for d, round3 in ((plain, False), (rounded, True)):
        out = S.files(sites, runs, logged, round3)
        for name, text in out.items():
            assert text == open(os.path.join(d, name)).read(), (name, round3)
    assert S.log_line("t") == "t: Data preparation ... Done.\n"
    assert S.n_declined([("t", 1, "AAAAAAA", [[0.0004] * 9, [float("nan")] + [1.0] * 8], [3, 2 ** 53])], round3=True) == 9 + 1 + 1


@pytest.mark.parametrize("flags, named", [(["--device", "cpu"], "--device cpu"), (["--device", "gpu", "--skip_index"], "--skip_index"),
                                          (["--device", "gpu", "--n_neighbors", "2"], "--n_neighbors")])
def test_writer_device_argument_errors(tmp_path, flags, named):
    out = tmp_path / "out"
    r = subprocess.run([sys.executable, "-m", "m6anet_amd", "dataprep", "--eventalign", str(tmp_path / "missing.txt"), "--out_dir", str(out),
                        "--writer", "device"] + flags, cwd=REPO, timeout=300, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 2, (r.returncode, r.stderr[-2000:])
    assert "--writer device" in r.stderr and named in r.stderr and "conflicts with" in r.stderr, r.stderr
    assert not out.exists()                                           # before anything is touched
    with pytest.raises(ValueError, match=named):
        _io.dataprep(str(tmp_path / "missing.txt"), str(out), writer="device", device=flags[1], skip_index="--skip_index" in flags,
                     n_neighbors=2 if "--n_neighbors" in flags else 1)
    assert not out.exists()


def test_writer_host_is_the_default_and_unknown_writers_are_refused(tmp_path):
    r = subprocess.run([sys.executable, "-m", "m6anet_amd", "dataprep", "--eventalign", "x", "--out_dir", str(tmp_path / "o"), "--writer", "gpu"],
                       cwd=REPO, timeout=300, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 2 and "--writer" in r.stderr
    with pytest.raises(ValueError, match="writer"):
        _io.dataprep("x", str(tmp_path / "o"), writer="gpu")
    ev = unpack(tmp_path, "ref_tests_data")
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    _io.dataprep(ev, a, min_segment_count=20)
    _io.dataprep(ev, b, min_segment_count=20, writer="host")
    for name in ("eventalign.index", "data.json", "data.info", "data.log"):
        assert open(os.path.join(a, name), "rb").read() == open(os.path.join(b, name), "rb").read()
