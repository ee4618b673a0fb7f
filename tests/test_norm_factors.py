"""compute_norm_factors without a GPU: the statement (tests/norm_statement.py) against what the reference returned and against np.sum,
the summation core (m6anet_amd/csrc/m6a_norm.h) as tests/norm_core_main.cpp, a program of its own built here with ASan and UBSan,
the host route of libm6a_io.so against the statement on the golden directory and every generated family (tests/norm_gen.py), and
the command with --device cpu.  tests/test_gpu_norm_factors.py holds the kernels to the same statement and the same host route."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import norm_gen as NG
import norm_statement as NS
from m6anet_amd import _io
from m6anet_amd.data_utils import compute_norm_factors, load_norm_factors, read_norm_sites

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
GOLD = os.path.join(HERE, "golden")
LENGTHS = list(range(1100)) + [4095, 4096, 4097, 8191, 8192, 8193, 12000, 16384, 20000, 100003]


def same_bits(a, b):
    """equal as bits; NaN equals NaN whatever its payload"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and np.array_equal(a[~nan].view(np.uint64), b[~nan].view(np.uint64))


def golden_dir(path):
    os.makedirs(path, exist_ok=True)
    shutil.copy(os.path.join(GOLD, "ref_tests_data", "data.json"), path)
    shutil.copy(os.path.join(GOLD, "norm_ref", "data.info.labelled"), path)
    return str(path)


def route(path, device="cpu", n_threads=3):
    tx, pos, start, end, n_reads = read_norm_sites(path)
    return _io.norm_factors(os.path.join(path, "data.json"), tx, pos, start, end, n_reads, device=device, n_threads=n_threads)


def assert_route_is_statement(r, want, what):
    """want: norm_statement.sums() -- the 5-mers and their order, N, S, S2 and the finished factors"""
    assert r["kmers"] == list(want), what
    assert [int(n) for n in r["N"]] == [want[k][0] for k in want], what
    for j, name in ((1, "S"), (2, "S2")):
        assert same_bits(r[name], [want[k][j] for k in want]), (what, name)
    fin = [[NS.finish(S[j], S2[j], N) for j in range(3)] for N, S, S2 in want.values()]
    assert same_bits(r["mean"], [[m for m, _ in f] for f in fin]), (what, "mean")
    assert same_bits(r["std"], [[d for _, d in f] for f in fin]), (what, "std")


@pytest.fixture(scope="module")
def columns():
    """one column of 100 003 values and the statement's two sums of its every prefix in LENGTHS"""
    x = np.random.default_rng(1).normal(100.0, 30.0, (100003, 9))
    col = [float(v) for v in x[:, 4]]
    sq = [v * v for v in col]
    return x, {n: (NS.colsum(col[:n]), NS.colsum(sq[:n])) for n in LENGTHS}


@pytest.fixture(scope="module")
def families(tmp_path_factory):
    root = tmp_path_factory.mktemp("norm_families")
    out = {"golden": (golden_dir(root / "golden"), None)}
    for name, make in NG.FAMILIES.items():
        d = make(str(root / name.replace(" ", "_")))
        out[name] = (d.path, d)
    return {name: (path, d, NS.sums(path)) for name, (path, d) in out.items()}


def test_statement_equals_what_the_reference_returned(families):
    with np.load(os.path.join(GOLD, "norm_ref", "norm_factors.npz")) as z:
        kmers, mean, std = [str(k) for k in z["kmers"]], z["mean"], z["std"]
    got = NS.norm_factors(families["golden"][0])
    assert list(got) == kmers and len(kmers) == 9 and len(NS.train_rows(families["golden"][0])) == 133
    assert same_bits([got[k][0] for k in kmers], mean) and same_bits([got[k][1] for k in kmers], std)
    assert not np.isnan(mean).any() and not np.isnan(std).any()


def test_statements_colsum_is_np_sum_of_the_reference_slice(columns):
    x, want = columns
    idx = np.arange(3, 6)                                      # features[:, indices] of the reference: a Fortran-contiguous copy
    for n in LENGTHS:
        sig = x[:n][:, idx]
        assert (float(np.sum(sig, axis=0)[1]), float(np.sum(np.square(sig), axis=0)[1])) == want[n], n
    # the pieces matter: one pairwise sum over the whole column differs from 8 193 elements on
    col = [float(v) for v in x[:8193, 4]]
    assert NS.pw(col, 0, 8192) == want[8192][0] and any(NS.pw([float(v) for v in x[:n, 4]], 0, n) != want[n][0] for n in (8193, 12000, 20000))


def test_core_under_sanitizers_is_the_statement(columns, tmp_path):
    x, want = columns
    exe = str(tmp_path / "norm_core")
    subprocess.run(["g++", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g", "-O1", "-std=c++17",
                    "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(REPO, "m6anet_amd", "csrc"),
                    os.path.join(HERE, "norm_core_main.cpp"), "-o", exe], check=True, timeout=300)
    np.ascontiguousarray(x[:, 4]).tofile(str(tmp_path / "doubles.bin"))
    np.array(LENGTHS, np.int64).tofile(str(tmp_path / "lengths.bin"))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, str(tmp_path / "doubles.bin"), str(tmp_path / "lengths.bin")], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stdout[-300:], r.stderr[-3000:])
    lines = r.stdout.splitlines()
    assert len(lines) == len(LENGTHS)
    for n, line in zip(LENGTHS, lines):
        f = line.split("\t")
        got = np.array([int(h, 16) for h in f[1:]], np.uint64).view(np.float64)
        assert int(f[0]) == n and same_bits(got[:2], want[n]), n
        if n:
            assert same_bits(got[2:], NS.finish(want[n][0], want[n][1], n)), n


def test_generated_families_hold_what_they_say(families):
    path, d, want = families["sizes"]
    train = d.train
    assert {s.n_reads for s in train} >= set(NG.READS)
    assert {st for _, st in d.rows} == set(NG.SETS) and [i for i, st in d.rows if st == "Train"].count(3) == 2
    assert [i for i, _ in d.rows] != sorted(i for i, _ in d.rows)                      # not the file's order
    assert {"AAAAA", NG.OUTSIDE[:5], NG.SINGLE[:5]} <= set(want)
    assert want["AAAAA"][0] == 3 * sum(s.n_reads for s in train if b'"AAAAAAA"' in s.text)        # one site, three entries of one 5-mer
    assert want[NG.SINGLE[:5]][0] == 1 and sum(s.text.count(b"AAGACTT") for s in train) > 200
    assert d.n_declined() == 0
    assert families["declined"][1].n_declined() == 5 and families["declined twin"][1].n_declined() == 0
    assert families["nonfinite"][1].n_declined() == 3
    for name, (_, _, w) in families.items():
        cols = np.array([w[k][1] + w[k][2] for k in w])
        assert not (cols == 0).any(), name                                             # no all-zero column: the sign of a zero sum is not pinned
        assert np.isnan(cols).any() == (name == "nonfinite"), name


def test_host_route_is_the_statement(families):
    for name, (path, _, want) in families.items():
        for n_threads in (1, 5):
            assert_route_is_statement(route(path, n_threads=n_threads), want, name)
    # a declined site gives what its all-regular twin gives
    a, b = families["declined"][2], families["declined twin"][2]
    assert list(a) == list(b) and all(a[k][0] == b[k][0] and same_bits(a[k][1:], b[k][1:]) for k in a)


def test_host_partials_are_the_statements(families):
    path, d, _ = families["sizes"]
    tx, pos, start, end, n_reads = read_norm_sites(path)
    with open(os.path.join(path, "data.json"), "rb") as f:
        blob = f.read()
    sites = list(range(0, len(tx), 7))
    s, s2, k7 = _io.norm_partials(os.path.join(path, "data.json"), tx, pos, start, end, n_reads, sites=sites, n_threads=2)
    for k, i in enumerate(sites):
        kmer, w, w2 = NS.site_partials(blob, tx[i], int(pos[i]), int(start[i]), int(end[i]), int(n_reads[i]))
        assert k7[k] == kmer and same_bits(s[k], w) and same_bits(s2[k], w2), i
    with pytest.raises(_io.M6AIOError, match="not ascending"):
        _io.norm_partials(os.path.join(path, "data.json"), tx, pos, start, end, n_reads, sites=[3, 3])


def test_compute_norm_factors_returns_load_norm_factors_dict(families):
    path, _, want = families["golden"]
    d = compute_norm_factors(path, device="cpu", n_threads=2)
    with np.load(os.path.join(GOLD, "norm_ref", "norm_factors.npz")) as z:
        assert list(d) == [str(k) for k in z["kmers"]]
        assert same_bits([d[k][0] for k in d], z["mean"]) and same_bits([d[k][1] for k in d], z["std"])


@pytest.mark.parametrize("name", sorted(NG.MALFORMED_TEXT))
def test_malformed_site_is_the_loaders_error(name, tmp_path):
    d = NG.malformed(str(tmp_path / "d"), name)
    with pytest.raises(_io.M6AIOError) as e:
        route(d.path)
    assert e.value.code == -4 and NG.MALFORMED_TEXT[name] in str(e.value) and "ENST_LATER" not in str(e.value), str(e.value)
    if "reads" in name:                                          # the count mismatch: the statement's own text
        with pytest.raises(NS.CountMismatch) as s:
            NS.sums(d.path)
        assert str(e.value).endswith(str(s.value)) and "data.info.labelled" in str(e.value)


def test_range_outside_the_file_is_the_loaders_error(tmp_path):
    d = NG.out_of_range(str(tmp_path / "d"))
    with pytest.raises(_io.M6AIOError, match="site ENST_R:2: byte range outside data.json") as e:
        route(d.path)
    assert e.value.code == -4


def run_cli(*argv, env=None):
    return subprocess.run([sys.executable, "-m", "m6anet_amd", "compute_norm_factors"] + [str(a) for a in argv], cwd=REPO, capture_output=True,
                          text=True, timeout=300, env=dict(os.environ, **(env or {})))


def test_cli_on_the_host_writes_both_files(families, tmp_path):
    import json
    path, _, want = families["golden"]
    out = tmp_path / "out"
    r = run_cli("--input_dir", path, "--out_dir", out, "--device", "cpu", "--n_processes", 2, env={"M6A_NORM_TIMES": "1"})
    assert r.returncode == 0, r.stderr[-2000:]
    import joblib  # noqa: F401  (the reference's format: written only where joblib imports, as it does here)
    assert sorted(os.listdir(out)) == ["norm_dict_nanopolish.joblib", "norm_dict_nanopolish.npz"]
    a, b = (load_norm_factors(str(out / ("norm_dict_nanopolish" + ext))) for ext in (".npz", ".joblib"))
    with np.load(os.path.join(GOLD, "norm_ref", "norm_factors.npz")) as z:
        kmers, mean, std = [str(k) for k in z["kmers"]], z["mean"], z["std"]
    for d in (a, b):
        assert list(d) == kmers and same_bits([d[k][0] for k in kmers], mean) and same_bits([d[k][1] for k in kmers], std)
    times = [json.loads(l[len("M6A_TIMES "):]) for l in r.stderr.splitlines() if l.startswith("M6A_TIMES ")]
    assert len(times) == 1 and times[0]["n_sites"] == 133 and times[0]["n_kmers"] == 9 and times[0]["n_reads"] == sum(w[0] for w in want.values()) // 3
    assert times[0]["device"] == "cpu" and times[0]["d2h_bytes"] == 0 and times[0]["peak_device_bytes"] == 0
    assert "--input_dir" in run_cli("--help").stdout


def test_every_refusal_is_exit_status_2_before_anything_is_written(families, tmp_path, capsys):
    from m6anet_amd.__main__ import main
    good = families["golden"][0]
    lines = open(os.path.join(good, "data.info.labelled")).read().splitlines()
    header = lines[0].split(",")
    first_train = next(i for i, l in enumerate(lines) if l.endswith(",Train"))

    def variant(name, labelled=None, json_file=True):
        d = tmp_path / name
        os.makedirs(d)
        if json_file:
            shutil.copy(os.path.join(good, "data.json"), d)
        if labelled is not None:
            (d / "data.info.labelled").write_text("\n".join(labelled) + "\n")
        return d

    def edit(col, value):
        f = lines[first_train].split(",")
        f[header.index(col)] = value
        return lines[:first_train] + [",".join(f)] + lines[first_train + 1:]

    drop = header.index("start")
    cases = [
        (variant("no_labelled"), "data.info.labelled: no such file"),
        (variant("no_json", lines, json_file=False), "data.json: no such file"),
        (variant("no_column", [",".join(f for i, f in enumerate(l.split(",")) if i != drop) for l in lines]), "missing column(s) ['start']"),
        (variant("no_set_type", [l.rsplit(",", 1)[0] for l in lines]), "missing column(s) ['set_type']"),
        (variant("no_train", [l for l in lines if not l.endswith(",Train")]), "no row with set_type Train"),
        (variant("bad_reads", edit("n_reads", "12x")), "line %d: transcript_position, start, end and n_reads must be integers" % (first_train + 1)),
        (variant("bad_position", edit("transcript_position", "130.5")), "line %d: transcript_position" % (first_train + 1)),
        (variant("bad_range", edit("start", lines[first_train].split(",")[header.index("end")])), "are no byte range"),
    ]
    for k, (d, word) in enumerate(cases):
        out = tmp_path / ("out%d" % k)
        with pytest.raises(SystemExit) as e:
            main(["compute_norm_factors", "--input_dir", str(d), "--out_dir", str(out), "--device", "cpu" if k % 2 else "gpu"])
        err = capsys.readouterr().err
        assert e.value.code == 2 and word in err, (d, e.value.code, err[-500:])
        assert not out.exists(), d
    r = run_cli("--input_dir", cases[4][0], "--out_dir", tmp_path / "out_sub")              # and once as the command itself, on the default device
    assert r.returncode == 2 and "no row with set_type Train" in r.stderr and "Traceback" not in r.stderr and not (tmp_path / "out_sub").exists()


def test_integer_valued_decimal_positions_are_taken(families):
    path, d, _ = families["sizes"]
    text = open(os.path.join(path, "data.info.labelled")).read()
    assert ".0," in text and sorted(int(p) for p in read_norm_sites(path)[1]) == sorted(s.pos for s in d.train)
