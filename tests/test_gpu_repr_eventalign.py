"""`eventalign_inference --read_representation`, --representation_dtype and what they stand on (include/m6a.h:
m6a_prep_sites_write_read_representation, m6a_read_representation_dtype; enc_repr_kernel<true> in m6anet_amd/csrc/m6a_kernels.hip).

1. twins     data.read_representation.npy and both CSVs of the fused command are the bytes of `dataprep` + `inference
             --read_representation` on the same text: every n_neighbors = 1 fixture of tests/test_dataprep_rows.py, generated families of
             tests/eventalign_gen.py, and one case per mode of the command
2. rounds    M6A_REPR_ROUND_KB from one site per round to everything in one: the same bytes, and the count the statement gives
3. float16   exactly the float32 result's .astype(np.float16), compared as uint16, at the kernel's edges and the conversion's
4. float32   m6a_read_representation_dtype(M6A_REPR_F32) is m6a_read_representation, bit for bit
5. refusals  each followed by one correct call
6. traffic   d2h_bytes rises by exactly the rows' bytes

The commands run in this process through the package's dispatcher (m6anet_amd.__main__.main: the command's own parser and main), so
a case costs no interpreter start and no second GPU context."""
import contextlib
import io
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import eventalign_gen as G                            # noqa: E402
import read_names_gen as NG                           # noqa: E402
import replicate_fixtures as F                        # noqa: E402
import repr_file_statement as stmt                    # noqa: E402
from m6anet_amd import _io, _lib                      # noqa: E402
from test_dataprep_rows import cases, unpack          # noqa: E402
from test_gpu_read_representation import EDGE_BAGS, rand_sites, to_device          # noqa: E402

CSVS = ("data.site_proba.csv", "data.indiv_proba.csv")
NPY = "data.read_representation.npy"
QUICK = ["--num_iterations", "50", "--n_processes", "2"]
SENTINEL16 = np.uint16(0xBEEF)                        # a negative binary16: no relu output is one
SENTINEL32 = np.float32(-12345.678)


@contextlib.contextmanager
def environ(**kw):
    old = {k: os.environ.get(k) for k in kw}
    os.environ.update({k: str(v) for k, v in kw.items()})
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def cmd(argv, **env):
    """One command through the dispatcher; returns its M6A_TIMES (eventalign_inference) or None."""
    from m6anet_amd.__main__ import main
    out = io.StringIO()
    with environ(M6A_EVENTALIGN_TIMES="1", **env), contextlib.redirect_stdout(out):
        main([str(a) for a in argv])
    lines = [l for l in out.getvalue().splitlines() if l.startswith("M6A_TIMES ")]
    return json.loads(lines[0][len("M6A_TIMES "):]) if lines else None


def read(d, fn):
    with open(os.path.join(str(d), fn), "rb") as f:
        return f.read()


def site_flags(kw):
    return ["--%s=%d" % (k, v) for k, v in kw.items() if k in ("readcount_min", "readcount_max", "min_segment_count")]


def two_step(tmp, files, flags=(), dtype=None):
    """K `dataprep`s and one `inference --read_representation`; returns the out_dir, or the loader's error when no site is kept"""
    files = [files] if isinstance(files, str) else list(files)
    site = [f for f in flags if f.split("=")[0] in ("--readcount_min", "--readcount_max", "--min_segment_count")]
    dirs = []
    for k, ev in enumerate(files):
        dirs.append(str(tmp / ("prep%d" % k)))
        cmd(["dataprep", "--eventalign", ev, "--out_dir", dirs[-1], "--n_processes", "2"] + site)
    out = str(tmp / "two")
    try:
        cmd(["inference", "--input_dir"] + dirs + ["--out_dir", out, "--read_representation"] + [f for f in flags if f not in site] +
            (["--representation_dtype", dtype] if dtype else []))
    except _io.M6AIOError as e:
        return out, e
    return out, None


def fused(tmp, files, flags=(), tag="fused", dtype=None, **env):
    files = [files] if isinstance(files, str) else list(files)
    out = str(tmp / tag)
    t = cmd(["eventalign_inference", "--eventalign"] + files + ["--out_dir", out, "--read_representation"] + list(flags) +
            (["--representation_dtype", dtype] if dtype else []), **env)
    return out, t


def same_three(a, b, tag):
    for fn in CSVS + (NPY,):
        assert read(a, fn) == read(b, fn), (tag, fn)
    rows = read(a, CSVS[1]).count(b"\n") - 1
    arr = np.load(os.path.join(a, NPY), mmap_mode="r")
    assert arr.shape == (rows, 32) and arr.dtype == np.float32 and rows > 0, tag
    return rows


# ---- 1. twins --------------------------------------------------------------------------------------------------------------------------
def fixture_files(tmp_path):
    out = [(name, ev, site_flags(kw)) for name, ev, kw in cases(tmp_path) if kw.get("n_neighbors", 1) == 1 and not kw.get("compress")]
    out.append(("ref_default", unpack(tmp_path, "ref_tests_data"), []))
    for family in ("plain", "combine", "filters_20", "declined"):
        c = G.case(family, 1)
        out.append(("gen_" + family, c.write(tmp_path)[0], site_flags(c.kw)))
    return out


FIXTURE_NAMES = ["ref_msc1", "synthetic_nn1", "noncontiguous", "header_only", "nonl", "crlf", "crafted", "crafted_rc3", "ref_default", "gen_plain", "gen_combine",
                 "gen_filters_20", "gen_declined"]


@pytest.mark.parametrize("name", FIXTURE_NAMES)
def test_fixture_twins(tmp_path, name):
    (ev, flags), = [(e, f) for n, e, f in fixture_files(tmp_path) if n == name]
    flags = flags + QUICK
    two, err = two_step(tmp_path, ev, flags)
    if err is not None:                                              # no site reaches 20 reads: both fail alike, and no .npy is left
        assert "no site with at least" in str(err), name
        with pytest.raises(_io.M6AIOError) as e:
            fused(tmp_path, ev, flags)
        assert "no site with at least" in str(e.value)
        assert not os.path.exists(os.path.join(str(tmp_path / "fused"), NPY))
        assert name in ("header_only", "crafted_rc3"), name          # the fixtures known to keep nothing
        return
    out, t = fused(tmp_path, ev, flags)
    rows = same_three(two, out, name)
    assert t["repr_rounds"] == 1 and t["repr_bytes"] == 128 + 128 * rows == os.path.getsize(os.path.join(out, NPY))


def test_fixture_names_are_the_fixtures(tmp_path):
    assert sorted(n for n, _, _ in fixture_files(tmp_path)) == sorted(FIXTURE_NAMES)


@pytest.fixture(scope="module")
def bundled(tmp_path_factory):
    """the bundled file, and its two-step outputs per flag set, made once"""
    root = tmp_path_factory.mktemp("bundled")
    ev = unpack(root, "ref_tests_data")
    made = {}

    def twin(flags=()):
        key = tuple(flags)
        if key not in made:
            d = root / ("twin%d" % len(made))
            d.mkdir()
            out, err = two_step(d, ev, list(flags) + QUICK)
            assert err is None
            made[key] = out
        return made[key]
    return ev, twin


TAIL = ["--drop_unflushed_tail", "--batch_size", "8", "--save_per_batch", "13", "--seed", "5"]     # 101 sites, 13 batches: the last one is dropped


@pytest.mark.parametrize("mode", ["plain", "windows", "bgzf", "fifo", "csv_device", "tail", "tail_csv_device", "site_proba", "compress"])
def test_mode_twins(tmp_path, bundled, mode):
    ev, twin = bundled
    flags, env, files, feed = [], {}, ev, None
    if mode == "windows":
        env = dict(M6A_PREP_WINDOW_KB="8")
    elif mode == "bgzf":
        cmd(["bgzip", ev])                                           # FILE.gz beside FILE, which stays
        files = ev + ".gz"
    elif mode == "fifo":
        from test_gpu_pipe_input import Feed
        feed = Feed(tmp_path, open(ev, "rb").read(), 1 << 16)
        files = feed.path
    elif mode == "csv_device":
        flags = ["--csv", "device"]
    elif mode == "tail":
        flags = TAIL
    elif mode == "tail_csv_device":
        flags = TAIL + ["--csv", "device"]
    elif mode == "site_proba":
        flags = ["--site_proba", "expected"]
    elif mode == "compress":
        flags = ["--compress", "--csv", "device"]
    base = [f for f in flags if f not in ("--csv", "device", "--compress")]
    want = twin(base)
    try:
        out, t = fused(tmp_path, files, flags + QUICK, **env)
    finally:
        if feed is not None:
            feed.done()
    if mode == "compress":                                           # the CSVs are BGZF; the .npy is not compressed
        import gzip
        for fn in CSVS:
            assert gzip.decompress(read(out, fn + ".gz")) == read(want, fn) and not os.path.exists(os.path.join(out, fn))
        assert read(out, NPY) == read(want, NPY)
        return
    rows = same_three(want, out, mode)
    if mode == "windows":
        assert t["n_windows"] > 1
    if mode == "bgzf":
        assert t["n_bgzf_blocks"] > 0
    if mode == "fifo":
        assert t["n_streams"] == 1
    if mode.endswith("csv_device"):
        assert t["csv_writer"] == "device"
    if mode.startswith("tail"):                                      # the tail is dropped from all three files alike
        assert rows < np.load(os.path.join(twin(()), NPY), mmap_mode="r").shape[0]


def test_read_names_against_its_twin(tmp_path):
    c = NG.case("again")
    named, twin = c.write(tmp_path)
    a, _ = fused(tmp_path, twin, QUICK, tag="twin")
    b, t = fused(tmp_path, named, QUICK + ["--read_names"], tag="named")
    assert read(a, NPY) == read(b, NPY) and read(a, CSVS[0]) == read(b, CSVS[0])
    assert t["n_read_names"] > 0 and np.load(os.path.join(b, NPY)).shape[0] == read(b, CSVS[1]).count(b"\n") - 1 > 0


def test_three_replicates_against_three_dataprep_and_one_inference(tmp_path):
    files = F.write(tmp_path, "three")
    flags = ["--min_segment_count=1"] + QUICK
    two, err = two_step(tmp_path, files, flags)
    assert err is None
    out, t = fused(tmp_path, files, flags)
    same_three(two, out, "three")
    assert t["n_replicates"] == 3


# ---- 2. round edges --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def round_file(tmp_path_factory):
    """sites of 20..40 reads and one of 300: with 2 KB rounds (16 float32 rows) every site is a round of its own and larger than a
    round; with 5 KB (40 rows) most rounds hold one site, the 300-read site is larger than its round, and the last round is whatever
    is left; the default holds everything in one."""
    root = tmp_path_factory.mktemp("rounds")
    rng = np.random.default_rng(7)
    f = G.File(rng)
    tx = G.Tx(rng, "ROUND", 60, (4, 11, 19, 30, 41, 52))
    for centre, n in zip((4, 11, 19, 30, 41, 52), (20, 25, 300, 21, 40, 23)):
        G.site_reads(f, tx, centre, range(1000 * centre, 1000 * centre + n), mismatch=0)
    ev = root / "rounds.txt"
    ev.write_bytes(f.bytes())
    return str(ev), root


@pytest.mark.parametrize("dtype", ["float32", "float16"])
def test_round_edges(round_file, tmp_path, dtype):
    ev, _ = round_file
    base, t0 = fused(tmp_path, ev, QUICK, tag="default", dtype=dtype)
    want = read(base, NPY)
    with _io.prep_sites(ev, n_threads=2) as p:
        off, S = [int(x) for x in p.off], p.n_sites
    n = [b - a for a, b in zip(off, off[1:])]
    assert S >= 5 and max(n) == 300 and off[-1] * 32 * stmt.ITEMSIZE[dtype] + 128 == len(want)
    assert t0["repr_rounds"] == stmt.n_rounds(off, S, stmt.DEFAULT_ROUND_KB, dtype) == 1
    seen = set()
    for kb in (1, 2, 5, 8, 40, 1 << 10):
        out, t = fused(tmp_path, ev, QUICK, tag="kb%d" % kb, dtype=dtype, M6A_REPR_ROUND_KB=kb)
        assert read(out, NPY) == want, kb
        cut = stmt.cut_rounds(off, S, kb, dtype)
        assert t["repr_rounds"] == len(cut) - 1 == stmt.n_rounds(off, S, kb, dtype), (kb, t["repr_rounds"], cut)
        assert t["repr_bytes"] == len(want)
        seen.add(len(cut) - 1)
    per = 1024 // (32 * stmt.ITEMSIZE[dtype])
    assert stmt.cut_rounds(off, S, 1, dtype) == list(range(S + 1)) and min(n) > per          # a round holds one site, each larger than it
    mid = stmt.cut_rounds(off, S, 8, dtype)
    assert 1 < len(mid) - 1 < S                                      # rounds of several sites, the 300-read site alone, a partial last one
    assert 1 in seen and S in seen and len(seen) >= 3


def test_round_limit_matches_the_csv_rows(round_file, tmp_path):
    """--drop_unflushed_tail with rounds smaller than a site: the rows are the CSV's"""
    ev, _ = round_file
    flags = ["--drop_unflushed_tail", "--batch_size", "2", "--save_per_batch", "3"] + QUICK       # 6 sites, 3 batches: the last one is dropped
    out, t = fused(tmp_path, ev, flags, M6A_REPR_ROUND_KB=2)
    rows = read(out, CSVS[1]).count(b"\n") - 1
    a = np.load(os.path.join(out, NPY))
    whole, _ = fused(tmp_path, ev, QUICK, tag="whole")
    b = np.load(os.path.join(whole, NPY))
    assert 0 < rows == a.shape[0] < b.shape[0] and np.array_equal(a.view(np.uint32), b[:rows].view(np.uint32))


# ---- 3. float16, exact -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def eng(weights):
    from m6anet_amd.engine import M6ANetEngine
    e = M6ANetEngine(weights=weights["hct116"])
    yield e
    e.close()


def both_types(e, X, km, off):
    """(float32 repr, its read_prob, float16 repr as uint16 with its sentinel rows checked, its read_prob), device pointers"""
    import torch
    R, pad = X.shape[0], 64
    t = to_device(X, km, off)
    h32, p32 = e.get_read_representation(*t, want_read_probs=True)
    big = torch.from_numpy(np.full((R + 2 * pad, 32), SENTINEL16, np.uint16).view(np.float16)).to("cuda:0")
    big_p = torch.full((R + 2 * pad,), float(SENTINEL32), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    out = e.get_read_representation(*t, out=(big[pad:pad + R], big_p[pad:pad + R]), want_read_probs=True, dtype="float16")
    e.sync()
    assert out[0].dtype == torch.float16 and out[0].data_ptr() == big[pad:].data_ptr()
    got = big.cpu().numpy().view(np.uint16)
    got_p = big_p.cpu().numpy()
    assert np.all(got[:pad] == SENTINEL16) and np.all(got[pad + R:] == SENTINEL16)
    assert np.all(got_p[:pad] == SENTINEL32) and np.all(got_p[pad + R:] == SENTINEL32)
    return h32.cpu().numpy(), p32.cpu().numpy(), got[pad:pad + R], got_p[pad:pad + R]


def as_f16_bits(h32):
    with np.errstate(over="ignore"):
        return np.ascontiguousarray(h32, np.float32).astype(np.float16).view(np.uint16)


@pytest.mark.parametrize("case", [c for c in EDGE_BAGS if c != "empty_sites"] + ["empty_sites"])
def test_f16_is_the_f32_result_cast_by_numpy(eng, case):
    X, km, off = rand_sites(sorted(EDGE_BAGS).index(case), EDGE_BAGS[case])
    h32, p32, h16, p16 = both_types(eng, X, km, off)
    assert h16.shape == h32.shape and np.array_equal(h16, as_f16_bits(h32)), case
    assert np.array_equal(p16.view(np.uint32), p32.view(np.uint32)), case
    assert eng.last_encoder_kernel == "enc_repr_kernel<true>"


def test_f16_kmer_ids_0_and_65_and_a_nan_row(eng):
    X, km, off = rand_sites(5, [20] * 6)
    km = np.array([[0, 65, 0], [65, 65, 65], [0, 0, 0], [65, 0, 1], [64, 65, 0], [0, 1, 65]], np.uint8)
    X[33, 4] = np.nan
    h32, p32, h16, p16 = both_types(eng, X, km, off)
    assert np.isnan(h32[33]).any() and not np.isnan(np.delete(h32, 33, 0)).any()
    assert np.array_equal(h16, as_f16_bits(h32))                     # a NaN stays a NaN, sign and the payload's top bits as NumPy keeps them
    assert np.array_equal(np.isnan(h16.view(np.float16)), np.isnan(h32))
    assert np.array_equal(p16.view(np.uint32), p32.view(np.uint32))


def test_f16_host_pointers_and_numpy_arrays(eng):
    X, km, off = rand_sites(8, [20] * 50 + [3, 1, 500])
    h32 = eng.get_read_representation(X, km, off)
    out = np.full((X.shape[0], 32), SENTINEL16, np.uint16).view(np.float16)
    h16, p = eng.get_read_representation(X, km, off, out=out, want_read_probs=True, dtype="float16")
    assert h16 is out and h16.dtype == np.float16 and np.array_equal(h16.view(np.uint16), as_f16_bits(h32))
    assert np.array_equal(p.view(np.uint32), eng.get_read_probability(X, km, off).view(np.uint32))
    with pytest.raises(TypeError):
        eng.get_read_representation(X, km, off, out=np.empty((X.shape[0], 32), np.float32), dtype="float16")
    with pytest.raises(ValueError):
        eng.get_read_representation(X, km, off, dtype="bfloat16")


# the conversion's edges, as float32 values of b2 (layer 2's bias): with W2 = 0 every row of the representation is relu(b2)
EDGES = [0.0, 2.0 ** -24, 2.0 ** -25, 1.5 * 2.0 ** -24, 1023 * 2.0 ** -24, 2.0 ** -14, 65504.0, 65519.996, 65520.0, 1 + 2.0 ** -11,
         1 + 2.0 ** -11 + 2.0 ** -23,
         # and around them: just above the tie at 2^-25, ties to even above it, the tie below 2^-14, ties among normals, a tie below
         # 65504, a float32 subnormal, the smallest float32 normal, values that need no rounding, a large finite value
         2.0 ** -25 * (1 + 2.0 ** -23), 2.5 * 2.0 ** -24, 3.5 * 2.0 ** -24, 2.0 ** -14 - 2.0 ** -25, 1 + 3 * 2.0 ** -11, 2049.0, 2051.0,
         65488.0, 65504.004, 1e-40, 2.0 ** -126, 1e-8, 6e-8, 0.1, 1.0 / 3, 1000.5, 1.0, 1e18, 2.0 ** -15, 3 * 2.0 ** -24]
BIG_UNIT = 31                                         # this unit gets 1e30 (below)


def edge_weights(weights):
    """W1 = b1 = 0 and gamma = 0, so that batch norm gives bn_beta whatever X is; W2 = 0 but for one entry; b2 = EDGES.
    m6a_create refuses a layer-2 weight or bias of 2^63 or more (the kernels carry them scaled by 2^64), so b2 cannot hold 1e30:
    unit BIG_UNIT gets it as the one product W2[BIG_UNIT][0] * relu(bn_beta[0]) = 1e15 * 1e15 in float32, with b2 = 0."""
    w = np.array(weights["hct116"], np.float32)
    o_w1 = 132
    o_b1 = o_w1 + 150 * 15
    o_g, o_be, o_mu, o_var = o_b1 + 150, o_b1 + 300, o_b1 + 450, o_b1 + 600
    o_w2 = o_var + 150
    o_b2 = o_w2 + 32 * 150
    o_w3 = o_b2 + 32
    assert o_w3 + 33 == w.size == 7997
    w[o_w1:o_g] = 0
    w[o_g:o_g + 150] = 0
    w[o_be:o_be + 150] = 0
    w[o_mu:o_mu + 150] = 0
    w[o_var:o_var + 150] = 1
    w[o_w2:o_b2] = 0
    b2 = np.array(EDGES + [0.0] * (32 - len(EDGES)), np.float32)
    assert len(EDGES) == BIG_UNIT and b2.size == 32
    w[o_b2:o_w3] = b2
    w[o_be] = 1e15
    w[o_w2 + 150 * BIG_UNIT] = 1e15
    w[o_w3:o_w3 + 32] = 0
    want = b2.copy()
    want[BIG_UNIT] = np.float32(1e15) * np.float32(1e15)
    return w, want


def test_f16_conversion_edges(weights):
    from m6anet_amd.engine import M6ANetEngine
    w, want = edge_weights(weights)
    assert want[BIG_UNIT] > 9e29 and np.isfinite(want[BIG_UNIT])
    X, km, off = rand_sites(3, [20, 13])
    e = M6ANetEngine(weights=w)
    try:
        h32, p32, h16, p16 = both_types(e, X, km, off)
    finally:
        e.close()
    assert np.array_equal(h32.view(np.uint32), np.tile(want.view(np.uint32), (33, 1)))          # every row is the chosen values
    got = h16[0].view(np.float16)
    for v, g in zip(want, got):                                      # each one by name, then all of them as bits
        with np.errstate(over="ignore"):
            assert np.float32(v).astype(np.float16).view(np.uint16) == g.view(np.uint16), (float(v), float(g))
    assert np.array_equal(h16, np.tile(as_f16_bits(want), (33, 1)))
    f = lambda x: np.float16(x).view(np.uint16)                     # noqa: E731  -- what the ties and the range edges must come to
    assert got[2].view(np.uint16) == 0 and got[1].view(np.uint16) == 1 and got[3].view(np.uint16) == 2       # 2^-25 -> 0, 1.5 * 2^-24 -> even
    assert got[4].view(np.uint16) == 0x03FF and got[5].view(np.uint16) == 0x0400 and got[6].view(np.uint16) == 0x7BFF
    assert got[7].view(np.uint16) == 0x7BFF and got[8].view(np.uint16) == 0x7C00 and got[BIG_UNIT].view(np.uint16) == 0x7C00
    assert got[9].view(np.uint16) == f(1.0) and got[10].view(np.uint16) == f(1.0) + 1 and got[11].view(np.uint16) == 1
    assert got[20].view(np.uint16) == 0 and got[21].view(np.uint16) == 0


def test_f16_file_is_the_f32_file_cast_by_numpy(bundled, tmp_path):
    ev, twin = bundled
    a, ta = fused(tmp_path, ev, QUICK, tag="f32")
    b, tb = fused(tmp_path, ev, QUICK, tag="f16", dtype="float16")
    assert read(a, NPY) == read(twin(()), NPY)
    for fn in CSVS:
        assert read(a, fn) == read(b, fn)
    want = str(tmp_path / "cast.npy")
    h32 = np.load(os.path.join(a, NPY))
    m = np.lib.format.open_memmap(want, mode="w+", dtype=np.float16, shape=h32.shape)
    m[:] = h32.astype(np.float16)
    del m
    assert read(b, NPY) == open(want, "rb").read()                   # header included
    assert tb["repr_bytes"] == 128 + 64 * h32.shape[0] and ta["repr_bytes"] == 128 + 128 * h32.shape[0]
    # and `inference --representation_dtype float16` writes the same file
    d = tmp_path / "two16"
    d.mkdir()
    two, err = two_step(d, ev, QUICK, dtype="float16")
    assert err is None and read(two, NPY) == read(b, NPY)


# ---- 4. float32 untouched ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["reads_1", "reads_33", "reads_65", "64_sites_of_1", "bags_15_16_17", "one_site_5000", "empty_sites"])
def test_dtype_f32_is_read_representation(eng, case):
    import torch
    X, km, off = rand_sites(sorted(EDGE_BAGS).index(case), EDGE_BAGS[case])
    R = X.shape[0]
    tX, tk, to = to_device(X, km, off)
    want, want_p = eng.get_read_representation(tX, tk, to, want_read_probs=True)
    got = torch.full((R, 32), float(SENTINEL32), dtype=torch.float32, device="cuda:0")
    got_p = torch.full((R,), float(SENTINEL32), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    eng.read_representation_ptrs(tX.data_ptr(), tk.data_ptr(), to.data_ptr(), len(off) - 1, got.data_ptr(), "float32", got_p.data_ptr())
    eng.sync()
    assert eng.last_encoder_kernel == "enc_repr_kernel"
    assert np.array_equal(got.cpu().numpy().view(np.uint32), want.cpu().numpy().view(np.uint32))
    assert np.array_equal(got_p.cpu().numpy().view(np.uint32), want_p.cpu().numpy().view(np.uint32))
    host = np.empty((R, 32), np.float32)                             # host pointers, through the same chunk loop
    eng.read_representation_ptrs(X.ctypes.data, km.ctypes.data, off.ctypes.data, len(off) - 1, host.ctypes.data, _lib.REPR_DTYPES["float32"])
    assert np.array_equal(host.view(np.uint32), want.cpu().numpy().view(np.uint32))


# ---- 5. refusals, each followed by one correct call ------------------------------------------------------------------------------------
def test_dtype_2_is_einval_and_nothing_is_written(eng):
    import torch
    X, km, off = rand_sites(10, [20, 21])
    tX, tk, to = to_device(X, km, off)
    out = torch.full((41, 32), float(SENTINEL32), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    with pytest.raises(_lib.M6AError) as e:
        eng.read_representation_ptrs(tX.data_ptr(), tk.data_ptr(), to.data_ptr(), 2, out.data_ptr(), 2)
    assert e.value.code == -1 and "dtype 2" in str(e.value)
    eng.sync()
    assert np.all(out.cpu().numpy() == SENTINEL32)
    eng.read_representation_ptrs(tX.data_ptr(), tk.data_ptr(), to.data_ptr(), 2, out.data_ptr(), "float16")     # the correct call
    eng.sync()
    h16 = out.cpu().numpy().view(np.uint16).reshape(-1)[:41 * 32].reshape(41, 32)
    assert np.array_equal(h16, as_f16_bits(eng.get_read_representation(X, km, off)))


@pytest.fixture(scope="module")
def handle(bundled, eng):
    """the bundled file's sites on the device, inferred once, and the whole float32 file the writer makes of them"""
    ev, twin = bundled
    from m6anet_amd.constants import PRETRAINED_CONFIGS
    from m6anet_amd.data_utils import load_norm_factors
    p = _io.prep_sites(ev, norm=load_norm_factors(PRETRAINED_CONFIGS["HCT116_RNA002"][2]), n_threads=2)
    yield p, read(twin(()), NPY)
    p.close()


def test_writer_refusals(handle, eng, weights, tmp_path, monkeypatch):
    import torch
    p, want = handle
    path = str(tmp_path / "r.npy")
    assert p.n_reads * 128 + 128 == len(want) and 2 * p.n_reads * 128 > (1 << 20)        # the one round's two buffers exceed 1 MB
    with pytest.raises(_io.M6AIOError) as e:                          # dtype 2
        p.write_read_representation(eng, path, 2)
    assert e.value.code == -1 and "dtype 2" in str(e.value) and not os.path.exists(path)
    with pytest.raises(_io.M6AIOError) as e:                          # a NULL path
        p.write_read_representation(eng, None)
    assert e.value.code == -1
    if torch.cuda.device_count() >= 2:                                # a context of another device
        from m6anet_amd.engine import M6ANetEngine
        other = M6ANetEngine(weights=weights["hct116"], device=1)
        try:
            with pytest.raises(_io.M6AIOError) as e:
                p.write_read_representation(other, path)
            assert e.value.code == -1 and "device" in str(e.value) and not os.path.exists(path)
        finally:
            other.close()
    monkeypatch.setenv("M6A_PREP_BUDGET_MB", "1")                     # a budget below two rounds
    with pytest.raises(_io.M6AIOError) as e:
        p.write_read_representation(eng, path)
    assert e.value.code == -2 and "M6A_REPR_ROUND_KB" in str(e.value) and not os.path.exists(path)
    monkeypatch.setenv("M6A_REPR_ROUND_KB", "64")                     # a smaller round succeeds under the same budget, with the same bytes
    st = p.write_read_representation(eng, path)
    assert read(tmp_path, "r.npy") == want and st["n_rounds"] == stmt.n_rounds([int(x) for x in p.off], p.n_sites, 64) > 1
    assert st["round_bytes"] * 4 <= (1 << 20) and st["bytes"] == len(want) and st["d2h_bytes"] == len(want) - 128
    monkeypatch.delenv("M6A_PREP_BUDGET_MB")
    monkeypatch.delenv("M6A_REPR_ROUND_KB")
    st = p.write_read_representation(eng, path, "float32", 3)         # n_sites_limit; the file is truncated, not overwritten in place
    assert read(tmp_path, "r.npy") == stmt.header_bytes(int(p.off[3]), "float32") + want[128:128 + int(p.off[3]) * 128] and st["n_rows"] == int(p.off[3])
    st = p.write_read_representation(eng, path, "float16", 0)         # no site asked for: the header of an empty array
    assert read(tmp_path, "r.npy") == stmt.header_bytes(0, "float16") and st["n_rounds"] == 0
    assert np.load(path).shape == (0, 32)


def test_a_handle_with_no_site_is_refused(eng, tmp_path):
    rng = np.random.default_rng(5)
    f = G.File(rng)
    tx = G.Tx(rng, "FEW", 12, (3,))
    G.site_reads(f, tx, 3, range(5), mismatch=0)
    ev = tmp_path / "few.txt"
    ev.write_bytes(f.bytes())
    path = str(tmp_path / "none.npy")
    with _io.prep_sites(str(ev), n_threads=2) as p:
        assert p.n_sites == 0
        with pytest.raises(_io.M6AIOError) as e:
            p.write_read_representation(eng, path)
        assert e.value.code == -1 and "no site" in str(e.value) and not os.path.exists(path)
    c = G.case("combine", 1)                                          # the correct call: a handle with sites, the same context
    with _io.prep_sites(c.write(tmp_path)[0], n_threads=2) as p:
        st = p.write_read_representation(eng, path)
        X, km, off = p.inputs()
        assert st["n_rows"] == p.n_reads > 0
    got = np.load(path)
    assert np.array_equal(got.view(np.uint32), eng.get_read_representation(X, km, off).view(np.uint32))


# ---- 6. traffic ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float32", "float16"])
def test_traffic(bundled, tmp_path, dtype):
    ev, _ = bundled
    out = str(tmp_path / "without")
    t0 = cmd(["eventalign_inference", "--eventalign", ev, "--out_dir", out] + QUICK)
    assert not os.path.exists(os.path.join(out, NPY))
    assert t0["repr_rounds"] == 0 and t0["repr_bytes"] == 0 and all(t0["ms"][k] == 0 for k in ("repr_kernel", "repr_copy", "repr_write"))
    _, t1 = fused(tmp_path, ev, QUICK, dtype=dtype)
    row = 32 * stmt.ITEMSIZE[dtype]
    assert t1["d2h_bytes"] - t0["d2h_bytes"] == t1["n_reads"] * row
    assert t1["repr_rounds"] == 1 and t1["ms"]["repr_kernel"] > 0 and t1["ms"]["repr_copy"] > 0 and t1["ms"]["repr_write"] > 0
    assert 0 <= t1["peak_bytes"] - t0["peak_bytes"] <= 4 * t1["n_reads"] * row
