"""The closed-form site probability on the GPU (include/m6a.h: m6a_site_expectation, m6a_set_site_mode): the kernels give the bits of
tests/site_expectation_statement.py on every bag size and value edge, with host and device pointers, with and without the host
offsets; in M6A_SITE_EXPECTED every entry point delivers those bits whatever n_iters, the seed, the flush geometry, the job offset
or the feed batches are; the default mode is left as it was; and the two commands write them with --site_proba expected."""
import os
import subprocess
import sys

import numpy as np
import pytest

import eventalign_gen as G
import site_expectation_statement as SE
from m6anet_amd import _lib, synthetic
from m6anet_amd.constants import DEFAULT_MIN_READS, DEFAULT_PRETRAINED_MODEL, PRETRAINED_CONFIGS, asset_path
from m6anet_amd.engine import M6ANetEngine

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATA = os.path.join(REPO, "tests", "golden", "ref_tests_data")
CSVS = ("data.site_proba.csv", "data.indiv_proba.csv")
THR = np.float32(0.033379376)
SIZES = (1, 2, 19, 20, 21, 63, 64, 65, 127, 128, 129, 500, 1000)


@pytest.fixture(scope="module")
def eng(weights):
    e = M6ANetEngine(weights=weights["hct116"], device=0)
    yield e
    e.close()


def same_bits(a, b):
    """equal bit for bit; NaN (whatever its payload) only where the other is NaN"""
    a, b = np.asarray(a), np.asarray(b)
    nan = np.isnan(a)
    u = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and \
        np.array_equal(a[~nan].view(u), b[~nan].view(u))


def csr(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def probs(rng, n):
    """read probabilities as the encoder gives them: most near 0, some anywhere"""
    p = rng.random(n, np.float32) ** 4
    return np.where(rng.random(n) < 0.1, rng.random(n, np.float32), p).astype(np.float32)


def run_expectation(eng, p, off, K, pointers, hint):
    if pointers == "host":
        return eng.site_expectation(p, off, K, want_sigma=True, read_proba_threshold=THR)
    import torch
    tp, to = torch.from_numpy(p).cuda(), torch.from_numpy(off).cuda()
    if hint:
        eng.set_host_offsets(off)
    out = eng.site_expectation(tp, to, K, want_sigma=True, read_proba_threshold=THR)
    eng.sync()
    return tuple(t.cpu().numpy() for t in out)


def check_call(eng, p, off, K, pointers, hint, tag):
    want = SE.site_expectation(p, off, K, THR)                   # (site, sigma, mod)
    site, mod, sigma = run_expectation(eng, p, off, K, pointers, hint)
    assert same_bits(site, want[0]), (tag, "site_prob")
    assert same_bits(sigma, want[1]), (tag, "mc_sigma")
    assert same_bits(mod, want[2]), (tag, "mod_ratio")
    return site, mod


@pytest.mark.parametrize("pointers, hint", [("host", False), ("device", False), ("device", True)])
def test_bits_of_the_statement_on_every_bag_size(eng, pointers, hint):
    rng = np.random.default_rng(11)
    for n in SIZES + (5000,):
        off = csr([n] * (1 if n == 5000 else 3))
        p = probs(rng, int(off[-1]))
        _, mod = check_call(eng, p, off, 20, pointers, hint, n)
        assert eng.last_pool_variant == ("expected-lane" if n <= 32 else "expected-wave"), n      # equal bags of <= 32 reads: a lane per site
        if pointers == "host":                                 # mod_ratio as m6a_site_pool gives it
            assert same_bits(mod, eng.calculate_site_proba(p, off, 1, 20, THR)[1]), n
    for S in (1, 2, 63, 64, 65, 1000):                          # uniform 20-read jobs
        off = csr([20] * S)
        check_call(eng, probs(rng, 20 * S), off, 20, pointers, hint, "uniform %d" % S)
        assert eng.last_pool_variant == "expected-lane"
    for n, S in ((32, 700), (31, 300), (7, 1000), (3, 257)):    # the lane variant's other sizes, whole float4s and single floats
        off = csr([n] * S)
        check_call(eng, probs(rng, n * S), off, 20, pointers, hint, "uniform %d x %d" % (S, n))
        assert eng.last_pool_variant == "expected-lane"
    if pointers == "device":                                    # read_prob off the 16-byte grid: the lane variant without float4s
        import torch
        off = csr([20] * 300)
        p = probs(rng, 20 * 300)
        buf = torch.zeros(20 * 300 + 1, dtype=torch.float32, device="cuda:0")
        buf[1:] = torch.from_numpy(p)
        out = eng.site_expectation(buf[1:], torch.from_numpy(off).cuda(), 20, want_sigma=True, read_proba_threshold=THR)
        eng.sync()
        want = SE.site_expectation(p, off, 20, THR)
        assert eng.last_pool_variant == "expected-lane" and buf[1:].data_ptr() % 16 == 4
        assert all(same_bits(g.cpu().numpy(), w) for g, w in zip(out, (want[0], want[2], want[1])))
    sizes = rng.permutation(np.concatenate([np.repeat(SIZES, 3), [5000, 0], rng.integers(1, 300, 200)]))
    off = csr(sizes)                                            # one call mixing all sizes, an empty bag among them
    check_call(eng, probs(rng, int(off[-1])), off, 20, pointers, hint, "mixed")
    assert eng.last_pool_variant == "expected-wave"
    small = csr(rng.integers(0, 33, 500))                       # ragged, every bag <= 32 reads: still a wavefront per site
    check_call(eng, probs(rng, int(small[-1])), small, 20, pointers, hint, "small ragged")
    assert eng.last_pool_variant == "expected-wave"


@pytest.mark.parametrize("K", [1, 20, 64])
@pytest.mark.parametrize("pointers", ["host", "device"])
def test_value_edges(eng, K, pointers):
    f32 = np.float32
    one_hot = np.zeros(20, f32)
    one_hot[7] = 1.0
    bags = [np.zeros(20, f32), np.ones(1, f32), one_hot, np.full(20, 1e-30, f32), np.full(1, 1e-30, f32),
            np.full(20, f32(1.0) - f32(2.0 ** -24), f32), np.full(1, f32(1.0) - f32(2.0 ** -24), f32), np.ones(65, f32),
            np.array([0.25, np.nan, 0.5], f32), np.array([1.5, 0.25, -0.5], f32), np.array([np.inf, 0.5], f32), np.full(70, 0.5, f32)]
    site, _ = check_call(eng, np.concatenate(bags), csr([b.size for b in bags]), K, pointers, False, "edges")    # a wavefront per site
    assert eng.last_pool_variant == "expected-wave"
    assert site[0] == 0.0 and not np.signbit(site[0]) and site[1] == 1.0 and site[3] == 0.0 and site[4] == 0.0
    for k, b in enumerate(bags):                                # each bag twice in a call of its own: a lane per site up to 32 reads
        site, _ = check_call(eng, np.concatenate([b, b]), csr([b.size] * 2), K, pointers, False, "edge bag %d" % k)
        assert eng.last_pool_variant == ("expected-lane" if b.size <= 32 else "expected-wave")


def test_expected_mode_is_one_value_across_entry_points(eng):
    for bag, variant in (((20, 90), "expected-wave"), (20, "expected-lane")):
        d = synthetic.make_sites(48, bag, seed=3)
        X, km, off = d["X"], d["site_kmers"], d["off"]
        eng.set_site_mode("sampled")
        rp = eng.get_read_probability(X, km, off)
        want_site, want_mod = eng.site_expectation(rp, off, 20, read_proba_threshold=THR)
        assert same_bits(want_site, SE.site_expectation(rp, off, 20)[0])
        eng.set_site_mode("expected")
        try:
            for n_iters in (1, 1000):
                for seed in (0, 7):
                    for bs, spb, job_off in ((16, 2, 0), (8, 3, 8), (16, 2, 16)):      # two flush geometries, job offsets that start a group
                        eng.set_job_offset(job_off)
                        got = eng.infer(X, km, off, n_iters, 20, THR, seed, bs, spb)
                        assert eng.last_pool_variant == variant
                        assert same_bits(got[0], rp) and same_bits(got[1], want_site) and same_bits(got[2], want_mod), (n_iters, seed, bs, spb)
            eng.set_job_offset(0)
            site, mod = eng.calculate_site_proba(rp, off, 1000, 20, THR, seed=5)
            assert same_bits(site, want_site) and same_bits(mod, want_mod) and eng.last_pool_variant == variant
            import torch
            t = [torch.from_numpy(a).cuda() for a in (X, km, off)]
            eng.set_host_offsets(off)
            got = eng.infer(t[0], t[1], t[2], 1000, 20, THR)
            eng.sync()
            assert same_bits(got[1].cpu().numpy(), want_site) and same_bits(got[2].cpu().numpy(), want_mod)
            for step in (1, 7, 16):
                eng.job_begin(1000, 20, THR, seed=step)
                for a in range(0, 48, step):
                    b = min(a + step, 48)
                    eng.job_feed(X[off[a]:off[b]], km[a:b], off[a:b + 1] - off[a])
                got = eng.job_end()
                assert same_bits(got[0], rp) and same_bits(got[1], want_site) and same_bits(got[2], want_mod), step
            eng.set_job_offset(24)                                  # not a group start at 16 x 2: refused in this mode as in the default
            with pytest.raises(_lib.M6AError) as e:
                eng.infer(X, km, off, 5, 20, THR)
            assert e.value.code == -1
        finally:
            eng.set_job_offset(0)
            eng.set_site_mode("sampled")


def test_default_mode_is_unaffected(eng, weights):
    fresh = M6ANetEngine(weights=weights["hct116"], device=0)      # a context on which the mode is never set
    try:
        for bag in (20, (20, 90)):
            d = synthetic.make_sites(64, bag, seed=4)
            want = fresh.infer(d["X"], d["site_kmers"], d["off"], 50, 20, THR, 3)
            eng.set_site_mode("expected")
            mid = eng.infer(d["X"], d["site_kmers"], d["off"], 50, 20, THR, 3)
            eng.set_site_mode("sampled")
            got = eng.infer(d["X"], d["site_kmers"], d["off"], 50, 20, THR, 3)
            assert not eng.last_pool_variant.startswith("expected") and eng.last_pool_variant == fresh.last_pool_variant
            assert all(same_bits(g, w) for g, w in zip(got, want))
            assert not same_bits(mid[1], want[1]) and same_bits(mid[2], want[2])       # another site_prob, the same mod_ratio
    finally:
        fresh.close()


def test_refusals_are_followed_by_a_correct_call(eng):
    import torch
    rng = np.random.default_rng(2)
    off = csr([20] * 10)
    p = probs(rng, 200)
    for bad in (2, -1, 7):
        assert eng._L.m6a_set_site_mode(eng._h, bad) == -1 and b"site mode" in eng._L.m6a_last_error(eng._h)
    with pytest.raises(ValueError):
        eng.set_site_mode("exact")
    site, _ = eng.calculate_site_proba(p, off, 10, 20, THR)         # still the default mode
    assert not eng.last_pool_variant.startswith("expected")
    with pytest.raises(_lib.M6AError) as e:
        eng.site_expectation(torch.from_numpy(p).cuda(), off, 20)   # read_prob on the device, off on the host
    assert e.value.code == -1
    with pytest.raises(_lib.M6AError) as e:
        eng.site_expectation(p, off, 65)                            # n_samples beyond M6A_MAX_SAMPLES, as in m6a_site_pool
    assert e.value.code == -1
    check_call(eng, p, off, 20, "host", False, "after refusals")
    assert eng.last_pool_variant == "expected-lane"


# ---- the commands -------------------------------------------------------------------------------------------------------------
def cli(argv, env=None):
    e = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
    e.update(env or {})
    r = subprocess.run([sys.executable, "-m", "m6anet_amd"] + argv, env=e, capture_output=True, text=True, timeout=300, cwd=REPO)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])


def read(out_dir, fn):
    return open(os.path.join(out_dir, fn), "rb").read()


def test_inference_site_proba_expected(tmp_path, eng):
    from m6anet_amd.data_utils import load_sites_native
    base, exp, exp2 = (str(tmp_path / d) for d in ("base", "exp", "exp_seed"))
    common = ["inference", "--input_dir", DATA, "--n_processes", "2"]
    cli(common + ["--out_dir", base, "--num_iterations", "20"])
    cli(common + ["--out_dir", exp, "--site_proba", "expected"])
    cli(common + ["--out_dir", exp2, "--site_proba", "expected", "--num_iterations", "7", "--seed", "9", "--batch_size", "8"])
    assert read(exp, CSVS[1]) == read(base, CSVS[1])                # data.indiv_proba.csv: byte-identical to the default run
    assert all(read(exp2, fn) == read(exp, fn) for fn in CSVS)      # --num_iterations, --seed and the flush geometry have no effect
    rows_b = [l.split(",") for l in read(base, CSVS[0]).decode().splitlines()]
    rows_e = [l.split(",") for l in read(exp, CSVS[0]).decode().splitlines()]
    assert len(rows_e) == len(rows_b) == 102 and rows_e[0] == rows_b[0]
    assert [r[:3] + r[4:] for r in rows_e] == [r[:3] + r[4:] for r in rows_b]        # every column but probability_modified
    assert [r[3] for r in rows_e] != [r[3] for r in rows_b]
    norm = asset_path(PRETRAINED_CONFIGS[DEFAULT_PRETRAINED_MODEL][2])
    batch = load_sites_native([DATA], DEFAULT_MIN_READS, norm, n_threads=2)
    rp = eng.get_read_probability(batch.X, batch.site_kmers, batch.off)
    site, _ = eng.site_expectation(rp, batch.off, 20)
    assert [r[3] for r in rows_e[1:]] == ["%.16f" % float(v) for v in site]


def test_inference_gpus_2_writes_the_one_gpu_bytes(tmp_path):
    one, two = str(tmp_path / "one"), str(tmp_path / "two")
    common = ["inference", "--input_dir", DATA, "--n_processes", "2", "--site_proba", "expected"]
    cli(common + ["--out_dir", one])
    cli(common + ["--out_dir", two, "--gpus", "2"], env={"M6A_SHARE_GPU": "1"})      # two ranks share the GPU
    assert all(read(two, fn) == read(one, fn) for fn in CSVS)
    assert read(one, CSVS[0]).count(b"\n") == 102


def test_eventalign_inference_site_proba_expected(tmp_path):
    ev = str(tmp_path / "plain.txt")
    with open(ev, "wb") as f:
        f.write(G.generate("plain", 1))
    prep, two, host, dev, base = (str(tmp_path / d) for d in ("prep", "two", "host", "dev", "base"))
    cli(["dataprep", "--eventalign", ev, "--out_dir", prep, "--n_processes", "2"])
    cli(["inference", "--input_dir", prep, "--out_dir", two, "--n_processes", "2", "--site_proba", "expected"])
    cli(["eventalign_inference", "--eventalign", ev, "--out_dir", host, "--n_processes", "2", "--site_proba", "expected", "--csv", "host"])
    cli(["eventalign_inference", "--eventalign", ev, "--out_dir", dev, "--n_processes", "2", "--site_proba", "expected", "--csv", "device"])
    cli(["eventalign_inference", "--eventalign", ev, "--out_dir", base, "--n_processes", "2", "--num_iterations", "20"])
    assert read(two, CSVS[0]).count(b"\n") > 3
    for fn in CSVS:
        assert read(host, fn) == read(two, fn) and read(dev, fn) == read(two, fn), fn
    assert read(base, CSVS[1]) == read(two, CSVS[1]) and read(base, CSVS[0]) != read(two, CSVS[0])
