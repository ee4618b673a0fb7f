"""GPU tests of the evaluation half (m6a_bag_forward, m6a_validate_pool, m6a_validate) and of every pooling kernel at the
value edges of read probabilities: NaN, the threshold and its float neighbours, both zeros, one, subnormals.

Everything here is bit-exact (np.array_equal, equal_nan where NaN is expected): the kernels replay NumPy's streams and
its float32 operations in its order.  The references are the plain NumPy statements in tests/test_oracle_golden.py
(np_validate, np_pool_one_group) where a case is small (T * S <= 20 000) and the CPU oracle above that; the oracle is held
to the same statements on the CPU.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from m6anet_amd import synthetic                                                             # noqa: E402
from test_oracle_golden import THR, MASK_BAGS, edge_probs, np_pool_one_group, np_validate    # noqa: E402

NP_LIMIT = 20000                       # T * S up to which the NumPy statement is the reference (the oracle above)


@pytest.fixture(scope="module")
def orc():
    from oracle import m6a_oracle
    m6a_oracle.build()
    return m6a_oracle


@pytest.fixture(scope="module")
def engines(weights):
    from m6anet_amd.engine import M6ANetEngine
    return {name: M6ANetEngine(weights=w) for name, w in weights.items()}


@pytest.fixture(scope="module")
def eng(engines):
    return engines["hct116"]


def to_dev(*arrays):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0") for a in arrays]


def want_validate(orc, p, off, T, seed, k):
    """The reference for a validate case: the NumPy statement when small, else the oracle (held to it on the CPU)."""
    if T * (len(off) - 1) <= NP_LIMIT:
        return np_validate(p, off, T, seed, k)
    return orc.validate(p, off, T, seed=seed, k=k)


def rand_probs(seed, n):
    return (np.random.Generator(np.random.PCG64(seed)).random(n, dtype=np.float32) ** 4).astype(np.float32)


# ------------------------------------------------------------------ validation-style forward -----
# (bags, T, k, seed).  One site at T >= 24 is where np.mean(y, axis=0) takes NumPy's pairwise sum instead of the
# pass-after-pass one; k = 20 takes sampled_noisy_or_kernel's dwordx4 path, every other k its scalar one.
VAL_GPU_CASES = [([25], 1, 20, 0), ([25], 9, 20, 1), ([25], 24, 20, 2), ([25], 129, 20, 3), ([25], 1000, 20, 4),
                 ([64], 200, 20, 5), ([25], 4099, 7, 6), ([64], 1000, 64, 2**31), ([300], 2500, 21, 2**32 - 1),
                 (MASK_BAGS, 5, 20, 0), (MASK_BAGS, 3, 1, 2**31), (MASK_BAGS, 3, 7, 2**32 - 1), (MASK_BAGS, 4, 21, 0),
                 (MASK_BAGS[4:], 3, 64, 2**31), ([70000, 20, 65536, 21], 2, 20, 2**32 - 1), ([20] * 50, 7, 20, 0),
                 ([7, 9, 7, 30], 5, 7, 2**31), ([21, 40] * 30, 9, 21, 0), ([20, 33, 64] * 400, 30, 20, 11)]


def val_inputs(bags, seed):
    """One site: random probabilities (the mean's summation order shows in their bits); several: edge_probs (NaN, 0, 1,
    the threshold's neighbours)."""
    if len(bags) == 1:
        return rand_probs(seed, bags[0]), np.array([0, bags[0]], np.int64)
    return edge_probs(bags, seed)


@pytest.mark.parametrize("bags,T,k,seed", VAL_GPU_CASES)
def test_validate_pool_vs_numpy(eng, orc, bags, T, k, seed):
    p, off = val_inputs(bags, len(bags) + T)
    want_y, want_avg = want_validate(orc, p, off, T, seed, k)
    y, avg = eng.validate_pool(p, off, T, n_samples=k, seed=seed)
    assert np.array_equal(y, want_y, equal_nan=True)
    assert np.array_equal(avg, want_avg, equal_nan=True), np.abs(avg - want_avg).max()
    ty, tavg = eng.validate_pool(*to_dev(p, off), T, n_samples=k, seed=seed)
    eng.sync()
    assert np.array_equal(ty.cpu().numpy(), want_y, equal_nan=True)
    assert np.array_equal(tavg.cpu().numpy(), want_avg, equal_nan=True)


@pytest.mark.parametrize("n_sites,bag,T,k", [(1, 25, 1000, 20), (1, 40, 300, 7), (1, 16, 24, 16), (3, 20, 50, 20),
                                             (400, (20, 90), 6, 20), (400, (21, 90), 6, 21)])
def test_validate_forward_is_validate_pool_of_its_read_probs(engines, n_sites, bag, T, k):
    """m6a_validate = encoder + m6a_validate_pool: with and without read probabilities requested, host and device, the
    same bits as validate_pool of the read probabilities it returns -- and the NumPy statement of those."""
    e = engines["hek293t_glori"]
    d = synthetic.make_sites(n_sites, bag, seed=T + k)
    y, avg, rp = e.validate_forward(d["X"], d["site_kmers"], d["off"], T, n_samples=k, seed=T, want_read_probs=True)
    y2, avg2 = e.validate_forward(d["X"], d["site_kmers"], d["off"], T, n_samples=k, seed=T, want_read_probs=False)
    py, pavg = e.validate_pool(rp, d["off"], T, n_samples=k, seed=T)
    ny, navg = np_validate(rp, d["off"], T, T, k)
    for gy, gavg in ((y, avg), (y2, avg2), (py, pavg)):
        assert np.array_equal(gy, ny) and np.array_equal(gavg, navg)
    ty, tavg, trp = e.validate_forward(*to_dev(d["X"], d["site_kmers"], d["off"]), T, n_samples=k, seed=T, want_read_probs=True)
    e.sync()
    assert np.array_equal(trp.cpu().numpy(), rp)
    assert np.array_equal(ty.cpu().numpy(), ny) and np.array_equal(tavg.cpu().numpy(), navg)


@pytest.mark.parametrize("threads", ["0", "3"])
def test_validate_sampler_threads(eng, monkeypatch, threads):
    """More than 8 192 (pass, site) items: the sampler's walk hands blocks to M6A_VALIDATE_THREADS workers (0: it shuffles
    them itself).  Same bits either way, NaN / 0 / 1 read probabilities included."""
    bags = np.random.Generator(np.random.PCG64(8)).integers(20, 300, size=2500)
    p, off = edge_probs(bags, 9)
    T = 4
    assert T * len(bags) > 8192
    monkeypatch.setenv("M6A_VALIDATE_THREADS", threads)
    y, avg = eng.validate_pool(p, off, T, seed=77)
    want_y, want_avg = np_validate(p, off, T, 77)
    assert np.isnan(want_avg).any() and (want_y == 1).any()
    assert np.array_equal(y, want_y, equal_nan=True)
    assert np.array_equal(avg, want_avg, equal_nan=True)


# ------------------------------------------------------------------ m6a_bag_forward -----
@pytest.mark.parametrize("bag", [1, 2, 15, 16, 17, 20, 21, 64, 700])
def test_bag_forward_is_the_oracle_bit_for_bit(engines, orc, weights, bag):
    """MILModel.forward on fixed bags: the encoder (enc_kernel below 16 reads, enc_site16_kernel from 16) and the noisy-or,
    against the oracle's encoder and product, every checkpoint, host and device pointers."""
    for B in (1, 3, 5000):
        g = np.random.Generator(np.random.PCG64(bag * 10 + B))
        X = np.clip(g.standard_normal((B, bag, 9)), -6, 6).astype(np.float32)
        km = g.integers(0, 66, size=(B, 3)).astype(np.uint8)
        off = np.arange(B + 1, dtype=np.int64) * bag
        for name, e in engines.items():
            want = orc.bag_noisy_or(orc.encode_reads(weights[name], X.reshape(-1, 9), km, off, n_threads=8), bag)
            got = e.forward(X, km, bag=bag)
            assert e.last_encoder_kernel == ("enc_site16_kernel" if bag >= 16 else "enc_kernel")
            assert np.array_equal(got, want), (name, B)
            tgot = e.forward(*to_dev(X, km), bag=bag)
            e.sync()
            assert np.array_equal(tgot.cpu().numpy(), want), (name, B, "device")


# ------------------------------------------------------------------ pooling at the value edges -----
def pool_case(eng, orc, p, off, T, K, spb, variant):
    site, mod = eng.calculate_site_proba(p, off, T, K, THR, seed=T, save_per_batch=spb)
    assert eng.last_pool_variant == variant
    want_site, want_mod = orc.site_pool(p, off, T, THR, seed=T, save_per_batch=spb, n_samples=K)
    assert np.array_equal(site, want_site, equal_nan=True), (variant, T, spb)
    assert np.array_equal(mod, want_mod), (variant, T, spb)
    if spb == 1 and T * (len(off) - 1) <= NP_LIMIT:
        np_site, np_mod = np_pool_one_group(p, off, T, THR, T, K)
        assert np.array_equal(site, np_site, equal_nan=True), (variant, T)
        assert np.array_equal(mod, np_mod), (variant, T)
    if T <= 3:   # which sites drew a NaN read: the index replay and the propagation together
        assert np.array_equal(np.isnan(site), np.isnan(want_site)) and np.isnan(site).any()
    return site, mod


def check_threshold_sites(p, off, mod):
    """edge_probs' sites 0, 4, 8, ... hold only thr and its two neighbours: mod_ratio is the count of p >= thr, which a
    strict comparison would get wrong on every such site holding thr itself."""
    ge = np.array([np.mean(p[off[s]:off[s + 1]] >= THR) for s in range(0, len(off) - 1, 4)])
    gt = np.array([np.mean(p[off[s]:off[s + 1]] > THR) for s in range(0, len(off) - 1, 4)])
    assert (ge != gt).any()
    assert np.array_equal(mod[0::4], ge)


@pytest.mark.parametrize("n", [1, 4, 20, 32])
@pytest.mark.parametrize("mode,variant", [(2, "table-reg"), (1, "table")])
def test_pool_uniform_kernels_at_value_edges(eng, orc, n, mode, variant):
    S = 600
    p, off = edge_probs([n] * S, n)
    eng.set_table_variant(mode)
    try:
        for T in (1, 3, 50):
            for spb in (2, 1):
                _, mod = pool_case(eng, orc, p, off, T, 20, spb, variant)
                check_threshold_sites(p, off, mod)
    finally:
        eng.set_table_variant(0)


@pytest.mark.parametrize("K", [20, 7])
@pytest.mark.parametrize("driver,variant", [(1, "scan-group"), (2, "scan-site"), (3, "ragged-table")])
def test_pool_ragged_kernels_at_value_edges(eng, orc, K, driver, variant):
    bags = np.repeat([1, 2, 20, 33, 64, 200], 4)
    bags = np.concatenate([bags, np.random.Generator(np.random.PCG64(K)).permutation(np.tile(bags, 8))])
    p, off = edge_probs(bags, K)
    eng.set_scan_driver(driver)
    try:
        for T in (1, 3, 50, 1000):
            for spb in (2, 1):
                _, mod = pool_case(eng, orc, p, off, T, K, spb, variant)
                check_threshold_sites(p, off, mod)
    finally:
        eng.set_scan_driver(0)


# ------------------------------------------------------------------ end to end with NaN features -----
@pytest.mark.parametrize("bag,knob,mode", [((20, 60), "scan", 0), ((20, 60), "scan", 1), ((20, 60), "scan", 2),
                                           ((20, 60), "scan", 3), (20, "table", 1), (20, "table", 2)])
def test_infer_with_nan_features(eng, orc, bag, knob, mode):
    """A NaN feature makes that read's probability NaN and nothing else; pooling takes it from there like the oracle."""
    d = synthetic.make_sites(800, bag, seed=mode + 3)
    X = d["X"].copy()
    bad = np.random.Generator(np.random.PCG64(5)).choice(X.shape[0], 12, replace=False)
    X[bad, bad % 9] = np.nan
    setter = eng.set_scan_driver if knob == "scan" else eng.set_table_variant
    setter(mode)
    try:
        rp, site, mod = eng.infer(X, d["site_kmers"], d["off"], 100, seed=4)
    finally:
        setter(0)
    mask = np.zeros(X.shape[0], bool)
    mask[bad] = True
    assert np.array_equal(np.isnan(rp), mask)
    want_site, want_mod = orc.site_pool(rp, d["off"], 100, THR, seed=4)
    assert np.isnan(want_site).any()
    assert np.array_equal(site, want_site, equal_nan=True)
    assert np.array_equal(mod, want_mod)


# ------------------------------------------------------------------ errors leave the context usable -----
def test_validate_errors_then_a_correct_call(eng):
    from m6anet_amd._lib import M6AError
    p, off = edge_probs([30, 19, 40], 1)

    def correct_call():
        y, avg = eng.validate_pool(p[:70], np.array([0, 30, 70], np.int64), 3, seed=9)
        want_y, want_avg = np_validate(p[:70], np.array([0, 30, 70], np.int64), 3, 9)
        assert np.array_equal(y, want_y, equal_nan=True) and np.array_equal(avg, want_avg, equal_nan=True)

    with pytest.raises(M6AError, match="M6A_EINVAL.*site 1 has 19 reads"):
        eng.validate_pool(p, off, 2)
    correct_call()
    for k in (0, 65):
        with pytest.raises(M6AError, match="M6A_EINVAL"):
            eng.validate_pool(p, off, 2, n_samples=k)
        correct_call()
    with pytest.raises(M6AError, match="M6A_EINVAL"):
        eng.validate_pool(p, off, 0)
    correct_call()
    # T * S * k > 2e9: refused before off[] or any output is touched, so short arrays are safe to pass
    L, h = eng._L, eng._h
    y, avg = np.empty(4, np.float32), np.empty(4, np.float32)
    X, km = np.zeros((89, 9), np.float32), np.zeros((3, 3), np.uint8)
    assert L.m6a_validate_pool(h, p.ctypes.data, off.ctypes.data, 10**8, 1001, 20, 0, y.ctypes.data, avg.ctypes.data) == -6
    assert b"too large" in L.m6a_last_error(h)
    correct_call()
    assert L.m6a_validate(h, X.ctypes.data, km.ctypes.data, off.ctypes.data, 10**8, 1001, 20, 0, None, y.ctypes.data,
                          avg.ctypes.data) == -6
    correct_call()
