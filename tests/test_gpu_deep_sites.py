"""The kernels that walk one bag, on the shapes of tests/deep_site_cases.py: bags of more than 2^16 reads and pairs whose counts pass
2^32 -- where a 16-bit index, a 32-bit count or a 32-bit product would wrap.  tests/test_deep_sites.py holds the references to
their size conditions, to closed forms and to scipy on the CPU.

  * m6a_site_ranksum, m6a_site_ks: three pairs of 70000 x 62000 reads and the same swapped, gt, eq, tie, d_pos and d_neg above 2^32 and
    a tie group above 2^16; m6a_site_signal_ranksum, m6a_site_signal_ks: one pair of 36000 x 30000 rows with those constructions in
    columns 0, 4 and 8 (a tie group of 66 000, tie above 2^32, n m above 2^30) and a NaN in column 2.  Device and host pointers, every
    output bit for bit, sentinels around the outputs.  A pair of 2^20 + 1 pooled reads is undefined at once and the context goes on.
    Measured on an MI355X: 4.2 to 4.3 s per scalar test and 5.0 to 5.5 s per nine-column test (27 s at 70000 x 62000 rows, which is
    why that pair is smaller): N^2 compares on one wavefront.
  * m6a_site_pool's scan kernels on the bags BIG (up to 131 073 reads) with an empty and a one-read site: the oracle's bits.
  * the encoder kernels and the read representation on sites of up to 70 000 reads (more than 2^11 tiles of 32 reads in one site).
  * m6a_site_expectation on bags of up to 131 073 reads: the statement's bits.
  * the pinned staging ring and the streaming job at M6A_STAGE_MB=1 (29 127 reads per slot): dozens of chunks, a bag larger than a
    slot, offsets larger than a slot, and a site the streaming chunk refuses."""
import numpy as np
import pytest

import deep_site_cases as D
from m6anet_amd import _lib
from m6anet_amd.engine import M6ANetEngine, pinned_empty
from test_gpu_parity import THR, rand_probs, rand_sites, same_sites
from test_gpu_site_expectation import check_call as check_expectation
from test_oracle_golden import edge_probs

pytestmark = pytest.mark.gpu
FILL = 7
RANKSUM = ("gt", "eq", "tie", "z")
KS = ("d_pos", "d_neg", "med_a", "med_b")


@pytest.fixture(scope="module")
def orc():
    from oracle import m6a_oracle
    m6a_oracle.build()
    return m6a_oracle


@pytest.fixture(scope="module")
def eng(weights):
    e = M6ANetEngine(weights=weights["hct116"], device=0)
    yield e
    e.close()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def to_device(*arrays):
    import torch
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0") for a in arrays)


# ------------------------------------------------------------------ pairwise statistics past 2^32 -----
def run_pairs(eng, what, sets, pointers, width=1):
    """the identity pairing of `sets` through the engine's *_ptrs call for `what` (RANKSUM or KS), with a sentinel before and behind each
    of the four outputs; returns them, each [P] or [P, 9], without the sentinels"""
    n_int = 3 if what is RANKSUM else 2
    call = {(RANKSUM, 1): eng.site_ranksum_ptrs, (RANKSUM, 9): eng.site_signal_ranksum_ptrs, (KS, 1): eng.site_ks_ptrs,
            (KS, 9): eng.site_signal_ks_ptrs}[what, width]
    P = sets[1].size - 1
    if pointers == "host":
        va, oa, vb, ob = sets
        out = [np.full(width * P + 2, FILL, np.int64) for _ in range(n_int)] + [np.full(width * P + 2, float(FILL), np.float64) for _ in range(4 - n_int)]
        ptr = lambda x, skip=0: x.ctypes.data + skip            # noqa: E731
    else:
        import torch
        va, oa, vb, ob = to_device(*sets)
        out = [torch.full((width * P + 2,), FILL, dtype=torch.int64, device="cuda:0") for _ in range(n_int)] + \
              [torch.full((width * P + 2,), float(FILL), dtype=torch.float64, device="cuda:0") for _ in range(4 - n_int)]
        torch.cuda.synchronize()
        ptr = lambda x, skip=0: x.data_ptr() + skip             # noqa: E731
    call(ptr(va), ptr(oa), P, ptr(vb), ptr(ob), P, None, None, P, *[ptr(o, 8) for o in out])
    if pointers == "device":
        eng.sync()
        out = [o.cpu().numpy() for o in out]
    for o in out:
        assert o[0] == FILL and o[-1] == FILL
    return [o[1:-1].reshape((P,) if width == 1 else (P, width)) for o in out]


def check_pairs(got, want, what, names):
    for g, w, field in zip(got, want, what):
        assert D.same_bits(np.ascontiguousarray(g), np.ascontiguousarray(w)), (field, [names[k] for k in np.argwhere(g != w)[:, 0][:6]], g, w)


@pytest.mark.parametrize("pointers", ["device", "host"])
def test_ranksum_counts_past_2_32(eng, pointers):
    check_pairs(run_pairs(eng, RANKSUM, D.scalar_sets(), pointers), D.scalar_ranksum_want(), RANKSUM, D.NAMES)


@pytest.mark.parametrize("pointers", ["device", "host"])
def test_ks_integers_past_2_32(eng, pointers):
    check_pairs(run_pairs(eng, KS, D.scalar_sets(), pointers), D.scalar_ks_want(), KS, D.NAMES)


@pytest.mark.parametrize("pointers", ["device", "host"])
def test_signal_ranksum_counts_past_2_32(eng, pointers):
    check_pairs(run_pairs(eng, RANKSUM, D.signal_sets(), pointers, 9), D.signal_ranksum_want(), RANKSUM, ["the pair"])


@pytest.mark.parametrize("pointers", ["device", "host"])
def test_signal_ks_integers_past_2_32(eng, pointers):
    check_pairs(run_pairs(eng, KS, D.signal_sets(), pointers, 9), D.signal_ks_want(), KS, ["the pair"])


@pytest.mark.parametrize("pointers", ["device", "host"])
def test_a_pair_of_2_20_and_one_pooled_reads_is_undefined_at_once(eng, pointers):
    """2^19 + 1 and 2^19 reads: (-1, -1, -1, NaN) and (-1, -1, NaN, NaN) without a compare -- counted, the pair would take the wavefront
    about a minute -- beside a pair of 30 and 25 reads in the same call; the context then answers a correct call"""
    sets, names = D.limit_sets(), ["2^20 + 1 pooled", "30 x 25"]
    want_rs, want_ks = D.limit_want()
    assert want_rs[0][0] == -1 and want_ks[0][0] == -1 and want_rs[0][1] >= 0
    check_pairs(run_pairs(eng, RANKSUM, sets, pointers), want_rs, RANKSUM, names)
    check_pairs(run_pairs(eng, KS, sets, pointers), want_ks, KS, names)
    va, oa, vb, ob = sets
    small = (va[oa[1]:], oa[1:] - oa[1], vb[ob[1]:], ob[1:] - ob[1])
    check_pairs(run_pairs(eng, RANKSUM, small, pointers), [w[1:] for w in want_rs], RANKSUM, names[1:])
    check_pairs(run_pairs(eng, KS, small, pointers), [w[1:] for w in want_ks], KS, names[1:])


# ------------------------------------------------------------------ pooling past 2^16 -----
POOL_BAGS = D.BIG[:5] + [0] + D.BIG[5:] + [1]


@pytest.mark.parametrize("spb", [2, 1])
@pytest.mark.parametrize("inputs", ["edges", "random"])
def test_pool_scan_on_bags_past_2_16(eng, orc, inputs, spb):
    """test_pool_scan_vs_oracle (tests/test_gpu_parity.py) on the bags BIG with an empty and a one-read site among them: NaN, the
    threshold and its neighbours, zeros and one (edge_probs) or skewed random probabilities"""
    if inputs == "edges":
        p, off = edge_probs(POOL_BAGS, D.SEED)
    else:
        off = D.csr(POOL_BAGS)
        p = rand_probs(D.SEED, off)
    empty = np.diff(off) == 0
    assert empty.sum() == 1 and int(np.diff(off).max()) == 131073
    try:
        for T in (7, 100):
            for K in (20, 7):
                want_site, want_mod = orc.site_pool(p, off, T, THR, seed=D.SEED, save_per_batch=spb, n_samples=K)
                assert np.array_equal(np.isnan(want_mod), empty)
                for driver, name in ((1, "scan-group"), (2, "scan-site"), (3, "ragged-table"), (0, None)):
                    eng.set_scan_driver(driver)
                    if driver == 3:                           # index tables exist for bags of <= 4096 reads
                        with pytest.raises(_lib.M6AError, match="M6A_EUNSUPPORTED"):
                            eng.calculate_site_proba(p, off, T, K, THR, seed=D.SEED, save_per_batch=spb)
                        continue
                    site, mod = eng.calculate_site_proba(p, off, T, K, THR, seed=D.SEED, save_per_batch=spb)
                    assert (eng.last_pool_variant == name) if name else eng.last_pool_variant.startswith("scan"), eng.last_pool_variant
                    assert same_sites(site, want_site), (T, K, driver, np.flatnonzero(~((site == want_site) | (np.isnan(site) & np.isnan(want_site)))))
                    assert np.array_equal(mod, want_mod, equal_nan=True), (T, K, driver)
    finally:
        eng.set_scan_driver(0)


# ------------------------------------------------------------------ the encoder on one very long site -----
@pytest.fixture(scope="module")
def long_sites(orc, weights):
    """name -> (X, km, off, the oracle's read_prob, its representation): sites of up to 70 000 reads, all of >= 16 reads, and the same
    bags with a one-read site behind them"""
    out = {}
    for name, bags in (("bags of 16 and more", D.ENCODER_BAGS), ("with a bag of one", D.ENCODER_BAGS + [1])):
        X, km, off = rand_sites(D.SEED, bags)
        p, h, _ = orc.encode_layers(weights["hct116"], X, km, off)
        out[name] = (X, km, off, p, h)
    return out


def test_encoder_kernels_on_sites_past_2_16_reads(eng, long_sites):
    X, km, off, want, _ = long_sites["bags of 16 and more"]
    assert int(np.diff(off).max()) > 32 << 11                     # one site spans more than 2^11 tiles of 32 reads
    try:
        for variant, kernel, exact in ((0, "enc_site16_kernel", True), (1, "enc_site16_kernel", True), (3, "enc_kernel", True),
                                       (2, "enc_csite_kernel", False), (4, "enc_csite_kernel", False)):
            eng.set_encoder_variant(variant)
            got = eng.get_read_probability(X, km, off)
            assert eng.last_encoder_kernel == kernel, (variant, eng.last_encoder_kernel)
            if exact:
                assert np.array_equal(bits(got), bits(want)), (variant, np.flatnonzero(bits(got) != bits(want))[:5])
            else:                                                 # the 12-slot kernel: the reference test's bar
                assert np.allclose(got, want, rtol=1e-5, atol=1e-8), variant
            dev = eng.get_read_probability(*to_device(X, km, off))
            eng.sync()
            assert np.array_equal(bits(dev.cpu().numpy()), bits(got)), variant
    finally:
        eng.set_encoder_variant(0)
    X, km, off, want, _ = long_sites["with a bag of one"]
    got = eng.get_read_probability(X, km, off)
    assert eng.last_encoder_kernel == "enc_kernel"                # one bag below 16 reads: the per-lane walk
    assert np.array_equal(bits(got), bits(want)), np.flatnonzero(bits(got) != bits(want))[:5]


@pytest.mark.parametrize("name", ["bags of 16 and more", "with a bag of one"])
def test_read_representation_on_sites_past_2_16_reads(eng, long_sites, name):
    X, km, off, want_p, want_h = long_sites[name]
    dX, dkm, doff = to_device(X, km, off)
    h2, p = eng.get_read_representation(dX, dkm, doff, want_read_probs=True)
    eng.sync()
    assert eng.last_encoder_kernel == "enc_repr_kernel"
    h2, p = h2.cpu().numpy(), p.cpu().numpy()
    assert np.array_equal(bits(h2), bits(want_h)) and np.array_equal(bits(p), bits(want_p))
    h16 = eng.get_read_representation(dX, dkm, doff, dtype="float16")
    eng.sync()
    h16 = h16.cpu().numpy()
    assert h16.dtype == np.float16 and np.array_equal(h16.view(np.uint16), h2.astype(np.float16).view(np.uint16))
    host16 = eng.get_read_representation(X, km, off, dtype="float16")
    assert np.array_equal(host16.view(np.uint16), h16.view(np.uint16))


# ------------------------------------------------------------------ site expectation -----
@pytest.mark.parametrize("K", [20, 64])
@pytest.mark.parametrize("pointers, hint", [("host", False), ("device", False), ("device", True)])
def test_site_expectation_on_bags_past_2_16(eng, pointers, hint, K):
    off = D.csr(D.EXPECTATION_BAGS)
    p = D.RC.probs(np.random.default_rng(D.SEED), int(off[-1]))
    check_expectation(eng, p, off, K, pointers, hint, "deep")
    assert eng.last_pool_variant == "expected-wave"


# ------------------------------------------------------------------ the staging ring and the streaming job at a 1 MB slot -----
SLOT_READS = (1 << 20) // 36                                  # 29 127 reads of nine float32 in a slot of M6A_STAGE_MB=1


@pytest.fixture(scope="module")
def small_ring(weights):
    """an engine of its own whose ring is pinned at 1 MB per slot (the module's other engine may hold one of 24 MB)"""
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("M6A_STAGE_MB", "1")
        e = M6ANetEngine(weights=weights["hct116"], device=0)
        e.prepare_host_io()
    yield e
    e.close()


def ragged_job(seed, n_sites=40_000, extra=()):
    g = np.random.Generator(np.random.PCG64(seed))
    bags = g.integers(0, 61, size=n_sites)
    bags[g.random(n_sites) < 0.1] = 0
    bags[n_sites // 2:n_sites // 2 + 700] = 0                     # a long run of empty sites inside a chunk
    for at, n in extra:
        bags[at] = n
    return rand_sites(seed, bags)


def device_infer(e, X, km, off, T):
    out = e.infer(*to_device(X, km, off), T)
    e.sync()
    return [t.cpu().numpy() for t in out]


def check_infer(got, want):
    for g, w, name in zip(got, want, ("read_prob", "site_prob", "mod_ratio")):
        if g is not None:
            assert g.dtype == w.dtype and np.array_equal(g, w, equal_nan=True), name


def test_host_ring_many_chunks_at_a_small_slot(small_ring):
    e = small_ring
    X, km, off = ragged_job(31)
    R, S = int(off[-1]), off.size - 1
    assert R > 30 * SLOT_READS                                    # dozens of chunks: the three slots wrap many times
    want = device_infer(e, X, km, off, 40)
    assert np.isnan(want[1]).any() and np.isfinite(want[0]).all()
    check_infer(e.infer(X, km, off, 40), want)
    check_infer(e.infer(X, km, off, 40, want_read_probs=False), want)
    pX, pkm, poff = pinned_empty((R, 9), np.float32), pinned_empty((S, 3), np.uint8), pinned_empty(S + 1, np.int64)
    pX[:], pkm[:], poff[:] = X, km, off
    outs = (pinned_empty(R, np.float32), pinned_empty(S, np.float32), pinned_empty(S, np.float64))
    for o in outs:
        o[:] = -1
    check_infer(e.infer(pX, pkm, poff, 40, out=outs), want)


def test_host_ring_with_a_bag_larger_than_a_slot(small_ring):
    """bag_max > chunk_reads with the ring ready: staged_encode's plain copies"""
    e = small_ring
    X, km, off = ragged_job(32, extra=((12_345, 70_000),))
    assert int(np.diff(off).max()) > 2 * SLOT_READS
    want = device_infer(e, X, km, off, 40)
    check_infer(e.infer(X, km, off, 40), want)
    check_infer(e.infer(X, km, off, 40, want_read_probs=False), want)


def test_host_ring_with_offsets_larger_than_a_slot(small_ring):
    """100 000 sites of one or two reads: off and the k-mer ids together do not fit slot 0, so they travel on the context's stream"""
    e = small_ring
    bags = np.random.Generator(np.random.PCG64(33)).integers(1, 3, size=100_000)
    X, km, off = rand_sites(33, bags)
    assert off.nbytes + km.nbytes > 1 << 20 and int(off[-1]) > 4 * SLOT_READS
    want = device_infer(e, X, km, off, 40)
    check_infer(e.infer(X, km, off, 40), want)
    check_infer(e.infer(X, km, off, 40, want_read_probs=False), want)


def test_streaming_job_at_a_small_slot(small_ring):
    e = small_ring
    X, km, off = ragged_job(34)
    S = off.size - 1
    want = e.infer(X, km, off, 40)

    def stream(batch):
        e.job_begin(40)
        for s0 in range(0, S, batch):
            s1 = min(S, s0 + batch)
            e.job_feed(X[off[s0]:off[s1]], km[s0:s1], off[s0:s1 + 1] - off[s0])
        assert e.job_size() == (S, int(off[-1]))
        return e.job_end()
    check_infer(stream(999), want)
    bX, bkm, boff = rand_sites(35, [20, 70_000, 20])
    e.job_begin(40)
    try:
        with pytest.raises(_lib.M6AError, match=r"a site of 70000 reads does not fit a streaming chunk \(26844 reads\)") as err:
            e.job_feed(bX, bkm, boff)
        assert err.value.code == -6                               # M6A_EUNSUPPORTED
    finally:
        e.job_abort()
    check_infer(stream(10 ** 9), want)                            # the next job runs
