"""The read representation on the GPU (include/m6a.h: m6a_read_representation; enc_repr_kernel in m6anet_amd/csrc/m6a_kernels.hip;
M6ANetEngine.get_read_representation; `inference --read_representation`): layer 2 after its ReLU, 32 floats per read.

Every comparison is of BITS: against tests/golden/reference_layers.npz, the reference's own get_read_representation on the sites
test_reference_at_scale.py::test_oracle_layers_are_the_references_bits regenerates, and against oracle.m6a_oracle.encode_layers, which
that test pins to the same capture.  The one exception is a row of X that holds NaN: there the NaN POSITIONS are compared (a NaN's
payload is not part of any statement) and the bits everywhere else."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from m6anet_amd import _lib, synthetic                # noqa: E402

MODELS = ("hct116", "arabidopsis", "hek293t_glori", "hek293t_m6ace")
SHAPES = {"uniform": (1_000_000, 20), "ragged": (1_000_000, (50, 500))}      # test_reference_at_scale.py SHAPES
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATA = os.path.join(REPO, "tests", "golden", "ref_tests_data")               # the directory bundled_inputs.npz was loaded from
SENTINEL = np.float32(-12345.678)                                            # no relu output is negative


@pytest.fixture(scope="module")
def orc():
    from oracle import m6a_oracle
    m6a_oracle.build()
    return m6a_oracle


@pytest.fixture(scope="module")
def engines(weights):
    from m6anet_amd.engine import M6ANetEngine
    made = {name: M6ANetEngine(weights=weights[name]) for name in MODELS}
    yield made
    for e in made.values():
        e.close()


@pytest.fixture(scope="module")
def eng(engines):
    return engines["hct116"]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def rand_sites(seed, bags):
    g = np.random.Generator(np.random.PCG64(seed))
    n = np.asarray(bags, np.int64)
    off = np.concatenate([[0], np.cumsum(n)]).astype(np.int64)
    X = np.clip(g.standard_normal((int(off[-1]), 9)), -6, 6).astype(np.float32)
    km = g.integers(0, 66, size=(len(n), 3)).astype(np.uint8)
    return X, km, off


def to_device(*arrays):
    import torch
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0") for a in arrays)


def device_repr(e, X, km, off, **kw):
    """The device-pointer form: tensors in, tensors out, read after the context's stream has drained."""
    out = e.get_read_representation(*to_device(X, km, off), **kw)
    e.sync()
    return tuple(o.cpu().numpy() for o in out) if isinstance(out, tuple) else out.cpu().numpy()


# ------------------------------------------------------------------ the reference's bits ------------------------------------
@pytest.mark.parametrize("tag", list(SHAPES))
def test_repr_is_the_references_bits(golden, engines, tag):
    """uniform: 64 sites x 20 reads = 1 280 reads (40 whole tiles).  ragged: 8 sites of 68..449 reads, 2 304 reads."""
    L = golden("reference_layers.npz")
    n, bag = SHAPES[tag]
    keep = int(L[f"{tag}_sites"])
    d = synthetic.make_sites(n, bag, seed=20250328, prefix_sites=keep)
    R = int(d["off"][keep])
    X, km, off = d["X"][:R], d["site_kmers"][:keep], d["off"][:keep + 1]
    assert R == {"uniform": 1280, "ragged": 2304}[tag]
    for name in MODELS:
        e = engines[name]
        h2, p = device_repr(e, X, km, off, want_read_probs=True)
        assert h2.shape == (R, 32) and h2.dtype == np.float32
        assert np.array_equal(bits(h2), bits(L[f"{tag}_{name}_h2"])), (tag, name)
        assert e.last_encoder_kernel == "enc_repr_kernel"
        assert np.array_equal(bits(p), bits(e.get_read_probability(X, km, off))), (tag, name)
        assert np.array_equal(bits(device_repr(e, X, km, off)), bits(h2)), (tag, name)          # without read_prob: the same store


# ------------------------------------------------------------------ edges, against the oracle --------------------------------
def share_cases():
    """One tile fewer and one tile more than a whole workgroup's share.  launch_repr (m6a_api.hip), as launch_encode: max_waves =
    8 x CUs, tiles_per_wave = ceil(n_tiles / max_waves), a workgroup = 4 waves, so its share is 4 x tiles_per_wave tiles.
    tiles_per_wave = 1 (up to max_waves tiles): 3 and 5 tiles.  tiles_per_wave = 2 (the wave's tile loop runs twice; share 8):
    max_waves + 7 and max_waves + 9 tiles -- 2 055 and 2 057 tiles on the 256 CUs of an MI355X, the last workgroup holding 7 tiles
    and 1 tile.  Each with a partial last tile (- 5 reads)."""
    import torch
    max_waves = 8 * torch.cuda.get_device_properties(0).multi_processor_count
    return {"tpw1_share-1": 3 * 32 - 5, "tpw1_share+1": 5 * 32 - 5,
            "tpw2_share-1": (max_waves + 7) * 32 - 5, "tpw2_share+1": (max_waves + 9) * 32 - 5}


def bags_summing_to(total, bag=20):
    return [bag] * (total // bag) + ([total % bag] if total % bag else [])


EDGE_BAGS = {
    **{"reads_%d" % n: [n] for n in (1, 31, 32, 33, 63, 64, 65)},            # n_sites = 1 each
    "64_sites_of_1": [1] * 64,                                               # a tile spans 32 sites
    "bags_15": [15] * 9, "bags_16": [16] * 9, "bags_17": [17] * 9, "bags_15_16_17": [15, 16, 17] * 5,
    "one_site_5000": [5000],
    "empty_sites": [0, 5, 0, 0, 40, 0],
}


def check_against_oracle(orc, w, e, X, km, off):
    p, h, _ = orc.encode_layers(w, X, km, off)
    h2, p2 = device_repr(e, X, km, off, want_read_probs=True)
    assert np.array_equal(bits(h2), bits(h))
    assert np.array_equal(bits(p2), bits(e.get_read_probability(X, km, off)))
    return h2


@pytest.mark.parametrize("case", list(EDGE_BAGS))
def test_repr_edges_against_oracle(orc, weights, eng, case):
    X, km, off = rand_sites(sorted(EDGE_BAGS).index(case), EDGE_BAGS[case])
    check_against_oracle(orc, weights["hct116"], eng, X, km, off)


@pytest.mark.parametrize("case", ["tpw1_share-1", "tpw1_share+1", "tpw2_share-1", "tpw2_share+1"])
def test_repr_around_a_workgroups_share(orc, weights, eng, case):
    X, km, off = rand_sites(77, bags_summing_to(share_cases()[case]))
    check_against_oracle(orc, weights["hct116"], eng, X, km, off)


def test_repr_kmer_ids_0_and_65(orc, weights, eng):
    X, km, off = rand_sites(5, [20] * 6)
    km = np.array([[0, 65, 0], [65, 65, 65], [0, 0, 0], [65, 0, 1], [64, 65, 0], [0, 1, 65]], np.uint8)
    check_against_oracle(orc, weights["hct116"], eng, X, km, off)


def test_repr_nan_row(orc, weights, eng):
    """A NaN feature makes that read's representation NaN wherever the oracle's is (relu keeps NaN, as torch's does) and leaves
    every other read's bits alone: reads are columns of the tile."""
    X, km, off = rand_sites(6, [20, 7, 40])
    X[33, 4] = np.nan
    _, h, _ = orc.encode_layers(weights["hct116"], X, km, off)
    h2 = device_repr(eng, X, km, off)
    assert np.isnan(h[33]).any()
    assert np.array_equal(np.isnan(h2), np.isnan(h))
    ok = ~np.isnan(h)
    assert np.array_equal(bits(h2)[ok], bits(h)[ok])


# ------------------------------------------------------------------ no store past the end ------------------------------------
@pytest.mark.parametrize("n_reads", [1, 31, 32, 33, 63, 64, 65])
def test_repr_stores_nothing_outside_its_rows(orc, weights, eng, n_reads):
    """out= is a view into a larger buffer with 64 sentinel rows on both sides (the kernel's stores are guarded by r < n_reads:
    a partial last tile computes on a clamped read and must write nothing for it); the same for read_prob."""
    import torch
    X, km, off = rand_sites(100 + n_reads, [n_reads])
    pad = 64
    big = torch.full((n_reads + 2 * pad, 32), float(SENTINEL), dtype=torch.float32, device="cuda:0")
    big_p = torch.full((n_reads + 2 * pad,), float(SENTINEL), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    out = eng.get_read_representation(*to_device(X, km, off), out=(big[pad:pad + n_reads], big_p[pad:pad + n_reads]), want_read_probs=True)
    eng.sync()
    assert out[0].data_ptr() == big[pad:].data_ptr()
    got, got_p = big.cpu().numpy(), big_p.cpu().numpy()
    for a in (got, got_p):
        assert np.all(a[:pad] == SENTINEL) and np.all(a[pad + n_reads:] == SENTINEL)
    _, h, _ = orc.encode_layers(weights["hct116"], X, km, off)
    assert np.array_equal(bits(got[pad:pad + n_reads]), bits(h))
    assert not np.any(got_p[pad:pad + n_reads] == SENTINEL)


# ------------------------------------------------------------------ determinism, queueing, the selected encoder --------------
def test_repr_back_to_back_calls_agree(eng):
    X, km, off = rand_sites(8, [20] * 50 + [3, 1, 500])
    t = to_device(X, km, off)
    a = eng.get_read_representation(*t)
    b = eng.get_read_representation(*t)                                # queued behind the first, no sync between
    eng.sync()
    assert np.array_equal(bits(a.cpu().numpy()), bits(b.cpu().numpy()))


def test_repr_does_not_depend_on_the_selected_encoder(monkeypatch, weights, eng):
    """M6A_ENCODER=fast (read by m6a_create) sends get_read_probability of 20-read bags to the 12-slot kernel; the representation
    stays the reference arithmetic, and so does the probability that comes with it."""
    from m6anet_amd.engine import M6ANetEngine
    X, km, off = rand_sites(9, [20] * 40)
    want, want_p = device_repr(eng, X, km, off, want_read_probs=True)
    monkeypatch.setenv("M6A_ENCODER", "fast")
    fast = M6ANetEngine(weights=weights["hct116"])
    try:
        fast.get_read_probability(X, km, off)
        assert fast.last_encoder_kernel == "enc_csite_kernel"
        got, got_p = device_repr(fast, X, km, off, want_read_probs=True)
        assert fast.last_encoder_kernel == "enc_repr_kernel"
        fast.set_encoder_variant(2)                                    # m6a_set_encoder_variant: the 12-slot kernel, strict
        got2 = device_repr(fast, X, km, off)
    finally:
        fast.close()
    assert np.array_equal(bits(got), bits(want)) and np.array_equal(bits(got2), bits(want))
    assert np.array_equal(bits(got_p), bits(want_p))


# ------------------------------------------------------------------ refusals, each followed by a correct call ----------------
def test_repr_null_is_einval_and_the_context_goes_on(orc, weights, eng):
    import torch
    X, km, off = rand_sites(10, [20, 21])
    tX, tk, to = to_device(X, km, off)
    rp = torch.full((41,), float(SENTINEL), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    rc = eng._L.m6a_read_representation(eng._h, tX.data_ptr(), tk.data_ptr(), to.data_ptr(), 2, None, rp.data_ptr())
    assert rc == -1 and b"repr" in eng._L.m6a_last_error(eng._h)                      # M6A_EINVAL
    eng.sync()
    assert np.all(rp.cpu().numpy() == SENTINEL)                                        # nothing was launched
    rc = eng._L.m6a_read_representation(eng._h, tX.data_ptr(), tk.data_ptr(), to.data_ptr(), 0, None, None)
    assert rc == -1                                                                    # also with no sites
    check_against_oracle(orc, weights["hct116"], eng, X, km, off)


def test_repr_kmer_id_66_is_what_encode_reads_reports(orc, weights, eng):
    """k-mer id 66 is outside the 66-word vocabulary; whatever m6a_encode_reads says about it (return code, and the deferred code
    of the sync that follows), m6a_read_representation says the same -- its arguments and checks are that call's."""
    X, km, off = rand_sites(11, [20, 20, 20])
    bad = km.copy()
    bad[1, 2] = 66

    def outcome(call):
        try:
            call(*to_device(X, bad, off))
            eng.sync()
            return 0
        except _lib.M6AError as exc:
            return exc.code

    assert outcome(eng.get_read_representation) == outcome(eng.get_read_probability)
    check_against_oracle(orc, weights["hct116"], eng, X, km, off)


# ------------------------------------------------------------------ host pointers ---------------------------------------------
@pytest.mark.parametrize("bags", [[20, 20, 25], [5000]], ids=["65_reads", "5000_reads"])
def test_repr_host_pointers_give_the_device_forms_bits(eng, bags):
    X, km, off = rand_sites(12, bags)
    want, want_p = device_repr(eng, X, km, off, want_read_probs=True)
    got, got_p = eng.get_read_representation(X, km, off, want_read_probs=True)
    assert isinstance(got, np.ndarray) and got.shape == want.shape
    assert np.array_equal(bits(got), bits(want)) and np.array_equal(bits(got_p), bits(want_p))
    out = np.full((int(off[-1]) + 2, 32), SENTINEL, np.float32)
    assert eng.get_read_representation(X, km, off, out=out[1:-1]) is not None
    assert np.array_equal(bits(out[1:-1]), bits(want)) and np.all(out[0] == SENTINEL) and np.all(out[-1] == SENTINEL)


# ------------------------------------------------------------------ INTEGRATION.md, as written ------------------------------
def test_integration_section_as_written(golden, weights, monkeypatch):
    """INTEGRATION.md section 1a appended to section 1's stub, both executed verbatim: the reference's call shape -- a dictionary of
    per-READ tensors -- gives the golden representation's bits."""
    import re
    import torch
    monkeypatch.setenv("M6A_HIP_LIB", _lib.LIB_PATH)
    _lib.load()                                   # one HIP runtime per process (see _lib._preload_hip_runtime)
    blocks = re.findall(r"```python\n(.*?)```", open(os.path.join(REPO, "INTEGRATION.md")).read(), flags=re.S)
    stub = [b for b in blocks if "class HipModel" in b]
    section = [b for b in blocks if "def get_read_representation(model, x)" in b]
    assert len(stub) == 1 and len(section) == 1
    ns = {}
    exec(compile(stub[0], "INTEGRATION.md:hip_backend.py", "exec"), ns)
    exec(compile(section[0], "INTEGRATION.md:1a", "exec"), ns)
    from m6anet_amd.engine import state_dict_from_weights
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in state_dict_from_weights(weights["hct116"]).items()}
    model = ns["HipModel"](sd)
    L = golden("reference_layers.npz")
    keep = int(L["uniform_sites"])
    d = synthetic.make_sites(*SHAPES["uniform"], seed=20250328, prefix_sites=keep)
    R = int(d["off"][keep])
    kmers = np.repeat(d["site_kmers"][:keep].astype(np.int64), 20, axis=0)
    got = ns["get_read_representation"](model, {"X": torch.from_numpy(d["X"][:R]), "kmer": torch.from_numpy(kmers)})
    assert isinstance(got, torch.Tensor) and tuple(got.shape) == (R, 32)
    assert np.array_equal(bits(got.numpy()), bits(L["uniform_hct116_h2"]))
    ns["_L"].m6a_destroy(model._h)


def test_repr_host_pointers_in_two_chunks(eng):
    """The host-pointer form cuts the job at site boundaries into chunks of at most 2^20 reads (m6a_read_representation in m6a_api.hip):
    43 sites of 25 000 reads are a chunk of 41 sites and one of 2, whose rows land where the device form puts them."""
    X, km, off = rand_sites(13, [25_000] * 43)
    assert off[41] <= (1 << 20) < off[42]
    want, want_p = device_repr(eng, X, km, off, want_read_probs=True)
    got, got_p = eng.get_read_representation(X, km, off, want_read_probs=True)
    assert np.array_equal(bits(got), bits(want)) and np.array_equal(bits(got_p), bits(want_p))


# ------------------------------------------------------------------ the command ------------------------------------------------
def test_cli_read_representation(tmp_path, eng, monkeypatch):
    """`inference --read_representation` on the reference's bundled data: one row per data row of data.indiv_proba.csv, the rows the
    engine gives on the loaded batch (the default checkpoint is the `eng` fixture's), and both CSVs byte for byte those of a run without
    the flag."""
    from m6anet_amd.__main__ import main
    from m6anet_amd.constants import DEFAULT_MIN_READS, DEFAULT_PRETRAINED_MODEL, PRETRAINED_CONFIGS
    from m6anet_amd.data_utils import load_sites_native
    assert DEFAULT_PRETRAINED_MODEL.lower().startswith("hct116")
    outs = {}
    for tag, extra in (("plain", []), ("repr", ["--read_representation"])):
        outs[tag] = str(tmp_path / tag)
        main(["inference", "--input_dir", DATA, "--out_dir", outs[tag], "--n_processes", "1", "--num_iterations", "5"] + extra)
    for fn in ("data.site_proba.csv", "data.indiv_proba.csv"):
        assert open(os.path.join(outs["repr"], fn), "rb").read() == open(os.path.join(outs["plain"], fn), "rb").read(), fn
    assert sorted(os.listdir(outs["plain"])) == ["data.indiv_proba.csv", "data.site_proba.csv"]
    assert sorted(os.listdir(outs["repr"])) == ["data.indiv_proba.csv", "data.read_representation.npy", "data.site_proba.csv"]
    h = np.load(os.path.join(outs["repr"], "data.read_representation.npy"))
    n_rows = len(open(os.path.join(outs["repr"], "data.indiv_proba.csv")).read().splitlines()) - 1
    assert h.dtype == np.float32 and h.shape == (n_rows, 32)
    batch = load_sites_native([DATA], DEFAULT_MIN_READS, PRETRAINED_CONFIGS[DEFAULT_PRETRAINED_MODEL][2], n_threads=1)
    assert int(batch.off[-1]) == n_rows
    want = eng.get_read_representation(batch.X, batch.site_kmers, batch.off)
    assert np.array_equal(bits(h), bits(want))
    # the same file when it is written in many pieces (of 64 reads, or one site where a site is larger)
    from m6anet_amd.scripts import inference
    monkeypatch.setattr(inference, "REPR_PIECE_READS", 64)
    small = str(tmp_path / "pieces")
    main(["inference", "--input_dir", DATA, "--out_dir", small, "--n_processes", "1", "--num_iterations", "5", "--read_representation"])
    assert open(os.path.join(small, "data.read_representation.npy"), "rb").read() == \
        open(os.path.join(outs["repr"], "data.read_representation.npy"), "rb").read()
