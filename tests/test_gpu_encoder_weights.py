"""The encoder kernels on weights other than the four shipped checkpoints: the seeded families of tests/weight_families.py (fresh,
trained-like, perturbed, negative / zero gammas with dead and always-on units, running_var down to 0, large activations, large
embeddings, one activation just below the 2^64 limit) and `trained`, a blob the training kernels produce here -- at the smallest bag
layouts that still reach the tile and site edges (weight_families.LAYOUTS).

Two rules, as everywhere in this suite:
  * the 16-slot kernels (enc_site16_kernel, enc_kernel, enc_repr_kernel; variants 0, 1, 3; m6a_bag_forward, m6a_infer, m6a_validate)
    give the oracle's BITS, host arrays and device tensors alike, and what is pooled from them is the oracle's pooling of those bits;
  * the 12-slot kernel (enc_csite_kernel; variants 2, 4) sums layer 1 in another order and promises no bits: it is judged against the
    float64 statement (tests/encoder_statement.py) relative to what the reference's own order achieves,
        u(q) = max over reads of |q - p64| / (1e-8 + 1e-5 |p64|), pooled over the family's seeds, layouts A and B and both variants
        E_ref = u(oracle),  E_hip = u(kernel),  required E_hip <= 8 E_ref          (train_torch.BAR, the project's standing allowance)
    Every E_ref / E_hip / ratio is printed before it is judged and, with M6A_ENCODER_PARITY_JSON set, written to that file
    (profiles/r25_encoder_weights_parity.json is one such run).

One engine per blob, made and closed in its test.  tests/test_encoder_statement.py holds the same (family, seed, layout) triples to the
conditions that make these checks mean something (finite, unsaturated probabilities; the oracle well inside the bar of float64)."""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import encoder_statement as ES                                   # noqa: E402
import weight_families as WF                                     # noqa: E402
from train_torch import BAR                                      # noqa: E402
from m6anet_amd.constants import DEFAULT_READ_THRESHOLD          # noqa: E402
from m6anet_amd.engine import M6ANetEngine, init_weights         # noqa: E402

THR = np.float32(DEFAULT_READ_THRESHOLD)
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIGURES = {}                                                     # family -> {"E_ref", "E_hip", "ratio"}: everything hold() judged


@pytest.fixture(scope="module")
def orc():
    from oracle import m6a_oracle
    m6a_oracle.build()
    return m6a_oracle


@pytest.fixture(scope="module")
def hct():
    e = M6ANetEngine(pretrained_model="HCT116_RNA002")
    yield e
    e.close()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def to_device(*arrays):
    import torch
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0") for a in arrays)


def kernel_of(variant, bags):
    if variant in (2, 4):
        return "enc_csite_kernel"
    return "enc_site16_kernel" if variant != 3 and min(bags) >= 16 else "enc_kernel"


def read_probs(e, variant, X, km, off, device):
    """get_read_probability under one encoder variant, host arrays or device tensors -> (float32 [R], the kernel launched)"""
    e.set_encoder_variant(variant)
    try:
        if device:
            got = e.get_read_probability(*to_device(X, km, off))
            e.sync()
            got = got.cpu().numpy()
        else:
            got = e.get_read_probability(X, km, off)
        return got, e.last_encoder_kernel
    finally:
        e.set_encoder_variant(0)


def hold(family, e_ref, e_hip):
    """train_torch.hold's sibling for one figure per family: print, record, then assert E_hip <= BAR * E_ref."""
    ratio = e_hip / e_ref if e_ref > 0 else (0.0 if e_hip == 0 else float("inf"))
    FIGURES[family] = {"E_ref": e_ref, "E_hip": e_hip, "ratio": ratio}
    print("%-14s 12-slot kernel against float64, in units of the bar rtol 1e-5, atol 1e-8:  E_ref %.4f  E_hip %.4f  ratio %.2f"
          % (family, e_ref, e_hip, ratio))
    path = os.environ.get("M6A_ENCODER_PARITY_JSON")
    if path:
        with open(path, "w") as f:
            json.dump(FIGURES, f, indent=1, sort_keys=True)
    assert e_hip <= BAR * e_ref, (family, e_ref, e_hip, ratio)


def sixteen_slot_checks(e, orc, w, family, seed, bad):
    """Every path that promises the oracle's bits, on one engine.  Mismatches are appended to `bad`, so that one does not hide the next."""
    def same(got, want, what):
        got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
        if got.shape != want.shape or not np.array_equal(got.view(np.uint8), want.view(np.uint8)):
            bad.append((family, seed, what, int(np.count_nonzero(got != want)) if got.shape == want.shape else "shape"))

    want_p, want_h = {}, {}
    for layout in ("A", "B", "C"):
        X, km, off = WF.inputs(family, seed, layout)
        want_p[layout], want_h[layout], _ = orc.encode_layers(w, X, km, off)
        # ---- get_read_probability: variants 0, 1 and 3 where every bag has 16 reads, the automatic choice elsewhere
        for variant in ((0, 1, 3) if layout != "C" else (0,)):
            for device in (False, True):
                got, kernel = read_probs(e, variant, X, km, off, device)
                assert kernel == kernel_of(variant, WF.LAYOUTS[layout]) and e.last_encoder_variant == "general16"
                same(bits(got), bits(want_p[layout]), "read_prob %s variant %d %s" % (layout, variant, "device" if device else "host"))
        # ---- the read representation, float32 and float16
        if layout in ("A", "C"):
            for device in (False, True):
                tag = "%s %s" % (layout, "device" if device else "host")
                args = to_device(X, km, off) if device else (X, km, off)
                h32, p = e.get_read_representation(*args, want_read_probs=True)
                assert e.last_encoder_kernel == "enc_repr_kernel"
                h16 = e.get_read_representation(*args, dtype="float16")
                assert e.last_encoder_kernel == "enc_repr_kernel<true>"
                if device:
                    e.sync()
                    h32, p, h16 = (t.cpu().numpy() for t in (h32, p, h16))
                assert h16.dtype == np.float16
                same(bits(h32), bits(want_h[layout]), "repr float32 " + tag)
                same(bits(p), bits(want_p[layout]), "repr read_prob " + tag)
                with np.errstate(over="ignore"):
                    want16 = np.float32(want_h[layout]).astype(np.float16)
                same(h16.view(np.uint16), want16.view(np.uint16), "repr float16 " + tag)
    # ---- m6a_bag_forward: 5 bags of 20 (enc_site16_kernel) and 7 bags of 5 (enc_kernel)
    for layout, bag in (("F20", 20), ("F5", 5)):
        X, km, off = WF.inputs(family, seed, layout)
        want = orc.bag_noisy_or(orc.encode_reads(w, X, km, off), bag)
        got = e.forward(X.reshape(-1, bag, 9), km, bag=bag)
        assert e.last_encoder_kernel == ("enc_site16_kernel" if bag >= 16 else "enc_kernel")
        same(bits(got), bits(want), "forward " + layout)
        tgot = e.forward(*to_device(X.reshape(-1, bag, 9), km), bag=bag)
        e.sync()
        same(bits(tgot.cpu().numpy()), bits(want), "forward %s device" % layout)
    # ---- m6a_infer on A, 7 iterations: the oracle's read probabilities, and the oracle's pooling of them
    X, km, off = WF.inputs(family, seed, "A")
    rp, site, mod = e.infer(X, km, off, 7)
    want_site, want_mod = orc.site_pool(want_p["A"], off, 7, THR)
    same(bits(rp), bits(want_p["A"]), "infer read_prob")
    same(bits(site), bits(want_site), "infer site_prob")
    same(np.asarray(mod, np.float64), want_mod, "infer mod_ratio")
    # ---- m6a_validate, 2 passes
    X, km, off = WF.inputs(family, seed, "V")
    y, avg, rp = e.validate_forward(X, km, off, n_iterations=2, seed=5, want_read_probs=True)
    p = orc.encode_reads(w, X, km, off)
    want_y, want_avg = orc.validate(p, off, 2, seed=5)
    same(bits(rp), bits(p), "validate read_prob")
    same(bits(y), bits(want_y), "validate y_pred")
    same(bits(avg), bits(want_avg), "validate y_pred_avg")


def twelve_slot_figures(e, orc, w, family, seed):
    """(u(oracle), u(kernel)) over layouts A and B and variants 2 and 4, against the float64 statement."""
    u_ref = u_hip = 0.0
    for layout in ("A", "B"):
        X, km, off = WF.inputs(family, seed, layout)
        p64, _, _ = ES.forward(w, X, km, off)
        u_ref = max(u_ref, float(WF.used(orc.encode_reads(w, X, km, off), p64).max()))
        for variant in (2, 4):
            got, kernel = read_probs(e, variant, X, km, off, device=(variant == 4))
            assert kernel == "enc_csite_kernel" and e.last_encoder_variant == "csite12"
            assert np.isfinite(got).all()
            u_hip = max(u_hip, float(WF.used(got, p64).max()))
    return u_ref, u_hip


def trained_blob(hct, seed):
    """Family `trained`: what the training kernels make of init_weights(seed) in 5 steps on batches of the reference's bundled data."""
    from test_gpu_train import make_batch
    d = np.load(os.path.join(GOLD, "bundled_inputs.npz"))
    bundled = (d["X"], d["site_kmers"], d["off"])
    tr = hct.trainer(init_weights(seed))
    try:
        for k in range(5):
            tr.step(*make_batch(bundled, 32, 20, 500 + 10 * seed + k))
        return tr.weights()
    finally:
        tr.close()


@pytest.mark.parametrize("family", WF.FAMILIES + ("trained",))
def test_family(orc, hct, family):
    bad, u_ref, u_hip = [], 0.0, 0.0
    for seed in (WF.TRAINED_SEEDS if family == "trained" else WF.SEEDS[family]):
        if family == "trained":
            w = trained_blob(hct, seed)
            assert np.isfinite(w).all() and not np.array_equal(w, init_weights(seed))
            for layout in WF.LAYOUTS:                            # the conditions test_encoder_statement.py asserts for the others
                WF.conditions(w, *WF.inputs(family, seed, layout), orc)
        else:
            w = WF.blob(family, seed)
        e = M6ANetEngine(weights=w)
        try:
            sixteen_slot_checks(e, orc, w, family, seed, bad)
            r, h = twelve_slot_figures(e, orc, w, family, seed)
        finally:
            e.close()
        u_ref, u_hip = max(u_ref, r), max(u_hip, h)
    try:
        hold(family, u_ref, u_hip)
    except AssertionError as exc:                                # reported beside the bit mismatches, not instead of them
        bad.append(("12-slot kernel beyond %g x E_ref" % BAR,) + exc.args)
    assert not bad, bad


def test_nan_weight(orc):
    """W1[7][3] = NaN, what a diverged run writes: NaN exactly where the oracle has NaN, whichever kernel; what stays finite (nothing,
    with this blob: unit 7 feeds every layer-2 output) follows its kernel's rule."""
    w = WF.blob("nan_weight", 0)
    X, km, off = WF.inputs("nan_weight", 0, "A")
    want = orc.encode_reads(w, X, km, off)
    p64, _, _ = ES.forward(w, X, km, off)
    nan = np.isnan(want)
    assert nan.any()
    e = M6ANetEngine(weights=w)
    try:
        for variant in (0, 1, 2, 3):
            got, kernel = read_probs(e, variant, X, km, off, device=False)
            assert kernel == kernel_of(variant, WF.LAYOUTS["A"])
            assert np.array_equal(np.isnan(got), nan), variant
            if variant == 2:
                assert (~nan).sum() == 0 or WF.used(got[~nan], p64[~nan]).max() <= BAR * WF.used(want[~nan], p64[~nan]).max()
            else:
                assert np.array_equal(bits(got)[~nan], bits(want)[~nan]), variant
    finally:
        e.close()


def test_context_health_after_the_families(orc, weights):
    """No blob leaves anything behind: after the engines above have come and gone, a fresh engine on the HCT116 checkpoint still gives
    the oracle's bits, every variant."""
    X, km, off = WF.inputs("fresh", 1, "A")
    want = orc.encode_reads(weights["hct116"], X, km, off)
    e = M6ANetEngine(weights=weights["hct116"])
    try:
        for variant in (0, 1, 3):
            for device in (False, True):
                got, kernel = read_probs(e, variant, X, km, off, device)
                assert kernel == kernel_of(variant, WF.LAYOUTS["A"])
                assert np.array_equal(bits(got), bits(want)), (variant, device)
        p64, _, _ = ES.forward(weights["hct116"], X, km, off)
        fast, kernel = read_probs(e, 2, X, km, off, False)
        assert kernel == "enc_csite_kernel" and WF.used(fast, p64).max() <= BAR * WF.used(want, p64).max()
    finally:
        e.close()
