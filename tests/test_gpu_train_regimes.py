"""The training kernels (m6anet_amd/csrc/m6a_train.hip) where tests/test_gpu_train.py does not reach (tables: tests/train_regimes.py;
their conditions, without a GPU: tests/test_train_regimes.py).

1. Where float32 loses the site probability.  s = fl(1 - prod (1 - p)) is one float32 rounding that torch makes and the kernels make
   by specification.  Where a labelled site has s near 0 (bags of 1 or 2 reads) or near 1 (a fresh blob at 20 reads, the state every
   run starts in; bags of 63 and 64 reads) that rounding alone moves torch float32's gradient by 1e-2 .. 1 of itself, and the plain
   bar E_hip <= 8 |torch float32 - torch float64| passes anything.  Those cases run under the given-s bar of tests/train_torch.py:
   each subject against the float64 statement evaluated at the site probabilities the subject itself produced, y_pred against the
   statement's own, the same hold() at the same 8.  Single steps.
2. Batches beyond 8 192 reads, where a chunk of train_fwd1_kernel / train_bwd1_kernel is more than one 32-read tile: the tile loops
   run again over xs / dhs / dzs and go on accumulating; last chunks of 4 and 8 reads and of a full tile and 16 reads; an epoch
   whose chunk goes 64 -> 64 -> 32 reads within one call.
3. The bag layouts of train_fwd2_kernel (64 / bag whole bags per wave) besides 20, 1, 5 and 64 reads: 33, 32, 21, 22, 3 and 2.
4. One trainer over changing shapes: scratch grown after use, bag and chunk changed between steps.
5. Weights other than HCT116: tests/weight_families.py's fresh, trained_like, perturbed, gamma_signs (gamma < 0, gamma = 0: cg = 0,
   dz1 = 0, y1 = beta; dead units at beta = -100), large and big_embedding blobs, under the given-s bar, so no saturation condition.

Every E_ref / E_hip is printed before it is judged and, with M6A_TRAIN_PARITY_JSON set, written to that file
(profiles/r27_train_regimes_parity.json is one such run)."""
import os

import numpy as np
import pytest
import torch

import train_regimes as TR
import train_statement as TS
import train_torch as TT
from m6anet_amd.engine import M6ANetEngine, load_weights, train_sample
from test_gpu_train import HCT, condition, epoch_inputs, family, hip_run, make_batch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    e = M6ANetEngine(pretrained_model=HCT)
    yield e
    e.close()


@pytest.fixture(scope="module")
def bundled():
    d = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bundled_inputs.npz"))
    return d["X"], d["site_kmers"], d["off"]


@pytest.mark.parametrize("kind,B,bag", TR.GIVEN_S)
def test_step_under_the_given_s_bar(eng, bundled, kind, B, bag):
    e_ref, e_hip = [], []
    for w, batch in TR.cases(bundled, kind, B, bag):
        f32 = TT.run(w, [batch], torch.float32)
        TT.has_teeth(w, batch, f32)
        got = hip_run(eng, w, [batch])
        assert all(np.isfinite(got[k]).all() for k in ("loss", "grad", "blob")) and np.isfinite(got["y_pred"][0]).all()
        assert np.abs(got["grad"]).max() > 0
        e_ref.append(TT.given_s_errors(w, batch, f32))
        e_hip.append(TT.given_s_errors(w, batch, got))
    TT.hold(TR.name(kind, B, bag), TT.pooled(e_ref), TT.pooled(e_hip))


def plain_family(eng, bundled, label, shapes_per_case, seeds):
    """HCT116 under the plain bar with condition(): one list of batches (of shapes_per_case) per seed."""
    w = load_weights(HCT)
    lists = [[make_batch(bundled, B, bag, TR.batch_seed(B, bag, s)) for B, bag in shapes_per_case] for s in seeds]
    for batches in lists:
        condition(w, batches)
    family(eng, label, w, lists)
    return w, lists


@pytest.mark.parametrize("B,bag", TR.BEYOND_ONE_TILE)
def test_step_beyond_one_tile_per_chunk(eng, bundled, B, bag):
    assert TR.chunking(B * bag)[0] > 32
    plain_family(eng, bundled, "step %dx%d" % (B, bag), [(B, bag)], TR.seeds_for(B, bag))


@pytest.mark.parametrize("B,bag", TR.BAG_GEOMETRIES)
def test_step_bag_geometries(eng, bundled, B, bag):
    plain_family(eng, bundled, "step %dx%d" % (B, bag), [(B, bag)], TR.seeds_for(B, bag))


def test_one_trainer_over_changing_shapes(eng, bundled):
    """(3, 20), (412, 20), (7, 5), (6, 33) on one trainer: the scratch grows after use, bag and chunk change between steps, and a
    stale row of wpart or part would be folded into the next step's gradient.  Twice, with the same bits."""
    w, lists = plain_family(eng, bundled, "changing shapes", TR.CHANGING_SHAPES, TR.SEEDS[:2])
    a, b = hip_run(eng, w, lists[0]), hip_run(eng, w, lists[0])
    for k in ("loss", "grad", "blob"):
        assert a[k].tobytes() == b[k].tobytes(), k
    assert all(p.tobytes() == q.tobytes() for p, q in zip(a["y_pred"], b["y_pred"]))
    # and the last step is the step a trainer takes that never saw the larger shapes: from the state before it, the same bits
    tr = eng.trainer(w)
    for X, km, y, bag in lists[0][:-1]:
        tr.step(X, km, y, bag)
    blob, st = tr.weights(), tr.optimizer_state()
    tr.close()
    small = eng.trainer(blob)
    small.load_optimizer_state(st)
    loss, pred = small.step(*lists[0][-1])
    assert np.float32(loss).tobytes() == a["loss"][-1].tobytes() and pred.tobytes() == a["y_pred"][-1].tobytes()
    assert small.grads().tobytes() == a["grad"].tobytes() and small.weights().tobytes() == a["blob"].tobytes()
    small.close()


def test_epoch_beyond_one_tile_per_chunk_equals_its_steps_bit_for_bit(eng, bundled):
    """Steps of 412, 412 and 76 sites of 20 reads in one call: the chunk goes 64 -> 64 -> 32 reads, the kernels read through ridx / sidx."""
    X, km, off, y, order = epoch_inputs(bundled)
    order = np.ascontiguousarray(np.tile(order, 7)[:900])
    bs, bag, seed, w = 412, 20, 77, load_weights(HCT)
    assert [TR.chunking(n * bag)[0] for n in (412, 412, 76)] == [64, 64, 32]
    idx = train_sample(off, order, bag, seed)
    assert np.array_equal(idx[:40 * bag], TS.sample(off, order[:40], bag, seed))
    tr = eng.trainer(w)
    s0 = tr.stats()
    loss, pred = tr.epoch(X, km, off, y, order, bs, bag, seed)
    s1 = tr.stats()
    ew, eg = tr.weights(), tr.grads()
    tr.close()
    assert loss.shape == (3,) and pred.shape == (900,) and s1["n_steps"] - s0["n_steps"] == 3
    tr = eng.trainer(w)
    for k in range(3):
        o = order[k * bs:(k + 1) * bs]
        l, p = tr.step(X[idx[k * bs * bag:(k + 1) * bs * bag]], km[o], y[o], bag)
        assert np.float32(l).tobytes() == loss[k].tobytes(), k
        assert p.tobytes() == pred[k * bs:(k + 1) * bs].tobytes(), k
    assert tr.weights().tobytes() == ew.tobytes() and tr.grads().tobytes() == eg.tobytes()
    tr.close()
    assert np.isfinite(loss).all() and np.isfinite(ew).all() and np.abs(eg).max() > 0
