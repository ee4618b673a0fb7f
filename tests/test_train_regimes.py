"""The yardstick of tests/test_gpu_train_regimes.py, held to its own conditions without a GPU (tables: tests/train_regimes.py).

The plain bar of tests/train_torch.py, E_hip <= 8 |torch float32 - torch float64|, is empty where s = fl(1 - prod (1 - p)) rounds
badly in float32; test_the_plain_bar_is_empty_there writes two such cases down.  The given-s bar replaces it there, and
test_given_s_cases_have_teeth holds every case the GPU file runs under it to train_torch.has_teeth: 8 E_ref(grad.t) is at most a
thousandth of the gradient, for every tensor but b1.  The cap is a condition, not a measurement: the worst figure measured when these
cases were chosen was 8 * 8e-6; a case that breaks the cap gets another seed, never a wider bar."""
import os

import numpy as np
import pytest
import torch

import train_regimes as TR
import train_statement as TS
import train_torch as TT
from m6anet_amd.engine import load_weights

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def bundled():
    d = np.load(os.path.join(GOLD, "bundled_inputs.npz"))
    return d["X"], d["site_kmers"], d["off"]


def test_the_tables_are_test_gpu_trains():
    import test_gpu_train as G
    import weight_families as WF
    assert TR.SEEDS == G.SEEDS and TR.HCT == G.HCT
    assert set(TR.WEIGHT_FAMILIES) <= set(WF.FAMILIES) and all(len(WF.SEEDS[f]) == 2 for f in TR.WEIGHT_FAMILIES)
    assert len(set(TR.GIVEN_S)) == len(TR.GIVEN_S) and set(TR.PLAIN_BAR_IS_EMPTY) <= set(TR.GIVEN_S)
    assert TR.seeds_for(8200, 1) == TR.SEEDS and TR.seeds_for(821, 20) == TR.SEEDS[:2]
    # what the shapes are there for (m6a_train.hip: queue_step, train_fwd2_kernel)
    assert [TR.chunking(B * bag) for B, bag in TR.BEYOND_ONE_TILE] == [(64, 129, 8), (64, 129, 48), (96, 172, 4), (64, 135, 4)]
    assert TR.chunking(8200) == (64, 129, 8) and TR.chunking(8192) == (32, 256, 32)
    assert [64 // bag for _, bag in TR.BAG_GEOMETRIES] == [1, 2, 3, 2, 21, 32]
    for B, bag in TR.BAG_GEOMETRIES:
        per_wave = 64 // bag
        assert per_wave == 1 or B % per_wave or (B, bag) == (9, 21), (B, bag)       # a short last wave; (9, 21): three full waves
    assert all(-(-B // (64 // bag)) % 4 for B, bag in [(6, 33), (9, 21), (9, 22)])   # a last block of fewer than 4 waves


def test_s_given_changes_the_loss_terms_and_dLds_only(bundled):
    from test_gpu_train import make_batch
    w = load_weights(TR.HCT)
    X, km, y, bag = make_batch(bundled, 6, 5, 3)
    loss, s, g, running = TS.step_gradient(w, X, km, y, bag)
    loss2, s2, g2, running2 = TS.step_gradient(w, X, km, y, bag, s_given=s)
    assert loss2 == loss and s2.tobytes() == s.tobytes() and g2.tobytes() == g.tobytes()     # given its own s: itself
    s32 = s.astype(np.float32)
    loss3, s3, g3, running3 = TS.step_gradient(w, X, km, y, bag, s_given=s32)
    assert s3.tobytes() == s.tobytes()                                                        # the returned s is the statement's own
    assert all(running3[k].tobytes() == running[k].tobytes() for k in running)
    sg = s32.astype(np.float64)
    assert loss3 == (-(y * np.log(sg) + (1.0 - y) * np.log(1.0 - sg))).mean()
    # the gradient is linear in dL/ds per site: site b alone given -> the change is that site's share, scaled
    one = s.copy()
    one[2] = 0.5 * s[2] + 0.25
    g4 = TS.step_gradient(w, X, km, y, bag, s_given=one)[2]
    ratio = ((one[2] - y[2]) / ((1 - one[2]) * one[2])) / ((s[2] - y[2]) / ((1 - s[2]) * s[2]))
    only2 = TS.step_gradient(w, X, km, np.where(np.arange(6) == 2, y, s), bag)[2]            # every other site: dL/ds = 0
    assert np.allclose(g4 - g, (ratio - 1.0) * only2, rtol=1e-9, atol=1e-15)
    # s exactly 0 and exactly 1: the clamps of torch.nn.BCELoss, and nothing is NaN
    edge = s32.copy()
    edge[0], edge[1] = 0.0, 1.0                                                               # y[0] = 0, y[1] = 1
    y2 = y.copy()
    y2[0], y2[1] = 1.0, 0.0
    loss5, _, g5, _ = TS.step_gradient(w, X, km, y2, bag, s_given=edge)
    assert np.isfinite(loss5) and np.isfinite(g5).all() and loss5 > 200.0 / 6
    t = TS.Trainer(w)
    assert t.step(X, km, y, bag, s_given=s32)[0] == loss3 and t.grad.tobytes() == g3.tobytes()


@pytest.mark.parametrize("kind,B,bag", TR.GIVEN_S)
def test_given_s_cases_have_teeth(bundled, kind, B, bag):
    worst = {}
    for w, batch in TR.cases(bundled, kind, B, bag):
        rel = TT.has_teeth(w, batch)
        worst = {t: max(r, worst.get(t, 0.0)) for t, r in rel.items()}
    print(TR.name(kind, B, bag), "E_ref / max|grad64|:", " ".join("%s %.1e" % kv for kv in worst.items()))


@pytest.mark.parametrize("kind,B,bag", TR.PLAIN_BAR_IS_EMPTY)
def test_the_plain_bar_is_empty_there(bundled, kind, B, bag):
    """Under the plain bar these cases let a gradient that is wrong by more than a thousandth of its size pass (by all of it, at
    500x1: 0.9 .. 1.0 was measured); under the given-s bar they have teeth (above)."""
    for w, batch in TR.cases(bundled, kind, B, bag):
        f32, f64 = TT.run(w, [batch], torch.float32), TT.run(w, [batch], torch.float64)
        scale = {t: float(np.abs(f64["grad"][TS.SLICES[t][0]]).max()) for t in TT.GRAD_TENSORS}
        rel = TT.relative_grad_errors(TT.errors(f32, f64), scale)
        print(TR.name(kind, B, bag), "plain E_ref / max|grad64|: %.2e" % max(rel.values()))
        assert max(rel.values()) > TT.TEETH_CAP, rel
