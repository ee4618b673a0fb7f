"""tests/train_statement.py (one training step in NumPy float64) against the reference: tests/golden/train_step.npz holds three Adam
steps of the reference's MILModel on one batch (tests/golden/make_train_golden.py).  The torch restatement of tests/train_torch.py
must BE the reference -- its float32 run equals the fixture's first step to the bit, or to one float32 ulp where the BLAS under torch
cuts the 160 x 15 product differently -- and then serves as the yardstick of the bar (train_torch.py) for the statement here and
for the kernels in test_gpu_train.py.

Which of the two held where the fixture was made: to the bit (loss and y_pred of all three steps) with torch on ONE thread, as
make_train_golden.py runs it; on eight threads torch's own reductions are cut differently and the same comparison is off by 2-3
ulp, so the runs here are made on one thread."""
import os

import numpy as np
import pytest
import torch

import train_statement as TS
import train_torch as TT
from m6anet_amd.engine import load_weights

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def fx():
    g = np.load(os.path.join(GOLD, "train_step.npz"))
    w = load_weights("HCT116_RNA002")
    batch = (g["X"].reshape(-1, 9), g["kmer"], g["y"], 20)
    threads = torch.get_num_threads()
    torch.set_num_threads(1)                                                    # as the fixture was made
    runs = {n: {"f32": TT.run(w, [batch] * n, torch.float32), "f64": TT.run(w, [batch] * n, torch.float64),
                "stmt": TT.statement_run(w, [batch] * n)} for n in (1, 3)}
    torch.set_num_threads(threads)
    return g, w, runs


def ulps(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return int(np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64)).max())


def test_restatement_is_the_reference(fx):
    g, _, runs = fx
    r = runs[3]["f32"]
    d_loss, d_pred = ulps(r["loss"][0], g["loss"][0]), ulps(r["y_pred"][0], g["y_pred"][0])
    print("restatement vs fixture, step 1: loss %d ulp, y_pred %d ulp (%s)" % (d_loss, d_pred, "to the bit" if d_loss + d_pred == 0 else "one ulp"))
    assert d_loss <= 1 and d_pred <= 1
    # the fixture's later tensors against the same restatement, under the bar's own measure
    e_ref = TT.errors(runs[1]["f32"], runs[1]["f64"])
    fixture1 = {"loss": g["loss"][:1], "y_pred": [g["y_pred"][0]], "grad": g["grad1"].astype(np.float64), "blob": g["blob1"].astype(np.float64)}
    TT.hold("fixture step 1", e_ref, TT.errors(fixture1, runs[1]["f64"]), bar=2.0)


def test_statement_reproduces_the_fixture(fx):
    g, _, runs = fx
    for n in (1, 3):
        e_ref = TT.errors(runs[n]["f32"], runs[n]["f64"])
        TT.hold("statement %d step%s" % (n, "s" * (n > 1)), e_ref, TT.errors(runs[n]["stmt"], runs[n]["f64"]))
    # and against the stored numbers themselves: the statement is as close to the fixture as float64 torch is
    s1, s3 = runs[1]["stmt"], runs[3]["stmt"]
    got = {"loss": g["loss"], "y_pred": list(g["y_pred"]), "grad": g["grad1"].astype(np.float64), "blob": g["blob3"].astype(np.float64)}
    want = {"loss": s3["loss"], "y_pred": s3["y_pred"], "grad": s1["grad"], "blob": s3["blob"]}
    e_ref = TT.errors(runs[3]["f32"], runs[3]["f64"])
    e_ref.update({k: v for k, v in TT.errors(runs[1]["f32"], runs[1]["f64"]).items() if k.startswith("grad.")})
    TT.hold("fixture vs statement", e_ref, TT.errors(got, want), bar=2.0)


def test_statement_properties():
    w = load_weights("HCT116_RNA002").astype(np.float64)
    g = np.random.Generator(np.random.PCG64(5))
    B, bag = 3, 4
    X, km, y = g.standard_normal((B * bag, 9)), g.integers(0, 66, (B, 3)), np.array([0.0, 1.0, 1.0])
    loss, s, grad, running = TS.step_gradient(w, X, km, y, bag)
    assert grad[TS.SLICES["running_mean"][0]].max() == 0 and grad[TS.SLICES["running_var"][0]].max() == 0
    assert np.abs(grad[TS.SLICES["b1"][0]]).max() < 1e-15                        # batch norm removes b1 from the loss
    # a central difference on a few floats of every trainable tensor
    for name in TS.TRAINABLE:
        sl = TS.SLICES[name][0]
        for e in {sl.start, (sl.start + sl.stop) // 2, sl.stop - 1}:
            h = 1e-6
            wp, wm = w.copy(), w.copy()
            wp[e] += h
            wm[e] -= h
            num = (TS.step_gradient(wp, X, km, y, bag)[0] - TS.step_gradient(wm, X, km, y, bag)[0]) / (2 * h)
            assert abs(num - grad[e]) <= 1e-6 * max(1.0, abs(grad[e])) + 1e-8, (name, e, num, grad[e])
    # a saturated read: the site's term is 100 (y = 0), its gradient exactly zero, nothing is NaN
    X2 = X.copy()
    X2[0] *= 1e4
    if TS.step_gradient(w, X2, km, y, bag)[1][0] == 1.0:
        loss2, s2, grad2, _ = TS.step_gradient(w, X2, km, y, bag)
        assert np.isfinite(grad2).all() and np.isfinite(loss2)
        assert np.array_equal(grad2, TS.step_gradient(w, X2, km, y, bag, zero_sites=(0,))[2])
