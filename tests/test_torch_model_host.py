"""MILModel (m6anet_amd/torch_model.py) without a GPU: the conditions of the bar tests/test_gpu_torch_model.py holds it to, from torch
float32, torch float64 and train_torch.Restated alone (tests/torch_model_cases.py); the restated weighted loss; and what the module
is before any kernel runs -- its import, its state_dict, its refusals."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import torch_model_cases as MC
import train_regimes as TR
import train_torch as TT
from m6anet_amd import _lib
from m6anet_amd.engine import STATE_DICT_KEYS, load_weights, state_dict_from_weights

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("kind,B,bag", MC.FAMILIES)
def test_the_given_g_bar_has_teeth(kind, B, bag):
    """8 E_ref(grad.t) <= 1e-3 max |grad64.t| for every tensor but b1, in every case of every family the GPU test judges."""
    worst = 0.0
    for case in MC.family_cases(kind, B, bag):
        assert np.abs(case["g"]).max() > 0 and case["g"].dtype == np.float32
        rel = MC.teeth(case["e_ref"], case["f64"]["grad"])
        worst = max(worst, max(rel.values()))
    print("%-28s worst E_ref / max |grad64| = %.2e" % (MC.name(kind, B, bag), worst))


def test_the_two_cases_the_plain_bar_cannot_judge_are_judged_here():
    assert set(TR.PLAIN_BAR_IS_EMPTY) == {("init", 64, 20), ("HCT116", 500, 1)}
    for kind, B, bag in TR.PLAIN_BAR_IS_EMPTY:
        for case in MC.family_cases(kind, B, bag)[:2]:
            MC.teeth(case["e_ref"], case["f64"]["grad"])


def test_weighted_loss_weights_are_the_other_class_count_and_the_mean_is_over_the_batch():
    s = torch.tensor([0.9, 0.2, 0.6, 0.3, 0.7], dtype=torch.float64)
    y = torch.tensor([1.0, 0.0, 1.0, 0.0, 1.0], dtype=torch.float64)             # 3 of class 1, 2 of class 0
    terms = -(y * torch.log(s) + (1 - y) * torch.log(1 - s))
    want = (terms * torch.tensor([2.0, 3.0, 2.0, 3.0, 2.0], dtype=torch.float64)).sum() / 5
    assert abs(MC.weighted_bce(s, y).item() - want.item()) <= 1e-15
    # equal counts: n / 2 times the plain loss
    y2 = torch.tensor([1.0, 0.0, 1.0, 0.0], dtype=torch.float64)
    assert abs(MC.weighted_bce(s[:4], y2).item() - 2 * MC.LOSSES["bce"](s[:4], y2).item()) <= 1e-15
    for one_class in (torch.ones(5, dtype=torch.float64), torch.zeros(5, dtype=torch.float64)):
        with pytest.raises(ValueError, match="both present"):
            MC.weighted_bce(s, one_class)


@pytest.mark.parametrize("loss", sorted(MC.LOSSES))
@pytest.mark.parametrize("B,bag", MC.LOSS_SHAPES)
def test_the_bar_has_teeth_under_the_losses(loss, B, bag):
    for case in MC.loss_cases(loss, B, bag):
        y = case["batch"][2]
        assert 0 < y.sum() < len(y)                                              # both classes
        assert TT.statement_run(case["w"], [case["batch"]])["y_pred"][0].max() <= 1 - 1e-3       # test_gpu_train.condition()
        MC.teeth(case["e_ref"], case["f64"]["grad"])
        assert np.isfinite(case["f32"]["loss"]) and abs(case["f32"]["loss"] - case["f64"]["loss"]) <= 1e-5 * abs(case["f64"]["loss"])


def test_import_m6anet_amd_does_not_import_torch():
    code = ("import sys; import m6anet_amd, m6anet_amd.engine, m6anet_amd._lib; "
            "assert 'torch' not in sys.modules and 'm6anet_amd.torch_model' not in sys.modules")
    subprocess.run([sys.executable, "-c", code], check=True, cwd=REPO)


def test_entry_points_are_declared_and_bound():
    h = open(os.path.join(REPO, "include", "m6a.h")).read()
    L = _lib.load()
    vp = C.c_void_p
    want = {"m6a_train_set_weights": [vp, vp], "m6a_train_forward": [vp, vp, vp, C.c_int64, C.c_int, C.c_int, vp, C.POINTER(C.c_int64)],
            "m6a_train_running_stats": [vp, vp], "m6a_train_backward": [vp, C.c_int64, vp, vp]}
    for fn, argtypes in want.items():
        assert re.search(r"\bint\s+%s\s*\(" % fn, h) and fn in _lib.SYMBOLS
        assert getattr(L, fn).argtypes == argtypes and getattr(L, fn).restype is C.c_int
        nothing = [0 if a in (C.c_int64, C.c_int) else None for a in argtypes]
        assert getattr(L, fn)(*nothing) == -1                                    # a null trainer is M6A_EINVAL, not a crash
    assert "Not built: the weighted loss" in h                                   # the fused step's text stays


def test_state_dict_has_the_reference_keys_and_shapes_and_round_trips():
    from m6anet_amd.torch_model import MILModel
    w = load_weights("HCT116_RNA002")
    m = MILModel(w, device="cpu")
    sd = m.state_dict()
    want = state_dict_from_weights(w)
    assert list(sd) == list(want)
    for (key, shape) in STATE_DICT_KEYS:
        assert tuple(sd[key].shape) == shape and sd[key].dtype == torch.float32
        assert np.array_equal(sd[key].numpy(), want[key])
    tracked = "read_level_encoder.3.layers.1.num_batches_tracked"
    assert sd[tracked].dtype == torch.int64 and sd[tracked].shape == () and int(sd[tracked]) == 0
    assert m.blob().tobytes() == w.tobytes()
    assert [n for n, _ in m.named_parameters()] == [k for k, _ in STATE_DICT_KEYS if "running_" not in k]
    assert all(p.is_leaf and p.requires_grad for p in m.parameters()) and sum(p.numel() for p in m.parameters()) == 7697
    # a reference checkpoint's dictionary goes in, and the blob follows
    other = MILModel(None, device="cpu")
    assert other.blob().tobytes() != w.tobytes()
    ref_sd = {k: torch.tensor(v) for k, v in state_dict_from_weights(w, num_batches_tracked=5).items()}
    other.load_state_dict(ref_sd)
    assert other.blob().tobytes() == w.tobytes() and int(other.state_dict()[tracked]) == 5
    assert MILModel("HCT116_RNA002", device="cpu").blob().tobytes() == w.tobytes()


def test_the_blob_follows_every_way_a_parameter_changes():
    from m6anet_amd.torch_model import MILModel
    m = MILModel("HCT116_RNA002", device="cpu")
    w = m.blob()
    opt = torch.optim.SGD(m.parameters(), lr=0.5)
    for p in m.parameters():
        p.grad = torch.ones_like(p)
    opt.step()                                                                   # in place
    d = m.blob() - w
    trainable = np.ones(7997, bool)
    trainable[2832:3132] = False
    assert np.allclose(d[trainable], -0.5, atol=1e-6) and not d[~trainable].any()
    e = m.read_level_encoder._modules["1"].embedding_layer.weight
    e.data = torch.full((66, 2), 3.0)                                            # moved away: packed again at the next look
    assert np.array_equal(m.blob()[:132], np.full(132, 3.0, np.float32))
    with torch.no_grad():
        e.add_(1.0)                                                              # ... and aliases the blob again
    assert np.array_equal(m.blob()[:132], np.full(132, 4.0, np.float32))
    import copy
    m2 = copy.deepcopy(m)
    assert m2.blob().tobytes() == m.blob().tobytes()
    with torch.no_grad():
        next(m2.parameters()).zero_()
    assert m2.blob()[:132].max() == 0 and m.blob()[:132].min() == 4.0           # the copy has its own storage


def test_refusals_before_any_kernel():
    from m6anet_amd.torch_model import MILModel
    with pytest.raises(ValueError, match="7997 floats"):
        MILModel(np.zeros(100, np.float32), device="cpu")
    with pytest.raises(ValueError, match="not a pretrained model"):
        MILModel("no_such_model", device="cpu")
    with pytest.raises(ValueError, match="bag must be in 1..64"):
        MILModel(None, device="cpu", bag=65)
    m = MILModel(None, device="cpu")
    X, km = torch.zeros(4, 20, 9), torch.zeros(4, 3, dtype=torch.int64)
    with pytest.raises(TypeError, match="needs the module on a GPU"):
        m.forward_bags(X, km)
    with pytest.raises(TypeError, match="torch tensor"):
        m.forward_bags(X.numpy(), km)
    with pytest.raises(TypeError, match="torch tensor"):
        m({"X": X, "kmer": km.numpy()})
    with pytest.raises(ValueError, match=r"\[B, bag, 3\]"):
        m({"X": X, "kmer": km})
    with pytest.raises(ValueError, match=r"\[B, bag, 3\]"):
        m({"X": X, "kmer": torch.zeros(4, 19, 3, dtype=torch.int64)})
