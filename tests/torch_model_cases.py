"""The cases and the yardstick of the MILModel tests (m6anet_amd/torch_model.py): tests/test_torch_model_host.py checks their
conditions without a GPU, tests/test_gpu_torch_model.py runs the module on them, and both read them from here.

The bar under a given upstream gradient g = dL/ds, per family and tensor t (train_torch.hold at train_torch.BAR = 8):
    E_ref(t) = the largest |Restated float32 - Restated float64| over the family's seeds, both from s.backward(g)
    E_hip(t) = the same with the module's .grad in place of Restated float32
Its condition, teeth(): 8 E_ref(grad.t) <= 1e-3 max |grad64.t| for every tensor but b1 (train_torch.TEETH_CAP, GRAD_TENSORS).  The
rounding of s that empties the plain BCE bar on some of these cases (train_regimes.PLAIN_BAR_IS_EMPTY) is no part of a backward from
a given dL/ds, so one bar serves every family here.

g = PCG64(7000 + seed).standard_normal(B) / B, rounded to float32; batches are train_clip_torch.make_batch's with train_regimes'
seed rule; the weights are train_regimes.weights'.
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

import train_clip_torch as CT
import train_regimes as TR
import train_statement as TS
import train_torch as TT

# (B, bag): the plain case | 12, 21, 32 and 64 bags per wave with a short last wave | idle lanes | more than one 32-read tile a chunk
SHAPES = [(3, 20), (13, 20), (7, 5), (45, 3), (70, 2), (64, 1), (6, 33), (412, 20)]
FAMILIES = [("HCT116", B, bag) for B, bag in SHAPES]
FAMILIES += [(kind, B, bag) for kind in ("init",) + TR.WEIGHT_FAMILIES for B, bag in TR.WEIGHT_SHAPES]
LOSS_SHAPES = [(13, 20), (256, 20)]                       # HCT116, where test_gpu_train.condition() holds


def name(kind, B, bag):
    return "given g: %s %dx%d" % (kind, B, bag)


def upstream(B, seed):
    return (np.random.Generator(np.random.PCG64(7000 + seed)).standard_normal(B) / B).astype(np.float32)


def weighted_bce(s, y):
    """The reference's weighted loss, restated: a site's term weighs the number of sites of the OTHER class in the batch, and the
    mean runs over the batch.  A batch of one class has no such weights: ValueError."""
    n_pos, n_neg = int((y == 1).sum()), int((y == 0).sum())
    if n_pos == 0 or n_neg == 0 or n_pos + n_neg != y.numel():
        raise ValueError("the weighted loss needs labels 0 and 1, both present in the batch")
    weights = torch.where(y == 1, float(n_neg), float(n_pos)).to(s.dtype)
    return (F.binary_cross_entropy(s, y.to(s.dtype), reduction="none") * weights).mean()


LOSSES = {"bce": lambda s, y: F.binary_cross_entropy(s, y.to(s.dtype)), "weighted": weighted_bce}


def restated(w, batch, dtype, g=None, loss=None):
    """One forward and backward of train_torch.Restated in training mode: under the upstream gradient g, or through LOSSES[loss].
    -> {'s', 'grad' (blob order, float64), 'running' (300 floats), 'loss'}"""
    X, kmers, y, bag = batch
    m = TT.Restated(w, dtype).train()
    s = m(torch.tensor(np.asarray(X), dtype=dtype), torch.tensor(np.asarray(kmers).astype(np.int64)), bag)
    value = None
    if g is not None:
        s.backward(torch.tensor(np.asarray(g), dtype=dtype))
    else:
        value = LOSSES[loss](s, torch.tensor(np.asarray(y), dtype=dtype))
        value.backward()
    running = np.concatenate([m.running_mean.numpy(), m.running_var.numpy()])
    return {"s": s.detach().numpy().copy(), "grad": m.blob(grads=True), "running": running, "loss": None if value is None else value.item()}


def grad_errors(got, want):
    """Largest absolute difference per trainable tensor between two gradients in blob order."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return {"grad." + t: float(np.abs(got[TS.SLICES[t][0]] - want[TS.SLICES[t][0]]).max()) for t in TS.TRAINABLE}


def teeth(e_ref, grad64):
    """8 E_ref(grad.t) <= 1e-3 max |grad64.t| for every tensor but b1 -> the relative errors; AssertionError with them otherwise."""
    rel = {t: e_ref["grad." + t] / float(np.abs(grad64[TS.SLICES[t][0]]).max()) for t in TT.GRAD_TENSORS}
    assert all(TT.BAR * r <= TT.TEETH_CAP for r in rel.values()), rel
    return rel


@functools.lru_cache(maxsize=None)
def family_cases(kind, B, bag):
    """-> [{'w', 'batch', 'g', 'f32', 'f64', 'e_ref'}], one per seed; computed once a process and not changed by the tests."""
    out = []
    for seed in TR.seeds_for(B, bag):
        w, batch = TR.weights(kind, seed), CT.make_batch(CT.bundled(), B, bag, TR.batch_seed(B, bag, seed))
        g = upstream(B, seed)
        f32, f64 = restated(w, batch, torch.float32, g=g), restated(w, batch, torch.float64, g=g)
        out.append({"w": w, "batch": batch, "g": g, "f32": f32, "f64": f64, "e_ref": grad_errors(f32["grad"], f64["grad"])})
    return out


@functools.lru_cache(maxsize=None)
def loss_cases(loss, B, bag):
    """HCT116 under LOSSES[loss] -> [{'w', 'batch', 'f32', 'f64', 'e_ref'}], one per seed."""
    out = []
    for seed in TR.SEEDS:
        w, batch = TR.weights("HCT116", seed), CT.make_batch(CT.bundled(), B, bag, TR.batch_seed(B, bag, seed))
        f32, f64 = restated(w, batch, torch.float32, loss=loss), restated(w, batch, torch.float64, loss=loss)
        out.append({"w": w, "batch": batch, "f32": f32, "f64": f64, "e_ref": grad_errors(f32["grad"], f64["grad"])})
    return out
