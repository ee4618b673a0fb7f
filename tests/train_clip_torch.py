"""The yardstick of the clipping tests: tests/train_torch.py's restated model with torch.nn.utils.clip_grad_norm_ between backward()
and step(), as the reference's train_one_epoch applies its clip_grad, in float32 and float64; the statement's run; and the cases.

The bar is train_torch.hold's, E_hip <= 8 E_ref per tensor, with one more judged quantity: "norm", the total norm
clip_grad_norm_ returns (Trainer.last_norm() here), the largest absolute difference over the steps.

Cases: batches by the recipe and seeds of test_gpu_train.py.  max_norm comes from the float64 statement's norm T of the first step:
0.25 T clips, 4 T does not.  Two conditions, checked from the statement alone and never met by a wider bar (a case that breaks one
gets another seed): every float64 site probability is <= 1 - 1e-3 (test_gpu_train.condition), and in every step the float64 norm is
>= 2 max_norm (clipped cases) or <= 0.5 max_norm (unclipped ones), so that float32 and float64 cannot decide the min differently.
"""
import os

import numpy as np
import torch

import train_clip_statement as CS
import train_torch as TT

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SEEDS = (11, 12, 13, 14)                                                       # test_gpu_train.SEEDS
SHAPES = [(1, 20), (3, 20), (13, 20), (256, 20), (7, 5), (5, 64)]
N_STEPS = 3


def bundled():
    d = np.load(os.path.join(GOLD, "bundled_inputs.npz"))
    return d["X"], d["site_kmers"], d["off"]


def make_batch(bundled, B, bag, seed, kmers=None):
    """test_gpu_train.make_batch, restated so that this helper imports no test module; test_train_clip_host.py holds the two equal."""
    X, km, _ = bundled
    g = np.random.Generator(np.random.PCG64(seed))
    rows = g.permutation(X.shape[0])[np.arange(B * bag) % X.shape[0]]
    sites = g.permutation(km.shape[0])[np.arange(B) % km.shape[0]]
    y = (g.random(B) < 0.5).astype(np.float32)
    if B > 1:
        y[0], y[1] = 0.0, 1.0
    k = km[sites] if kmers is None else np.broadcast_to(np.asarray(kmers, np.uint8), (B, 3))
    return np.ascontiguousarray(X[rows]), np.ascontiguousarray(k, np.uint8), y, bag


def case_batches(bundled, B, bag, s, n_steps=N_STEPS):
    """The batches of seed s: test_step_shapes' batch of that seed, stepped on n_steps times (as test_train_statement.py steps on one
    batch).  From one batch to another the norm moves by a factor of up to 4.7 at these sizes, more than the factor 2 the second
    condition leaves; on one batch it moves by less than 1.4 over three steps."""
    return [make_batch(bundled, B, bag, 1000 * B + 10 * bag + s)] * n_steps


def run(w, batches, dtype, max_norm, lr=4e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0):
    """train_torch.run with the clip.  -> its dictionary and 'norm' [n]: what clip_grad_norm_ returned in every step."""
    m = TT.Restated(w, dtype).train()
    opt = torch.optim.Adam(m.parameters(), lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
    crit = torch.nn.BCELoss()
    losses, preds, norms = [], [], []
    for X, kmers, y, bag in batches:
        opt.zero_grad()
        s = m(torch.tensor(np.asarray(X), dtype=dtype), torch.tensor(np.asarray(kmers).astype(np.int64)), bag)
        loss = crit(s, torch.tensor(np.asarray(y), dtype=dtype))
        loss.backward()
        norms.append(float(torch.nn.utils.clip_grad_norm_(m.parameters(), max_norm)))
        opt.step()
        losses.append(loss.item() if dtype == torch.float64 else np.float32(loss.item()))
        preds.append(s.detach().numpy().copy())
    return {"loss": np.asarray(losses), "y_pred": preds, "grad": m.blob(grads=True), "blob": m.blob(), "norm": np.asarray(norms, np.float64)}


def statement_run(w, batches, max_norm=0.0, zero_sites=(), **cfg):
    t = CS.Trainer(w, max_norm=max_norm, **cfg)
    losses, preds, norms = [], [], []
    for X, kmers, y, bag in batches:
        loss, s = t.step(X, kmers, y, bag, zero_sites)
        losses.append(loss)
        preds.append(s)
        norms.append(t.norm)
    return {"loss": np.asarray(losses), "y_pred": preds, "grad": t.grad.copy(), "blob": t.w.copy(), "norm": np.asarray(norms, np.float64)}


def errors(got, want):
    e = TT.errors(got, want)
    e["norm"] = float(np.abs(np.asarray(got["norm"], np.float64) - np.asarray(want["norm"], np.float64)).max())
    return e


def first_norm(w, batches, **cfg):
    """T: the float64 statement's gradient norm of the first step."""
    return float(statement_run(w, batches[:1], **cfg)["norm"][0])


def conditions(w, batches, max_norm, clipped, **cfg):
    """Asserts both conditions of a case from the float64 statement."""
    r = statement_run(w, batches, max_norm=max_norm, **cfg)
    for p in r["y_pred"]:
        assert p.max() <= 1 - 1e-3, p.max()
    for n in r["norm"]:
        assert (n >= 2 * max_norm) if clipped else (n <= 0.5 * max_norm), (n, max_norm, clipped)
    return r
