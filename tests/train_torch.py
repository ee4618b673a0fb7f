"""The yardstick of the training tests: the m6anet.toml model restated in a few lines of torch, run on the CPU in float32 (the
reference's arithmetic; tests/golden/train_step.npz pins it to the reference) and in float64, and the bar built from the two.

The bar, per case family and tensor t:
    E_ref(t) = the largest |torch float32 - torch float64| over the family's seeds
    E_hip(t) = the same with the kernels (or the NumPy statement) in place of torch float32
    required:  E_hip(t) <= 8 E_ref(t)
Absolute errors, so tensors whose exact gradient is zero (b1 always, E when all reads share their k-mers) need no special scale.

That bar has teeth only while torch float32 is itself accurate.  One float32 rounding, s = fl(1 - prod (1 - p)), which torch makes and
the kernels make by specification (include/m6a.h), ruins it where a labelled site has s near 0 (bags of 1 or 2 reads: s rounds to a
few ulps of 1.0, or to exactly 0) or near 1 (a fresh blob at 20 reads: 1 - s is about 1e-6): there E_ref is 1e-2 .. 1 of the
gradient itself and 8 E_ref passes anything (tests/test_train_regimes.py writes two such cases down).  The given-s bar takes that
rounding out of the comparison, for a single step (trajectories part after one):
    E_ref(t) = |torch float32 - statement64(s_given = torch float32's y_pred)|
    E_hip(t) = |kernels       - statement64(s_given = the kernels' y_pred)|
    for y_pred itself: |s32 - s64| against the statement's own s, which s_given does not change
judged by the same hold() at the same 8.  Its condition, has_teeth(): 8 E_ref(grad.t) <= 1e-3 max |grad64.t|.
"""
import json
import os

import numpy as np
import torch
import torch.nn.functional as F

import train_statement as TS

BAR = 8.0


class Restated(torch.nn.Module):
    def __init__(self, w, dtype):
        super().__init__()
        for k, v in TS.unpack(np.asarray(w, np.float32)).items():
            t = torch.tensor(v, dtype=dtype)
            if k.startswith("running_"):
                self.register_buffer(k, t)
            else:
                setattr(self, k, torch.nn.Parameter(t))

    def forward(self, X, kmers, bag):
        emb = F.embedding(kmers.repeat_interleave(bag, dim=0).view(-1, 1), self.E).reshape(-1, 6)
        z = F.linear(torch.cat([X.view(-1, 9), emb], axis=1), self.W1, self.b1)
        a1 = F.relu(F.batch_norm(z, self.running_mean, self.running_var, self.gamma, self.beta, training=True, momentum=0.1, eps=1e-5))
        a2 = F.relu(F.linear(a1, self.W2, self.b2))
        p = torch.sigmoid(F.linear(a2, self.W3.view(1, 32), self.b3)).view(-1, bag)
        return 1 - torch.prod(1 - p, axis=1)

    def blob(self, grads=False):
        out = np.zeros(TS.N_FLOATS, np.float64)
        for k, (sl, _) in TS.SLICES.items():
            t = getattr(self, k)
            if grads:
                t = None if k.startswith("running_") else t.grad
            if t is not None:
                out[sl] = t.detach().numpy().astype(np.float64).ravel()
        return out


def run(w, batches, dtype, lr=4e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0):
    """batches: [(X, kmers, y, bag)], one Adam step each.  -> {'loss' [n], 'y_pred' [n][B], 'grad' (of the LAST step), 'blob'}"""
    m = Restated(w, dtype).train()
    opt = torch.optim.Adam(m.parameters(), lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
    crit = torch.nn.BCELoss()
    losses, preds = [], []
    for X, kmers, y, bag in batches:
        opt.zero_grad()
        s = m(torch.tensor(np.asarray(X), dtype=dtype), torch.tensor(np.asarray(kmers).astype(np.int64)), bag)
        loss = crit(s, torch.tensor(np.asarray(y), dtype=dtype))
        loss.backward()
        opt.step()
        losses.append(loss.item() if dtype == torch.float64 else np.float32(loss.item()))
        preds.append(s.detach().numpy().copy())
    return {"loss": np.asarray(losses), "y_pred": preds, "grad": m.blob(grads=True), "blob": m.blob()}


def statement_run(w, batches, zero_sites=(), s_given=None, **cfg):
    """s_given: one array of site probabilities per batch (train_statement.step_gradient), or None."""
    t = TS.Trainer(w, **cfg)
    losses, preds = [], []
    for k, (X, kmers, y, bag) in enumerate(batches):
        loss, s = t.step(X, kmers, y, bag, zero_sites, s_given=None if s_given is None else s_given[k])
        losses.append(loss)
        preds.append(s)
    return {"loss": np.asarray(losses), "y_pred": preds, "grad": t.grad.copy(), "blob": t.w.copy()}


def errors(got, want):
    """Largest absolute difference per tensor between two results of run(): loss, y_pred, grad.<tensor>, blob.<tensor>."""
    e = {"loss": float(np.abs(np.asarray(got["loss"], np.float64) - np.asarray(want["loss"], np.float64)).max()),
         "y_pred": max(float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max()) for a, b in zip(got["y_pred"], want["y_pred"]))}
    for k, (sl, _) in TS.SLICES.items():
        if not k.startswith("running_"):
            e["grad." + k] = float(np.abs(np.asarray(got["grad"], np.float64)[sl] - want["grad"][sl]).max())
        e["blob." + k] = float(np.abs(np.asarray(got["blob"], np.float64)[sl] - want["blob"][sl]).max())
    return e


def pooled(list_of_errors):
    return {k: max(e[k] for e in list_of_errors) for k in list_of_errors[0]}


# ---- the given-s bar ---------------------------------------------------------------------------------------------------------------
GRAD_TENSORS = [t for t in TS.TRAINABLE if t != "b1"]      # b1's exact gradient is 0: it has no scale to be small against
TEETH_CAP = 1e-3


def given_s_errors(w, batch, subject, **cfg):
    """The errors of one single-step result `subject` (a dictionary as run() returns it) against the float64 statement evaluated with
    the site probabilities the subject itself produced.  y_pred is judged against the statement's own float64 s."""
    assert len(subject["y_pred"]) == 1
    return errors(subject, statement_run(w, [batch], s_given=[subject["y_pred"][0]], **cfg))


def grad_scales(w, batch, s_given=None, **cfg):
    """max |grad64.t| per tensor of GRAD_TENSORS, of the float64 statement (at s_given, where given)."""
    g = statement_run(w, [batch], s_given=None if s_given is None else [s_given], **cfg)["grad"]
    return {t: float(np.abs(g[TS.SLICES[t][0]]).max()) for t in GRAD_TENSORS}


def relative_grad_errors(e_ref, scales):
    """E_ref(grad.t) / max |grad64.t| per tensor of GRAD_TENSORS."""
    return {t: e_ref["grad." + t] / scales[t] for t in GRAD_TENSORS}


def has_teeth(w, batch, f32=None, **cfg):
    """The condition of a given-s case, from torch float32 and the statement alone: 8 E_ref(grad.t) <= 1e-3 max |grad64.t| for every
    tensor but b1, so a gradient wrong by a thousandth of its size cannot pass, and not every site probability of torch float32 is
    exactly 0 or 1.  -> the relative errors; raises AssertionError with them otherwise.  A case that breaks it gets another seed."""
    f32 = run(w, [batch], torch.float32, **cfg) if f32 is None else f32
    s32 = np.asarray(f32["y_pred"][0])
    assert not np.all((s32 == 0.0) | (s32 == 1.0)), "every site probability is exactly 0 or 1 in float32"
    rel = relative_grad_errors(given_s_errors(w, batch, f32, **cfg), grad_scales(w, batch, s32, **cfg))
    assert all(BAR * r <= TEETH_CAP for r in rel.values()), rel
    return rel


FIGURES = {}          # family -> {tensor: {"E_ref", "E_hip", "ratio"}}: everything hold() judged in this process


def hold(family, e_ref, e_hip, bar=BAR):
    """Prints every figure, records it, then asserts E_hip <= bar * E_ref for every tensor."""
    rows, bad = {}, []
    for k in e_ref:
        ratio = e_hip[k] / e_ref[k] if e_ref[k] > 0 else (0.0 if e_hip[k] == 0 else float("inf"))
        rows[k] = {"E_ref": e_ref[k], "E_hip": e_hip[k], "ratio": ratio}
        print("%-28s %-18s E_ref %.3e  E_hip %.3e  ratio %.2f" % (family, k, e_ref[k], e_hip[k], ratio))
        if not e_hip[k] <= bar * e_ref[k]:
            bad.append((k, e_ref[k], e_hip[k], ratio))
    FIGURES[family] = rows
    path = os.environ.get("M6A_TRAIN_PARITY_JSON")
    if path:
        with open(path, "w") as f:
            json.dump(FIGURES, f, indent=1, sort_keys=True)
    assert not bad, (family, bad)
