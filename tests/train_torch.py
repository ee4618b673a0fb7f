"""The yardstick of the training tests: the m6anet.toml model restated in a few lines of torch, run on the CPU in float32 (the
reference's arithmetic; tests/golden/train_step.npz pins it to the reference) and in float64, and the bar built from the two.

The bar, per case family and tensor t:
    E_ref(t) = the largest |torch float32 - torch float64| over the family's seeds
    E_hip(t) = the same with the kernels (or the NumPy statement) in place of torch float32
    required:  E_hip(t) <= 8 E_ref(t)
Absolute errors, so tensors whose exact gradient is zero (b1 always, E when all reads share their k-mers) need no special scale.
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


def statement_run(w, batches, zero_sites=(), **cfg):
    t = TS.Trainer(w, **cfg)
    losses, preds = [], []
    for X, kmers, y, bag in batches:
        loss, s = t.step(X, kmers, y, bag, zero_sites)
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
