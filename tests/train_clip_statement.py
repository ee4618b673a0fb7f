"""tests/train_statement.py with gradient clipping between the gradient and Adam, as include/m6a.h states it (m6a_train_set_clip):

  total = sqrt(sum g^2) over the 7 697 trainable floats;  coef = min(1, max_norm / (total + 1e-6));  g <- coef g
  (torch.nn.utils.clip_grad_norm_(params, max_norm) with the 2-norm), then Adam: g += weight_decay theta, m, v, theta.

max_norm = 0 is no clipping, the library's default; the norm of every step is recorded either way.
"""
import numpy as np

import train_statement as TS


def clip(g, max_norm):
    """-> (the clipped gradient in blob order, total): the running-statistic slots of g are zeros and stay zeros."""
    total = float(np.sqrt(np.sum(g[TS.trainable_mask()] ** 2)))
    coef = min(1.0, max_norm / (total + 1e-6))
    return g * coef, total


class Trainer(TS.Trainer):
    """The state a m6a_trainer holds, in float64, with m6a_train_set_clip's max_norm."""

    def __init__(self, weights, max_norm=0.0, **cfg):
        super().__init__(weights, **cfg)
        self.max_norm, self.norm = float(max_norm), None

    def step(self, X, kmers, y, bag, zero_sites=()):
        loss, s, g, running = TS.step_gradient(self.w, X, kmers, y, bag, zero_sites)
        tr = TS.trainable_mask()
        self.norm = float(np.sqrt(np.sum(g[tr] ** 2)))
        if self.max_norm > 0:
            g, _ = clip(g, self.max_norm)
        self.grad = g
        for k, val in running.items():
            self.w[TS.SLICES[k][0]] = val
        b1, b2 = self.betas
        self.t += 1
        gd = g[tr] + self.weight_decay * self.w[tr]
        self.m[tr] = b1 * self.m[tr] + (1 - b1) * gd
        self.v[tr] = b2 * self.v[tr] + (1 - b2) * gd * gd
        self.w[tr] -= self.lr / (1 - b1 ** self.t) * self.m[tr] / (np.sqrt(self.v[tr]) / np.sqrt(1 - b2 ** self.t) + self.eps)
        return loss, s
