"""One training step of the m6anet.toml model, stated once in NumPy float64: forward, gradient, Adam, and the read draw.
include/m6a.h (m6a_train_step) states the same thing; m6anet_amd/csrc/m6a_train.hip computes it in float32.

Blob layout (include/m6a.h): E[66][2] | W1[150][15] | b1 | gamma | beta | running_mean | running_var | W2[32][150] | b2[32] | W3[32] | b3.

  x    = [X (9) | E[k0] | E[k1] | E[k2]]                                  15 values per read, N = B * bag reads
  z1   = W1 x + b1
  mu   = mean(z1), var = biased variance over the N reads, xhat = (z1 - mu) / sqrt(var + 1e-5), y1 = gamma xhat + beta
         running_mean <- 0.9 running_mean + 0.1 mu;  running_var <- 0.9 running_var + 0.1 var N / (N - 1)
  a1   = relu(y1), a2 = relu(W2 a1 + b2), p = sigmoid(W3 a2 + b3)
  s_b  = 1 - prod_k (1 - p_bk)
  loss = mean_b -(y log s + (1 - y) log(1 - s)), both logs clamped at -100          (torch.nn.BCELoss)
  dL/ds = (s - y) / max((1 - s) s, 1e-12) / B;   ds/dp_k = prod_{j != k} (1 - p_j) from prefix and suffix products
  Adam (torch.optim.Adam): g += weight_decay theta; m, v; theta -= lr / (1 - beta1^t) m / (sqrt(v) / sqrt(1 - beta2^t) + eps)
"""
import numpy as np

N_FLOATS = 7997
SLICES = {}
_o = 0
for _name, _shape in (("E", (66, 2)), ("W1", (150, 15)), ("b1", (150,)), ("gamma", (150,)), ("beta", (150,)), ("running_mean", (150,)),
                      ("running_var", (150,)), ("W2", (32, 150)), ("b2", (32,)), ("W3", (32,)), ("b3", (1,))):
    _n = int(np.prod(_shape))
    SLICES[_name] = (slice(_o, _o + _n), _shape)
    _o += _n
assert _o == N_FLOATS
TENSORS = list(SLICES)
TRAINABLE = [t for t in TENSORS if not t.startswith("running_")]
BN_EPS, MOMENTUM = 1e-5, 0.1


def unpack(w):
    w = np.asarray(w)
    return {k: w[sl].reshape(shape) for k, (sl, shape) in SLICES.items()}


def trainable_mask():
    m = np.ones(N_FLOATS, bool)
    for k in ("running_mean", "running_var"):
        m[SLICES[k][0]] = False
    return m


def step_gradient(w, X, kmers, y, bag, zero_sites=(), logits_only=False, s_given=None):
    """-> (loss, y_pred [B], gradient in blob order with zeros in the running-statistic slots, the blob's new running statistics).
    zero_sites: sites whose dL/dlogit is set to zero (what a site with a saturated read contributes in float32).
    logits_only: return the N logits instead.
    s_given [B]: the site probabilities a float32 subject produced.  The loss terms and dL/ds are evaluated at np.float64(s_given), so
    1 - s is the exact float64 of the float32 value and the one rounding s = fl(1 - prod) is the subject's and the statement's alike;
    p, the prefix and suffix products, the backward pass and the returned y_pred stay the statement's own."""
    p = unpack(np.asarray(w, np.float64))
    X = np.asarray(X, np.float64).reshape(-1, 9)
    kmers = np.asarray(kmers).reshape(-1, 3).astype(np.int64)
    y = np.asarray(y, np.float64).ravel()
    B, N = len(y), len(y) * bag
    assert X.shape[0] == N and kmers.shape[0] == B and N >= 2
    kr = np.repeat(kmers, bag, axis=0)                                          # [N, 3]
    x = np.concatenate([X, p["E"][kr].reshape(N, 6)], axis=1)                   # [N, 15]
    z1 = x @ p["W1"].T + p["b1"]
    mu, var = z1.mean(axis=0), z1.var(axis=0)
    istd = 1.0 / np.sqrt(var + BN_EPS)
    xhat = (z1 - mu) * istd
    y1 = p["gamma"] * xhat + p["beta"]
    a1 = np.maximum(y1, 0.0)
    h2 = a1 @ p["W2"].T + p["b2"]
    a2 = np.maximum(h2, 0.0)
    logit = a2 @ p["W3"] + p["b3"][0]
    if logits_only:
        return logit
    with np.errstate(over="ignore"):
        pr = 1.0 / (1.0 + np.exp(-logit))
    q = (1.0 - pr).reshape(B, bag)
    pre, suf = np.ones((B, bag)), np.ones((B, bag))
    for k in range(1, bag):
        pre[:, k] = pre[:, k - 1] * q[:, k - 1]
    for k in range(bag - 2, -1, -1):
        suf[:, k] = suf[:, k + 1] * q[:, k + 1]
    s = 1.0 - pre[:, -1] * q[:, -1]
    sl = s if s_given is None else np.asarray(s_given).astype(np.float64).reshape(B)
    with np.errstate(divide="ignore"):
        terms = -(y * np.maximum(np.log(sl), -100.0) + (1.0 - y) * np.maximum(np.log(1.0 - sl), -100.0))
    loss = terms.mean()
    dLds = (sl - y) / np.maximum((1.0 - sl) * sl, 1e-12) / B
    dlogit = (dLds[:, None] * pre * suf).reshape(N) * pr * (1.0 - pr)
    for b in zero_sites:
        dlogit[b * bag:(b + 1) * bag] = 0.0
    g = np.zeros(N_FLOATS)
    G = unpack(g)                                                               # views into g
    G["W3"][:] = dlogit @ a2
    G["b3"][0] = dlogit.sum()
    dh2 = dlogit[:, None] * p["W3"][None, :] * (h2 > 0)
    G["W2"][:] = dh2.T @ a1
    G["b2"][:] = dh2.sum(axis=0)
    dy1 = (dh2 @ p["W2"]) * (y1 > 0)
    G["gamma"][:] = (dy1 * xhat).sum(axis=0)
    G["beta"][:] = dy1.sum(axis=0)
    dz1 = p["gamma"] * istd / N * (N * dy1 - G["beta"] - xhat * G["gamma"])
    G["W1"][:] = dz1.T @ x
    G["b1"][:] = dz1.sum(axis=0)
    dxe = (dz1 @ p["W1"])[:, 9:].reshape(N, 3, 2)
    np.add.at(G["E"], kr, dxe)
    running = {"running_mean": (1 - MOMENTUM) * p["running_mean"] + MOMENTUM * mu,
               "running_var": (1 - MOMENTUM) * p["running_var"] + MOMENTUM * var * N / (N - 1)}
    return loss, s, g, running


class Trainer:
    """The state a m6a_trainer holds, in float64."""

    def __init__(self, weights, lr=4e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0):
        self.w = np.array(weights, np.float64)
        assert self.w.size == N_FLOATS
        self.m, self.v, self.t = np.zeros(N_FLOATS), np.zeros(N_FLOATS), 0
        self.lr, self.betas, self.eps, self.weight_decay = lr, betas, eps, weight_decay
        self.grad = np.zeros(N_FLOATS)

    def step(self, X, kmers, y, bag, zero_sites=(), s_given=None):
        loss, s, g, running = step_gradient(self.w, X, kmers, y, bag, zero_sites, s_given=s_given)
        self.grad = g
        for k, val in running.items():
            self.w[SLICES[k][0]] = val
        tr = trainable_mask()
        b1, b2 = self.betas
        self.t += 1
        gd = g[tr] + self.weight_decay * self.w[tr]
        self.m[tr] = b1 * self.m[tr] + (1 - b1) * gd
        self.v[tr] = b2 * self.v[tr] + (1 - b2) * gd * gd
        self.w[tr] -= self.lr / (1 - b1 ** self.t) * self.m[tr] / (np.sqrt(self.v[tr]) / np.sqrt(1 - b2 ** self.t) + self.eps)
        return loss, s


# ---- the read draw (m6anet_amd/csrc/m6a_train_draw.h) ------------------------------------------------------------------------------
M64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15


def mix(z):
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def draw(seed, i, n, bag):
    """The `bag` site-local read numbers of position i of an epoch's order: a partial Fisher-Yates shuffle of arange(n)."""
    a = {}
    for j in range(bag):
        u = mix((seed + GOLDEN * (64 * i + j + 1)) & M64) >> 32
        r = j + ((u * (n - j)) >> 32)
        a[j], a[r] = a.get(r, r), a.get(j, j)
    return [a[j] for j in range(bag)]


def sample(off, order, bag, seed):
    """m6a_train_sample: global read indices [len(order) * bag]."""
    out = []
    for i, s in enumerate(order):
        lo, n = int(off[s]), int(off[s + 1] - off[s])
        out += [lo + r for r in draw(seed, i, n, bag)]
    return np.asarray(out, np.int64)
