"""The site probability in closed form (include/m6a.h: m6a_site_expectation), stated in plain NumPy float64.

The reference draws n_samples reads of a site uniformly, independently and with replacement, n_iters times, and averages
1 - prod(1 - p).  One iteration has the expectation  E = 1 - (mean_i (1 - p_i)) ^ K  and the second moment of its product is
(mean_i (1 - p_i)^2) ^ K, so its standard deviation is  sqrt(m2^K - (m1^K)^2).  That difference cancels: one unit in the last
place of either power is 1e-16 / sigma in the root.  So the two sums and the two powers are carried as unevaluated pairs
hi + lo of float64 (error-free transformations: Knuth's two-sum, Dekker's split and two-product -- IEEE additions and
multiplications only, no fma, no pow / exp / log) and rounded ONCE, and this file fixes the ORDER of every operation, so that the
kernels can be held to it bit for bit:

  u_i   = 1.0 - float64(p_i);  w_i = u_i * u_i (one rounded product)
  sums  64 partial pairs, all (0, 0) at first; read i joins partial i % 64 by pair_add_double, reads in increasing i; then the
        partials are folded 32, 16, 8, 4, 2, 1: a[j] = pair_add(a[j], a[j + h]) for j < h.  S1 = hi of a[0]; the same over w_i for S2.
  m1    = S1 / n, m2 = S2 / n (one division each)
  x^K   r = (1, 0), b = (x, 0), e = K;  while e: { if e & 1: r = pair_mul(r, b);  e >>= 1;  if e: b = pair_mul(b, b) };  hi of r
  site_prob = float32(1.0 - m1^K);  mc_sigma = sqrt(max(m2^K - m1^K * m1^K, 0.0));  mod_ratio = mean(p >= thr) in float64
An empty bag gives NaN three times.
"""
import numpy as np

WIDTH = 64
SPLIT = 134217729.0                                         # 2^27 + 1


def two_sum(a, b):
    """a + b = s + e exactly"""
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def quick_pair(s, e):
    """(s, e) with |e| small against |s| -> the pair whose hi is the rounded s + e"""
    hi = s + e
    return hi, e - (hi - s)


def split(a):
    c = SPLIT * a
    h = c - (c - a)
    return h, a - h


def two_prod(a, b):
    """a * b = p + e exactly (Dekker)"""
    p = a * b
    ah, al = split(a)
    bh, bl = split(b)
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def pair_add_double(a, b):
    s, e = two_sum(a[0], b)
    return quick_pair(s, e + a[1])


def pair_add(a, b):
    s, e = two_sum(a[0], b[0])
    return quick_pair(s, e + (a[1] + b[1]))


def pair_mul(a, b):
    p, e = two_prod(a[0], b[0])
    return quick_pair(p, e + (a[0] * b[1] + a[1] * b[0]))


def fold_sums(u):
    """u float64 [B, n] -> the statement's sum over axis 1, [B]."""
    B, n = u.shape
    rows = (n + WIDTH - 1) // WIDTH
    pad = np.zeros((B, rows * WIDTH), np.float64)
    pad[:, :n] = u
    pad = pad.reshape(B, rows, WIDTH)
    a = (np.zeros((B, WIDTH), np.float64), np.zeros((B, WIDTH), np.float64))
    for r in range(rows):                                   # read i joins partial i % 64, in increasing i
        a = pair_add_double(a, pad[:, r, :])
    h = WIDTH // 2
    while h >= 1:
        a = pair_add((a[0][:, :h], a[1][:, :h]), (a[0][:, h:2 * h], a[1][:, h:2 * h]))
        h //= 2
    return a[0][:, 0]


def int_power(x, K):
    """x^K by square-and-multiply from the lowest bit of K in pairs, rounded once (x float64 array)."""
    r = (np.ones_like(x), np.zeros_like(x))
    b = (x.copy(), np.zeros_like(x))
    e = int(K)
    while e:
        if e & 1:
            r = pair_mul(r, b)
        e >>= 1
        if e:
            b = pair_mul(b, b)
    return r[0]


def expectation_f64(p, K=20):
    """p float32 [B, n], n >= 1 -> (1.0 - m1^K, mc_sigma), both float64 [B]: site_prob before its rounding to float32."""
    p = np.asarray(p, np.float32)
    n = p.shape[1]
    with np.errstate(all="ignore"):
        u = 1.0 - p.astype(np.float64)
        m1 = fold_sums(u) / np.float64(n)
        m2 = fold_sums(u * u) / np.float64(n)
        q1, q2 = int_power(m1, K), int_power(m2, K)
        v = q2 - q1 * q1
        return 1.0 - q1, np.sqrt(np.where(v < 0.0, 0.0, v))     # a negative rounding residue is 0; NaN stays NaN


def uniform_expectation(p, K=20, thr=None):
    """p float32 [B, n], every bag of n reads -> (site_prob float32 [B], mc_sigma float64 [B], mod_ratio float64 [B] or None)."""
    p = np.asarray(p, np.float32)
    B, n = p.shape
    with np.errstate(all="ignore"):
        if n == 0:
            nan = np.full(B, np.nan)
            return nan.astype(np.float32), nan.copy(), (nan.copy() if thr is not None else None)
        e64, sigma = expectation_f64(p, K)
        site = e64.astype(np.float32)
        mod = None
        if thr is not None:
            mod = (p >= np.float32(thr)).sum(axis=1).astype(np.float64) / np.float64(n)
    return site, sigma, mod


def site_expectation(read_prob, off, K=20, thr=None):
    """CSR bags: read_prob float32 [R], off int64 [S + 1] -> (site_prob [S], mc_sigma [S], mod_ratio [S] or None).  Bags of one
    size are evaluated together; the operations per site are those of the docstring."""
    p = np.asarray(read_prob, np.float32)
    off = np.asarray(off, np.int64)
    S = off.size - 1
    n = np.diff(off)
    site, sigma = np.empty(S, np.float32), np.empty(S, np.float64)
    mod = np.empty(S, np.float64) if thr is not None else None
    for size in np.unique(n):
        idx = np.flatnonzero(n == size)
        bags = p[(off[idx][:, None] + np.arange(size)[None, :]).reshape(-1)].reshape(idx.size, int(size))
        s, g, m = uniform_expectation(bags, K, thr)
        site[idx], sigma[idx] = s, g
        if mod is not None:
            mod[idx] = m
    return site, sigma, mod
