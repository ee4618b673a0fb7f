"""The read encoder's forward pass (eval mode), stated once in NumPy float64 from the float32 blob values.  No torch, no tricks: the
high-precision reference of tests/test_encoder_statement.py and tests/test_gpu_encoder_weights.py.  oracle/m6a_oracle.c stays what it
is, the float32 restatement of the reference's operation order; include/m6a.h (m6a_encode_reads) states the same operation.

Blob layout: train_statement.SLICES (the one layout table of the tests).

  x     = [X (9) | E[k0] | E[k1] | E[k2]]                       15 values per read, the k-mer ids being the read's site's
  z1    = x W1^T + b1
  y1    = (z1 - running_mean) gamma / sqrt(running_var + float32(1e-5)) + beta
  a1    = relu(y1),  h2 = relu(a1 W2^T + b2)                    h2 = the read representation
  logit = h2 . W3 + b3,  p = 1 / (1 + exp(-logit))
"""
import numpy as np

import train_statement as TS

BN_EPS = np.float64(np.float32(1e-5))


def relu(a):
    return np.where(a < 0.0, 0.0, a)                            # keeps NaN, as torch's relu does (np.maximum would too)


def layers(w, X, site_kmers, off):
    """Every intermediate, float64: {'x', 'z1', 'alpha', 'y1', 'a1', 'h2', 'logit', 'p'} plus the unpacked blob under 'w'."""
    p = TS.unpack(np.asarray(w, np.float32).astype(np.float64))
    off = np.asarray(off, np.int64)
    X = np.asarray(X, np.float32).astype(np.float64).reshape(-1, 9)
    km = np.asarray(site_kmers).reshape(-1, 3).astype(np.int64)
    assert X.shape[0] == off[-1] and km.shape[0] == off.size - 1
    kr = np.repeat(km, np.diff(off), axis=0)                    # [R, 3]: every read carries its site's k-mers
    R = X.shape[0]
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        x = np.concatenate([X, p["E"][kr].reshape(R, 6)], axis=1)
        z1 = x @ p["W1"].T + p["b1"]
        alpha = p["gamma"] / np.sqrt(p["running_var"] + BN_EPS)
        y1 = (z1 - p["running_mean"]) * alpha + p["beta"]
        a1 = relu(y1)
        h2 = relu(a1 @ p["W2"].T + p["b2"])
        logit = h2 @ p["W3"] + p["b3"][0]
        prob = 1.0 / (1.0 + np.exp(-logit))
    return {"w": p, "x": x, "z1": z1, "alpha": alpha, "y1": y1, "a1": a1, "h2": h2, "logit": logit, "p": prob}


def forward(w, X, site_kmers, off):
    """-> (p [R], h2 [R, 32], logit [R]), float64."""
    L = layers(w, X, site_kmers, off)
    return L["p"], L["h2"], L["logit"]
