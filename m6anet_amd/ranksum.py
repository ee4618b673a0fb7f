"""The host side of the rank-sum test between two conditions (include/m6a.h: m6a_site_ranksum; the `eventalign_diff` command): what
follows from the three counts and z of a pair of sites, the join of two site tables, and the text of data.diff.csv.  NumPy and `math`
only.
  p_value     the two-sided p of the normal approximation, erfc(|z| / sqrt(2)); NaN where z is NaN
  auc         U / (n m) = (2 gt + eq) / 2 / (n m), the probability that a read of the first bag scores above a read of the second
              (ties count half); NaN for an undefined pair
  bh          Benjamini-Hochberg q over the rows whose p is not NaN: stable order by p, q_(i) = min(1, min_{j >= i} p_(j) M / j)
  join        the inner join of two site tables on (transcript_id, transcript_position), in the order of the first table
  diff_rows   the lines of data.diff.csv
  signal_rows the lines of data.diff_signal.csv (`eventalign_diff --signal`; m6a_site_signal_ranksum): nine per pair, one BH family"""
import math

import numpy as np

DIFF_HEADER = ("transcript_id,transcript_position,kmer,n_reads_a,n_reads_b,probability_modified_a,probability_modified_b,"
               "mod_ratio_a,mod_ratio_b,auc,z,p_value,q_value")
DIFF_FILE = "data.diff.csv"
SIGNAL_HEADER = "transcript_id,transcript_position,kmer,n_reads_a,n_reads_b,position_offset,feature,auc,z,p_value,q_value"
SIGNAL_FILE = "data.diff_signal.csv"
# the columns of X [R][9] as (position_offset, feature): the reference's order, dwell_time, norm_std, norm_mean per position
# (m6anet/utils/dataprep_utils.py:132) and positions -1, 0, +1 (the loader's left, centre and right indices)
SIGNAL_COLUMNS = tuple((o, f) for o in (-1, 0, 1) for f in ("dwell_time", "norm_std", "norm_mean"))
N_SIGNAL = len(SIGNAL_COLUMNS)
_SQRT2 = math.sqrt(2.0)


def p_value(z):
    z = np.asarray(z, np.float64)
    return np.array([float("nan") if math.isnan(v) else math.erfc(abs(v) / _SQRT2) for v in z.ravel().tolist()], np.float64).reshape(z.shape)


def auc(gt, eq, n, m):
    gt, eq = np.asarray(gt, np.int64), np.asarray(eq, np.int64)
    nm = np.asarray(n, np.float64) * np.asarray(m, np.float64)
    out = np.full(gt.shape, np.nan)
    ok = gt >= 0
    out[ok] = (2 * gt[ok] + eq[ok]).astype(np.float64) * 0.5 / nm[ok]
    return out


def bh(p):
    p = np.asarray(p, np.float64)
    q = np.full(p.shape, np.nan)
    rows = np.flatnonzero(~np.isnan(p))
    M = rows.size
    if M == 0:
        return q
    order = np.argsort(p[rows], kind="stable")
    adj = p[rows][order] * float(M) / np.arange(1, M + 1, dtype=np.float64)
    adj = np.minimum(np.minimum.accumulate(adj[::-1])[::-1], 1.0)
    q[rows[order]] = adj
    return q


def join(tx_a, pos_a, tx_b, pos_b):
    """tx_* [S] transcript names (str or bytes), pos_* [S] positions -> (pair_a, pair_b) int64: pair k is row pair_a[k] of the first
    table and row pair_b[k] of the second, the rows with the same (name, position), in the order of the first table.  A key names
    one row of its table (a site table has no duplicates); were the second table to repeat one, its first row is taken."""
    where = {}
    for j, key in enumerate(zip(tx_b, (int(x) for x in pos_b))):
        where.setdefault(key, j)
    pa, pb = [], []
    for i, key in enumerate(zip(tx_a, (int(x) for x in pos_a))):
        j = where.get(key)
        if j is not None:
            pa.append(i)
            pb.append(j)
    return np.array(pa, np.int64), np.array(pb, np.int64)


def _repr(v):
    return "nan" if math.isnan(v) else repr(v)


def diff_rows(tx, pos, kmer, n_a, n_b, site_a, site_b, mod_a, mod_b, gt, eq, z):
    """The data lines of data.diff.csv (no header, each with its newline) for P pairs: tx [P] names, pos [P], kmer [P] the 5-mers,
    n_a / n_b the bag sizes, site_* float32 and mod_* float64 the two conditions' columns of data.site_proba.csv, and the test's
    gt, eq, z.  The probabilities and ratios are '%.16f' as the site CSV prints them; auc, z, p_value and q_value are repr(float)."""
    z = np.asarray(z, np.float64)
    p = p_value(z)
    q = bh(p)
    a = auc(gt, eq, n_a, n_b)
    return ["%s,%d,%s,%d,%d,%.16f,%.16f,%.16f,%.16f,%s,%s,%s,%s\n"
            % (tx[k], pos[k], kmer[k], n_a[k], n_b[k], site_a[k], site_b[k], mod_a[k], mod_b[k], _repr(float(a[k])), _repr(float(z[k])),
               _repr(float(p[k])), _repr(float(q[k]))) for k in range(len(z))]


def diff_text(*columns):
    return DIFF_HEADER + "\n" + "".join(diff_rows(*columns))


def signal_rows(tx, pos, kmer, n_a, n_b, gt, eq, z):
    """The data lines of data.diff_signal.csv (no header, each with its newline) for P pairs: tx, pos, kmer, n_a, n_b as diff_rows takes
    them and gt, eq, z [P, 9] of m6a_site_signal_ranksum.  Nine lines per pair in column order, SIGNAL_COLUMNS naming the column;
    q_value is Benjamini-Hochberg over all 9 P rows whose p is not NaN, one family; auc, z, p_value and q_value are repr(float)."""
    z = np.asarray(z, np.float64).reshape(-1, N_SIGNAL)
    P = z.shape[0]
    gt, eq = np.asarray(gt, np.int64).reshape(P, N_SIGNAL), np.asarray(eq, np.int64).reshape(P, N_SIGNAL)
    p = p_value(z)
    q = bh(p.ravel()).reshape(P, N_SIGNAL)
    n_a, n_b = np.asarray(n_a, np.int64).reshape(P), np.asarray(n_b, np.int64).reshape(P)
    a = auc(gt, eq, np.repeat(n_a[:, None], N_SIGNAL, axis=1), np.repeat(n_b[:, None], N_SIGNAL, axis=1))
    return ["%s,%d,%s,%d,%d,%d,%s,%s,%s,%s,%s\n"
            % (tx[k], pos[k], kmer[k], n_a[k], n_b[k], SIGNAL_COLUMNS[c][0], SIGNAL_COLUMNS[c][1], _repr(float(a[k, c])), _repr(float(z[k, c])),
               _repr(float(p[k, c])), _repr(float(q[k, c]))) for k in range(P) for c in range(N_SIGNAL)]


def signal_text(*columns):
    return SIGNAL_HEADER + "\n" + "".join(signal_rows(*columns))
