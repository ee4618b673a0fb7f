"""The host side of the rank-sum test between two conditions (include/m6a.h: m6a_site_ranksum; the `eventalign_diff` command): what
follows from the three counts and z of a pair of sites, the join of two site tables, and the text of data.diff.csv.  NumPy and `math`
only.
  p_value     the two-sided p of the normal approximation, erfc(|z| / sqrt(2)); NaN where z is NaN
  auc         U / (n m) = (2 gt + eq) / 2 / (n m), the probability that a read of the first bag scores above a read of the second
              (ties count half); NaN for an undefined pair
  bh          Benjamini-Hochberg q over the rows whose p is not NaN: stable order by p, q_(i) = min(1, min_{j >= i} p_(j) M / j)
  join        the inner join of two site tables on (transcript_id, transcript_position), in the order of the first table
  diff_rows   the lines of data.diff.csv
  signal_rows the lines of data.diff_signal.csv (`eventalign_diff --signal`; m6a_site_signal_ranksum): nine per pair, one BH family
What follows from the Kolmogorov-Smirnov integers and the medians of m6a_site_ks / m6a_site_signal_ks (`eventalign_diff --ks`):
  ks_d        D = max(d_pos, d_neg) / (n m), scipy.stats.ks_2samp's statistic; NaN for an undefined pair
  ks_sign     +1 where d_pos >= d_neg (the first bag's CDF lies above at the widest gap: its values tend lower), else -1; 0: undefined
  ks_p_value  Q(lambda), lambda = sqrt(n m / (n + m)) D, Q the Kolmogorov limit distribution: scipy.stats.kstwobign.sf(lambda), NOT
              ks_2samp's p (exact for small bags); the limit is conservative for small bags
  ks_h        h = max(d_pos, d_neg), the statistic in units of 1 / (n m) as m6a_ks_exact takes it (include/m6a.h); -1: undefined
  ks_rows     the lines of data.diff_ks.csv;  signal_ks_rows  those of data.diff_signal_ks.csv, nine per pair, one BH family.  Given
              p_exact, m6a_ks_exact's p-values of the same tests (`eventalign_diff --ks_exact`), p_value is the exact one wherever it
              is not NaN and Q(lambda) elsewhere, q_value corrects p_value as written, and a last column p_method says which it is"""
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
KS_HEADER = "transcript_id,transcript_position,kmer,n_reads_a,n_reads_b,median_a,median_b,median_shift,ks_d,ks_sign,p_value,q_value"
KS_FILE = "data.diff_ks.csv"
SIGNAL_KS_HEADER = ("transcript_id,transcript_position,kmer,n_reads_a,n_reads_b,position_offset,feature,median_a,median_b,median_shift,"
                    "ks_d,ks_sign,p_value,q_value")
SIGNAL_KS_FILE = "data.diff_signal_ks.csv"
P_METHOD_COLUMN = ",p_method"            # behind either KS header when the exact p-values are given
P_METHODS = ("asymptotic", "exact")
KS_SWITCH = 1.18                        # lambda below it: the theta-function form of Q; seven terms of either series
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


def ks_d(d_pos, d_neg, n, m):
    d_pos, d_neg = np.asarray(d_pos, np.int64), np.asarray(d_neg, np.int64)
    nm = np.asarray(n, np.float64) * np.asarray(m, np.float64)
    out = np.full(d_pos.shape, np.nan)
    ok = d_pos >= 0
    out[ok] = np.maximum(d_pos, d_neg)[ok].astype(np.float64) / nm[ok]
    return out


def ks_h(d_pos, d_neg):
    return np.maximum(np.asarray(d_pos, np.int64), np.asarray(d_neg, np.int64))


def ks_sign(d_pos, d_neg):
    d_pos, d_neg = np.asarray(d_pos, np.int64), np.asarray(d_neg, np.int64)
    return np.where(d_pos < 0, 0, np.where(d_pos >= d_neg, 1, -1)).astype(np.int64)


def kolmogorov_sf(lam):
    """Q(lambda) = 2 sum_{k>=1} (-1)^(k-1) exp(-2 k^2 lambda^2); below KS_SWITCH its theta-function form
    1 - sqrt(2 pi) / lambda sum_{k>=1} exp(-(2k-1)^2 pi^2 / (8 lambda^2)), whose terms fall off as fast there.  Seven terms of either."""
    if math.isnan(lam):
        return lam
    if lam <= 0.0:
        return 1.0
    if lam < KS_SWITCH:
        c = math.pi * math.pi / (8.0 * lam * lam)
        return 1.0 - math.sqrt(2.0 * math.pi) / lam * sum(math.exp(-float((2 * k - 1) ** 2) * c) for k in range(1, 8))
    return 2.0 * sum((1.0 if k % 2 else -1.0) * math.exp(-2.0 * float(k * k) * lam * lam) for k in range(1, 8))


def ks_lambda(d, n, m):
    return math.sqrt(float(n) * float(m) / float(n + m)) * d


def ks_p_value(d, n, m):
    """d = ks_d(...), n and m the bag sizes, arrays of one shape -> p, NaN where d is NaN"""
    d = np.asarray(d, np.float64)
    n, m = np.broadcast_to(np.asarray(n, np.int64), d.shape), np.broadcast_to(np.asarray(m, np.int64), d.shape)
    return np.array([float("nan") if math.isnan(v) else kolmogorov_sf(ks_lambda(v, int(i), int(j)))
                     for v, i, j in zip(d.ravel().tolist(), n.ravel().tolist(), m.ravel().tolist())], np.float64).reshape(d.shape)


def _ks_fields(d_pos, d_neg, med_a, med_b, n_a, n_b, p_exact=None):
    """per test, flat: the seven strings median_a .. q_value, and p_method behind them where p_exact is given; one BH family over all
    of them"""
    d_pos, d_neg = np.asarray(d_pos, np.int64).ravel(), np.asarray(d_neg, np.int64).ravel()
    med_a, med_b = np.asarray(med_a, np.float64).ravel(), np.asarray(med_b, np.float64).ravel()
    d = ks_d(d_pos, d_neg, n_a, n_b)
    sign = ks_sign(d_pos, d_neg)
    p = ks_p_value(d, n_a, n_b)
    method = ()
    if p_exact is not None:
        p_exact = np.asarray(p_exact, np.float64).ravel()
        assert p_exact.size == d.size
        exact = ~np.isnan(p_exact)
        p = np.where(exact, p_exact, p)                          # an item m6a_ks_exact leaves undefined keeps the limit's p (NaN: stays NaN)
        method = [(P_METHODS[int(e)],) for e in exact]
    q = bh(p)
    with np.errstate(invalid="ignore"):
        shift = med_a - med_b                                    # inf - inf: NaN
    return [(_repr(float(med_a[k])), _repr(float(med_b[k])), _repr(float(shift[k])), _repr(float(d[k])), "%d" % sign[k] if sign[k] else "nan",
             _repr(float(p[k])), _repr(float(q[k]))) + (method[k] if method else ()) for k in range(d.size)]


def ks_rows(tx, pos, kmer, n_a, n_b, d_pos, d_neg, med_a, med_b, p_exact=None):
    """The data lines of data.diff_ks.csv (no header, each with its newline) for P pairs: tx, pos, kmer, n_a, n_b as diff_rows takes them
    and the four outputs [P] of m6a_site_ks.  median_shift = median_a - median_b; floats are repr(float), ks_sign is 1 or -1, and an
    undefined pair is `nan` in all seven; q_value is Benjamini-Hochberg over the rows whose p is not NaN.  p_exact [P]: see above."""
    n_a, n_b = np.asarray(n_a, np.int64).ravel(), np.asarray(n_b, np.int64).ravel()
    f = _ks_fields(d_pos, d_neg, med_a, med_b, n_a, n_b, p_exact)
    return ["%s,%d,%s,%d,%d,%s\n" % (tx[k], pos[k], kmer[k], n_a[k], n_b[k], ",".join(f[k])) for k in range(len(f))]


def ks_text(*columns, p_exact=None):
    return KS_HEADER + (P_METHOD_COLUMN if p_exact is not None else "") + "\n" + "".join(ks_rows(*columns, p_exact=p_exact))


def signal_ks_rows(tx, pos, kmer, n_a, n_b, d_pos, d_neg, med_a, med_b, p_exact=None):
    """The data lines of data.diff_signal_ks.csv for P pairs and the four outputs [P, 9] of m6a_site_signal_ks: nine lines per pair in
    column order, SIGNAL_COLUMNS naming the column, the medians in the normalised units of X; q_value is Benjamini-Hochberg over all
    9 P rows whose p is not NaN, one family.  p_exact [P, 9]: see above."""
    n_a, n_b = np.asarray(n_a, np.int64).ravel(), np.asarray(n_b, np.int64).ravel()
    P = n_a.size
    f = _ks_fields(d_pos, d_neg, med_a, med_b, np.repeat(n_a, N_SIGNAL), np.repeat(n_b, N_SIGNAL), p_exact)
    assert len(f) == P * N_SIGNAL
    return ["%s,%d,%s,%d,%d,%d,%s,%s\n" % (tx[k], pos[k], kmer[k], n_a[k], n_b[k], SIGNAL_COLUMNS[c][0], SIGNAL_COLUMNS[c][1],
                                          ",".join(f[k * N_SIGNAL + c])) for k in range(P) for c in range(N_SIGNAL)]


def signal_ks_text(*columns, p_exact=None):
    return SIGNAL_KS_HEADER + (P_METHOD_COLUMN if p_exact is not None else "") + "\n" + "".join(signal_ks_rows(*columns, p_exact=p_exact))
