"""data.site_proba.csv and data.indiv_proba.csv stated in plain Python on arrays: the reference's
'%s,%d,%s,%.16f,%s,%.16f' and '%s,%d,%s,%.16f' (m6anet/utils/inference_utils.py:62,66) with the read id as str(float64) of an
integral index (`<int>.0`) for one file and `<int>_<replicate>` for pooled replicates.  Shares no code with m6a_io.cpp or m6a_csv.h.

    site row   <tx>,<pos>,<n_reads>,<%.16f of float(site_prob)>,<5-mer>,<%.16f of mod_ratio>
    read row   <tx>,<pos>,<id>,<%.16f of float(read_prob)>

CPython's '%.16f' rounds the exact binary value correctly (half to even on the exact decimal expansion), which is what glibc's printf
does; a NaN prints as glibc prints it, 'nan' or '-nan' by its sign bit, an infinity 'inf' or '-inf'.

declines(): the values the DEVICE writer hands back to the host (include/m6a.h, m6a_csv_format) -- a finite probability or ratio that
is negative (-0.0 included) or >= 2; a read id that is not integral, is negative (-0.0 included) or is >= 10^15.  texts() is defined
where nothing is declined."""
import math

SITE_HEADER = b"transcript_id,transcript_position,n_reads,probability_modified,kmer,mod_ratio\n"
INDIV_HEADER = b"transcript_id,transcript_position,read_index,probability_modified\n"


def f16(v):
    v = float(v)
    if math.isnan(v):
        return "-nan" if math.copysign(1.0, v) < 0 else "nan"
    if math.isinf(v):
        return "-inf" if v < 0 else "inf"
    return "%.16f" % v


def value_declined(v):
    v = float(v)
    return math.isfinite(v) and (math.copysign(1.0, v) < 0 or v >= 2.0)


def id_declined(v):
    v = float(v)
    return not math.isfinite(v) or v != math.floor(v) or math.copysign(1.0, v) < 0 or v >= 1e15


def names_of(tx_blob, tx_off):
    return [bytes(tx_blob[int(tx_off[t]):int(tx_off[t + 1])]).decode("latin-1") for t in range(len(tx_off) - 1)]


def declines(off, read_ids, read_prob, site_prob, mod_ratio, site_begin=0, site_end=None):
    """how many values of sites [site_begin, site_end) the device declines"""
    e = len(site_prob) if site_end is None else site_end
    r0, r1 = int(off[site_begin]), int(off[e])
    n = sum(1 for r in range(r0, r1) if id_declined(read_ids[r])) + sum(1 for r in range(r0, r1) if value_declined(read_prob[r]))
    return n + sum(1 for i in range(site_begin, e) if value_declined(site_prob[i])) + sum(1 for i in range(site_begin, e) if value_declined(mod_ratio[i]))


def texts(off, tx_pos, tx_blob, tx_off, site_tx, kmer5, read_ids, read_prob, site_prob, mod_ratio, read_rep=None, n_rep=1,
          site_begin=0, site_end=None):
    """(data.site_proba.csv rows, data.indiv_proba.csv rows) of sites [site_begin, site_end) as bytes, no header lines"""
    names = names_of(tx_blob, tx_off)
    e = len(tx_pos) if site_end is None else site_end
    site, indiv = [], []
    for i in range(site_begin, e):
        tx, pos = names[int(site_tx[i])], int(tx_pos[i])
        r0, r1 = int(off[i]), int(off[i + 1])
        k5 = bytes(bytearray(kmer5[i])).decode("latin-1")
        site.append("%s,%d,%s,%s,%s,%s\n" % (tx, pos, "%d" % (r1 - r0), f16(site_prob[i]), k5, f16(mod_ratio[i])))
        for r in range(r0, r1):
            rid = "%d.0" % int(read_ids[r]) if n_rep == 1 else "%d_%d" % (int(read_ids[r]), int(read_rep[r]))
            indiv.append("%s,%d,%s,%s\n" % (tx, pos, rid, f16(read_prob[r])))
    return "".join(site).encode("latin-1"), "".join(indiv).encode("latin-1")
