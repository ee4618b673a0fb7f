"""Several eventalign.txt files that are replicates -> the loader's arrays, stated in plain Python on top of eventalign_statement.

This is the definition `inference --input_dir d0 d1 ...` after `dataprep` of every file (m6a_io_load_sites with several directories)
and `eventalign_inference --eventalign f0 f1 ...` (m6a_prep_sites_build_multi) are held to.  It shares no code with either:

    per file   eventalign_statement.records(): the file's own transcripts, readcount cut, one run per read, rows by (position, place),
               a site = a position with at least min_segment_count rows.  No floor of 20 reads here.
    union      sites keyed by (transcript name, position) in order of first appearance: file 0's in file 0's order, then what file 1
               adds in file 1's order, ...; a site's parts in file order
    filter     kept when the parts' reads SUM to at least min_reads (20)
    checks     kept sites only, in order, and inside a site: the normalisation factors of the three 5-mers of the FIRST part's
               7-mer, then every later part's 7-mer against the first, then the vocabulary
    arrays     X, km, off, tx_pos, read_ids, tx, kmer7 as eventalign_statement.sites() makes them per read, and read_rep: the
               position of the read's file in the list (a file without sites still takes its number)
"""
import numpy as np

import eventalign_statement as S


def file_records(data, readcount_min=1, readcount_max=1000, min_segment_count=20):
    names, runs = S.table(data, 1)
    return S.records(names, runs, readcount_min, readcount_max, min_segment_count)


def union(per_file):
    """{(name, position): [(replicate, sequence, rows)]} in order of first appearance (a dict keeps insertion order)"""
    pooled = {}
    for rep, recs in enumerate(per_file):
        for name, position, seq, rows in recs:
            pooled.setdefault((name, position), []).append((rep, seq, rows))
    return pooled


def sites(per_file, norm=None, min_reads=20):
    """per_file: file_records() of every file, in command-line order.  Returns eventalign_statement.sites()' dict plus read_rep
    int32 [R], n_replicates, and parts: per kept site the read count of every part [(replicate, n)]."""
    voc = S.vocabulary()
    X, km, off, tx_pos, read_ids, read_rep, tx, kmer7, parts_out = [], [], [0], [], [], [], [], [], []
    for (name, position), parts in union(per_file).items():
        n = sum(len(rows) for _, _, rows in parts)
        if n < min_reads:
            continue
        seq = parts[0][1]
        fives = [seq[c:c + 5] for c in range(3)]
        for k in fives:
            if norm is not None and k not in norm:
                raise S.StatementError(S.EFORMAT, "no normalisation factors for %s" % k)
        for _, other, _ in parts[1:]:
            if other != seq:
                raise S.StatementError(S.EFORMAT, "replicates disagree on the sequence of %s:%d" % (name, position))
        for k in fives:
            if k not in voc:
                raise S.StatementError(S.EFORMAT, "site %s:%d: %s is not a DRACH context" % (name, position, seq))
        if norm is not None:
            mean = np.concatenate([np.asarray(norm[k][0], np.float64) for k in fives])
            std = np.concatenate([np.asarray(norm[k][1], np.float64) for k in fives])
        for rep, _, rows in parts:
            for features, read in rows:
                v = np.array(features, np.float64)
                v[np.isnan(v)] = S.CANONICAL_NAN
                with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
                    X.append((v if norm is None else (v - mean) / std).astype(np.float32))
                read_ids.append(float(read))
                read_rep.append(rep)
        km.append([voc.index(k) for k in fives])
        off.append(off[-1] + n)
        tx_pos.append(position)
        tx.append(name)
        kmer7.append(seq)
        parts_out.append([(rep, len(rows)) for rep, _, rows in parts])
    if not tx:
        raise S.StatementError(S.EFORMAT, "no site with at least %d reads" % min_reads)
    return dict(X=np.array(X, np.float32).reshape(-1, 9), km=np.array(km, np.uint8).reshape(-1, 3), off=np.array(off, np.int64),
                tx_pos=np.array(tx_pos, np.int64), read_ids=np.array(read_ids, np.float64), read_rep=np.array(read_rep, np.int32),
                tx=tx, kmer7=kmer7, n_replicates=len(per_file), parts=parts_out)
