"""What `dataprep` writes, stated in plain Python from arrays: the record of data.json, the rows of data.info and eventalign.index
and the line of data.log.  The host writer (m6a_io.cpp: emit_transcript, dataprep_impl) and the device writer
(m6anet_amd/csrc/m6a_dataprep.h) both give these bytes; test_dataprep_json_statement.py holds the statement itself to the files of
tests/golden/ref_tests_data, which the reference wrote.  from_eventalign joins it to tests/eventalign_statement.py: the four files
from the bytes of eventalign.txt alone (tests/test_dataprep_files_statement.py holds the host writer to that join)."""
import math

import numpy as np

import eventalign_statement as E

INFO_HEADER = "transcript_id,transcript_position,start,end,n_reads\n"
INDEX_HEADER = "transcript_id,read_index,pos_start,pos_end\n"


def number(v, round3=False):
    """repr(float), of np.round(v, 3) under --compress; a value that is not finite as the writers spell it (json.dumps' words)."""
    v = float(np.round(np.float64(v), 3)) if round3 else float(v)
    if math.isnan(v):
        return "NaN"
    if math.isinf(v):
        return "Infinity" if v > 0 else "-Infinity"
    return repr(v)


def record(tx, pos, kmer7, features, reads, round3=False):
    """One site: features [n][3 (2 n_neighbors + 1)] float64 in the writer's read order, reads [n] the read indices."""
    rows = []
    for f, r in zip(features, reads):
        assert len(f) == 3 * (len(kmer7) - 4)
        rows.append("[" + ",".join(number(x, round3) for x in f) + "," + repr(float(int(r))) + "]")
    return '{"%s":{"%d":{"%s":[%s]}}}\n' % (tx, int(pos), kmer7, ",".join(rows))


def info_row(tx, pos, start, end, n_reads):
    return "%s,%d,%d,%d,%d\n" % (tx, pos, start, end, n_reads)


def log_line(tx):
    return "%s: Data preparation ... Done.\n" % tx


def index_row(tx, read, start, end):
    return "%s,%d,%d,%d\n" % (tx, read, start, end)


def files(sites, runs, logged, round3=False):
    """The four files as text: sites = [(tx, pos, kmer7, features, reads)] in the writer's order, runs = [(tx, read, start, end)]
    in file order, logged = transcripts in order.  Returns a dict by file name."""
    js, info, at = [], [INFO_HEADER], 0
    for tx, pos, kmer7, features, reads in sites:
        rec = record(tx, pos, kmer7, features, reads, round3)
        js.append(rec)
        info.append(info_row(tx, pos, at, at + len(rec), len(reads)))
        at += len(rec)
    return {"data.json": "".join(js), "data.info": "".join(info), "data.log": "".join(log_line(t) for t in logged),
            "eventalign.index": INDEX_HEADER + "".join(index_row(*r) for r in runs)}


def from_eventalign(names, runs, readcount_min=1, readcount_max=1000, min_segment_count=20):
    """(sites, runs, logged) for files() and n_declined() from eventalign_statement's names and runs (with npos and rows).
    Sites are eventalign_statement.records'; runs are (name, read, start, end) in file order; `logged` are the transcripts, in order
    of first appearance, that reached readcount_min runs -- walking their runs as records() does, up to the one that takes the count
    over readcount_max -- and whose dict of reads (a later run of a read replaces the earlier one) then holds at least one candidate
    row.  min_segment_count does not enter into it: a transcript none of whose sites is kept is logged all the same."""
    sites = [(tx, pos, seq, [f for f, _ in rows], [rd for _, rd in rows])
             for tx, pos, seq, rows in E.records(names, runs, readcount_min, readcount_max, min_segment_count)]
    logged = []
    for t in range(len(names)):
        by_read, count = {}, 0
        for r in (r for r in runs if r["tx"] == t):
            if r["npos"] > 1:
                by_read[r["read"]] = r
            count += 1
            if count > readcount_max:
                break
        if count >= readcount_min and any(r["rows"] for r in by_read.values()):
            logged.append(names[t].decode())
    return sites, [(names[r["tx"]].decode(), r["read"], r["start"], r["end"]) for r in runs], logged


def n_declined(sites, round3=False):
    """How many numbers of these sites the device printer declines (m6a_repr.h): a feature outside [1e-4, 1e16) after the rounding,
    or not finite; a read index outside [0, 2^53)."""
    n = 0
    for _, _, _, features, reads in sites:
        f = np.asarray(features, np.float64)
        if round3:
            f = np.round(f, 3)
        n += int((~((f >= 1e-4) & (f < 1e16))).sum()) + sum(1 for r in reads if not 0 <= int(r) < 2 ** 53)
    return n
