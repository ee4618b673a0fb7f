"""What `dataprep` writes, stated in plain Python from arrays: the record of data.json, the rows of data.info and eventalign.index
and the line of data.log.  The host writer (m6a_io.cpp: emit_transcript, dataprep_impl) and the device writer
(m6anet_amd/csrc/m6a_dataprep.h) both give these bytes; test_dataprep_json_statement.py holds the statement itself to the files of
tests/golden/ref_tests_data, which the reference wrote."""
import numpy as np

INFO_HEADER = "transcript_id,transcript_position,start,end,n_reads\n"
INDEX_HEADER = "transcript_id,read_index,pos_start,pos_end\n"


def number(v, round3=False):
    """repr(float), of np.round(v, 3) under --compress."""
    return repr(float(np.round(np.float64(v), 3))) if round3 else repr(float(v))


def record(tx, pos, kmer7, features, reads, round3=False):
    """One site: features [n][9] float64 in the writer's read order, reads [n] the read indices."""
    rows = []
    for f, r in zip(features, reads):
        assert len(f) == 9
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
