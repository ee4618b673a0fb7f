"""Grouped input, stated in plain Python (include/m6a.h: m6a_prep_group; `eventalign_inference --grouped`).

Take the file's runs in file order, as tests/eventalign_statement.py's index() forms them (lines without a tab belong to no run).
The input is GROUPED when no contig name heads a run after a run with a different contig has followed an earlier run of that name:
every transcript's runs form one stretch.  Otherwise the OFFENDER is the first run in file order that breaks the rule, and the error
names its transcript and the file offset of its first byte.  Nothing here depends on a window size or a group size.
"""
import eventalign_statement as S

EFORMAT = -7                                  # M6A_EFORMAT (include/m6a.h)


def offender(data):
    """None for grouped input, else (name, start) of the first run whose contig was seen before and left since"""
    names, runs = S.index(data)
    closed, current = set(), None
    for r in runs:
        if r["tx"] != current:
            if current is not None:
                closed.add(current)
            if r["tx"] in closed:
                return names[r["tx"]], r["start"]
            current = r["tx"]
    return None


def grouped(data):
    return offender(data) is None


def error_text(path, name, start):
    return "%s: transcript %s appears again at byte %d after other transcripts: the input is not grouped by transcript (run without --grouped)" % (
        path, name.decode(), start)


def flush_boundaries(n_sites, batch_size, save_per_batch):
    """the site counts at which a job of n_sites sites ends a flush group before its end: batch b (sites [b * batch_size, ...)) ends
    one when (b + 1) % save_per_batch != 0 -- they depend on the batch index alone"""
    return [(b + 1) * batch_size for b in range(n_sites // batch_size) if (b + 1) % save_per_batch and (b + 1) * batch_size < n_sites]
