"""Read names (`eventalign_inference --read_names`) stated in plain Python.

nanopolish and f5c run with --print-read-names write the read's UUID into field 4 of eventalign.txt, where the integer read_index
stands otherwise.  This is the definition m6anet_amd/csrc/m6a_uuid.h, the prep kernels and both CSV writers are held to; it
shares no code with them and is meant to be read top to bottom:

    parse      a field -> its 128 bits, or None
    show       128 bits -> the 36 bytes
    twin       a named file -> the same file with every name replaced by its dense index, and the names in index order
    table      names -> the [n][16] bytes the handle reports
    indiv      the twin's data.indiv_proba.csv -> the named file's: column 3 mapped through the tables

A read name is exactly 36 bytes: 8-4-4-4-12 lowercase hex digits with '-' at offsets 8, 13, 18 and 23.  The feature is defined by
the twin: whatever the product makes of the twin file, it makes of the named file, and only column 3 of data.indiv_proba.csv shows
the difference.
"""
import numpy as np

import eventalign_statement as S

DASHES = (8, 13, 18, 23)
HEX = b"0123456789abcdef"


def parse(field):
    """the 128-bit value of a read name, or None for anything else: upper case, 35 or 37 bytes, a dash elsewhere, an integer, b''"""
    if len(field) != 36:
        return None
    digits = []
    for i, c in enumerate(field):
        if i in DASHES:
            if c != ord("-"):
                return None
        elif c in HEX:
            digits.append(HEX.index(c))
        else:
            return None
    v = 0
    for d in digits:
        v = v * 16 + d
    return v


def show(v):
    h = "%032x" % v
    return ("%s-%s-%s-%s-%s" % (h[:8], h[8:12], h[12:16], h[16:20], h[20:])).encode()


def twin(data):
    """(twin bytes, [names as 128-bit integers, in order of first appearance]).

    The body lines with at least three tabs carry a name in field 4 (the text between the third tab and the fourth, or the line's
    end); a line without a tab is left alone, as eventalign_statement.index skips it.  A line with one or two tabs is the error
    'short line at byte <offset of the line>', a field that is no name is 'read name at byte <offset of the field>: not a lowercase
    UUID'; of all such errors of the file the one at the lowest offset is raised, whichever kind it is."""
    first = data.find(b"\n")
    if first < 0:
        raise S.StatementError(S.EFORMAT, "no header line")
    out, names, ids, errors = [data[:first + 1]], [], {}, []
    p, n = first + 1, len(data)
    while p < n:
        nl = data.find(b"\n", p)
        end, nxt = (n, n) if nl < 0 else (nl, nl + 1)
        line = data[p:end]
        tabs = [i for i, c in enumerate(line) if c == 9]
        if not tabs:
            out.append(data[p:nxt])
        elif len(tabs) < 3:
            errors.append((p, "short line at byte %d" % p))
        else:
            a, b = tabs[2] + 1, tabs[3] if len(tabs) > 3 else len(line)
            v = parse(line[a:b])
            if v is None:
                errors.append((p + a, "read name at byte %d: not a lowercase UUID" % (p + a)))
            else:
                if v not in ids:
                    ids[v] = len(names)
                    names.append(v)
                out.append(line[:a] + b"%d" % ids[v] + line[b:] + data[end:nxt])
        p = nxt
    if errors:
        raise S.StatementError(S.EFORMAT, min(errors)[1])
    return b"".join(out), names


def table(names):
    """the names as the handle reports them: uint8 [n][16], the 32 hex digits of each, first digit first"""
    return np.frombuffer(b"".join(v.to_bytes(16, "big") for v in names), np.uint8).reshape(len(names), 16)


def indiv(text, tables):
    """data.indiv_proba.csv of the named files from the twins': column 3 is `<index>.0` (one file: tables = [names]) and becomes
    `<uuid>`, or `<index>_<k>` (replicates: tables[k] is file k's names) and becomes `<uuid>_<k>`; every other byte stays."""
    lines = text.split(b"\n")
    out = [lines[0]]
    for line in lines[1:]:
        if not line:
            out.append(line)
            continue
        f = line.split(b",")
        if len(tables) == 1:
            assert f[-2].endswith(b".0"), line
            f[-2] = show(tables[0][int(f[-2][:-2])])
        else:
            index, k = f[-2].split(b"_")
            f[-2] = show(tables[int(k)][int(index)]) + b"_" + k
        out.append(b",".join(f))
    return b"\n".join(out)
