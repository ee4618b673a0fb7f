"""How a window size W cuts eventalign.txt into the windows the device parses one at a time (include/m6a.h,
m6a_prep_sites_build_windows), stated in plain Python over tests/eventalign_statement.py's `index` and nothing else.

    window k is data[b:e], b = 0 for the first
    e        the byte after the last newline among the W bytes from b, or len(data) when b + W reaches it
    runs     `index` of the slice: line 0 of the first window is the header, a later window has none
    cut      unless the window is the last, its last run may go on behind e: it is left out and the next window starts with it;
             a window without a run hands on at e
    growth   a window without a newline, or whose only run starts at b, is taken again at 2 W, 4 W, ... from the same b

`index` reads a read index as atoll of the text up to the end of what it is given, so here it stops at e, as on the device.
"""
import eventalign_statement as S


def index_of_window(data, b, e):
    """(names, runs) of data[b:e] with byte offsets of the file.  A window behind the first has no header line: `index` is given
    an empty one."""
    head = b"" if b == 0 else b"\n"
    try:
        names, runs = S.index(head + data[b:e])
    except S.StatementError as err:
        word = "short line at byte "
        if err.text.startswith(word):              # the offset is the file's
            raise S.StatementError(err.code, word + "%d" % (int(err.text[len(word):]) - len(head) + b))
        raise
    for r in runs:
        r["start"] += b - len(head)
        r["end"] += b - len(head)
    return names, runs


def windows(data, W):
    """[dict(b, e, size, names, runs)]: the windows in order, `size` the bytes the window was taken at (W, or W doubled as often as
    it took), `runs` the runs that are the window's own, with `tx` an index into the window's `names`."""
    assert W > 0 and W % 4096 == 0
    n, b, out = len(data), 0, []
    while True:
        size = W
        while True:
            last = b + size >= n
            e = n if last else data.rfind(b"\n", b, b + size) + 1
            if not last and e == 0:                # no newline in it
                size *= 2
                continue
            names, runs = index_of_window(data, b, e)
            if last:
                keep, nxt = runs, n
            elif not runs:
                keep, nxt = [], e
            else:
                keep, nxt = runs[:-1], runs[-1]["start"]
                if nxt == b:                       # its only run, from its first byte
                    size *= 2
                    continue
            break
        out.append(dict(b=b, e=e, size=size, names=names, runs=keep))
        if last:
            return out
        b = nxt


def runs_of_windows(wins):
    """The runs of all windows as `index` of the whole file gives them: names interned by their bytes across the windows."""
    names, ids, runs = [], {}, []
    for w in wins:
        for r in w["runs"]:
            name = w["names"][r["tx"]]
            if name not in ids:
                ids[name] = len(names)
                names.append(name)
            runs.append(dict(tx=ids[name], read=r["read"], start=r["start"], end=r["end"]))
    return names, runs
