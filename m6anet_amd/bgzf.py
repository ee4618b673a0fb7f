"""BGZF (SAM specification section 4.1; include/m6a.h states what this package reads): the writer behind
`python -m m6anet_amd bgzip` and tools/measure_eventalign_inference.py --bgzf, for users without htslib, and the check by content
that `eventalign_inference` makes before it treats a file as compressed.  Python's zlib; no code of the readers is here."""
import os
import struct
import zlib

BLOCK_INPUT = 0xff00                 # input bytes per block, as htslib's bgzip cuts them
EOF_MARKER = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")       # the specification's 28 bytes


def block(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, extra_before=b"", extra_after=b""):
    """one BGZF block holding `data` (at most 65536 bytes); extra_before / extra_after: whole extra subfields around BC"""
    assert len(data) <= 65536
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    body = c.compress(data) + c.flush()
    return wrap(body, zlib.crc32(data), len(data), extra_before, extra_after)


def wrap(deflate, crc, isize, extra_before=b"", extra_after=b""):
    """a raw deflate stream as a BGZF block: header with BSIZE, the stream, CRC32 and ISIZE"""
    xlen = len(extra_before) + 6 + len(extra_after)
    total = 12 + xlen + len(deflate) + 8
    if total > 65536:
        raise ValueError("a BGZF block of %d bytes" % total)
    head = b"\x1f\x8b\x08\x04" + b"\0\0\0\0" + b"\0\xff" + struct.pack("<H", xlen)
    return (head + extra_before + b"BC" + struct.pack("<HH", 2, total - 1) + extra_after + deflate
            + struct.pack("<II", crc & 0xffffffff, isize))


def compress(data, level=6, block_input=BLOCK_INPUT):
    """the whole of `data` as BGZF blocks and the end-of-file marker"""
    return b"".join(block(data[i:i + block_input], level) for i in range(0, len(data), block_input)) + EOF_MARKER


def _span(args):
    path, start, size, level = args
    with open(path, "rb") as f:
        f.seek(start)
        data = f.read(size)
    return b"".join(block(data[i:i + BLOCK_INPUT], level) for i in range(0, len(data), BLOCK_INPUT))


def compress_file(path, out_path=None, level=6, n_processes=1, span_blocks=4096, threads=False):
    """path -> out_path (default path + ".gz"): blocks of BLOCK_INPUT input bytes, then the marker; spans of span_blocks blocks are
    compressed by n_processes processes (threads=True: threads of this process; zlib releases the interpreter lock) and written in
    order.  Returns (input bytes, output bytes)."""
    out_path = out_path or path + ".gz"
    n = os.path.getsize(path)
    span = span_blocks * BLOCK_INPUT
    jobs = [(path, s, min(span, n - s), level) for s in range(0, n, span)]
    written = 0
    with open(out_path, "wb") as out:
        if n_processes > 1 and len(jobs) > 1:
            import multiprocessing as mp
            import multiprocessing.pool
            with (mp.pool.ThreadPool(n_processes) if threads else mp.get_context("spawn").Pool(n_processes)) as pool:
                for part in pool.imap(_span, jobs):
                    out.write(part)
                    written += len(part)
        else:
            for j in jobs:
                part = _span(j)
                out.write(part)
                written += len(part)
        out.write(EOF_MARKER)
    return n, written + len(EOF_MARKER)


def is_gzip(path):
    with open(path, "rb") as f:
        return f.read(2) == b"\x1f\x8b"


def is_bgzf(path):
    """by content, never by name: the first member meets the block header rules (1f 8b 08 04, a BC subfield of two bytes among the
    extra subfields)"""
    with open(path, "rb") as f:
        h = f.read(12)
        if len(h) < 12 or h[:4] != b"\x1f\x8b\x08\x04":
            return False
        xlen = struct.unpack("<H", h[10:12])[0]
        x = f.read(xlen)
    if len(x) < xlen:
        return False
    q, found = 0, False
    while q + 4 <= xlen:
        slen = struct.unpack("<H", x[q + 2:q + 4])[0]
        if q + 4 + slen > xlen:
            return False
        found = found or (x[q:q + 2] == b"BC" and slen == 2)
        q += 4 + slen
    return q == xlen and found
