"""BGZF as `eventalign_inference` reads it (include/m6a.h), in plain Python: the walk of the block chain (SAM specification 4.1)
and an RFC 1951 inflate, block by block.  inflate_file(data) returns (text, blocks) or raises Bad(offset of the first bad block in
file order, reason); blocks[i] says where block i stands, which deflate block types it holds and its largest distance and match
length, so that a fixture can prove it reaches the edge it is named for.  Shares no code with m6a_bgzf.h or m6anet_amd/bgzf.py."""
import zlib

REASONS = ("bad header", "BSIZE runs past the end of the file", "ISIZE over 65536", "deflate block type 3", "stored LEN/NLEN mismatch",
           "invalid code lengths", "invalid literal/length or distance symbol", "distance reaches before the block's output",
           "output beyond ISIZE", "input exhausted before the end-of-block code", "deflate stream does not end at the footer",
           "inflated length is not ISIZE", "CRC-32 mismatch")
(HEADER, BSIZE, ISIZE, BTYPE, STORED, CODELEN, SYMBOL, DISTANCE, OVERFLOW, INPUT, TRAILING, LENGTH, CRC) = REASONS
ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
LBASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LEXT = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
DBASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289,
         16385, 24577)
DEXT = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)


class Bad(Exception):
    def __init__(self, offset, reason):
        super().__init__("BGZF block at byte %d: %s" % (offset, reason))
        self.offset, self.reason = offset, reason


class Refused(Exception):
    """a deflate stream's own error: the reason"""


class Bits:
    def __init__(self, data):
        self.data, self.pos, self.buf, self.cnt = data, 0, 0, 0

    def get(self, need):
        while self.cnt < need:
            if self.pos >= len(self.data):
                raise Refused(INPUT)
            self.buf |= self.data[self.pos] << self.cnt
            self.pos += 1
            self.cnt += 8
        v = self.buf & ((1 << need) - 1)
        self.buf >>= need
        self.cnt -= need
        return v


def code_of(lengths):
    """canonical Huffman code of a set of lengths: ({(length, code): symbol}, left, longest); left > 0: incomplete, < 0: over-subscribed"""
    count = [0] * 16
    for n in lengths:
        count[n] += 1
    longest = max((n for n in range(1, 16) if count[n]), default=0)
    if longest == 0:
        return {}, 0, 0
    left = 1
    for n in range(1, 16):
        left = 2 * left - count[n]
        if left < 0:
            return {}, left, longest
    table, code = {}, 0
    for n in range(1, 16):
        for sym, m in enumerate(lengths):
            if m == n:
                table[(n, code)] = sym
                code += 1
        code <<= 1
    return table, left, longest


def accepted(left, longest, code_length_code=False):
    """zlib's verdict on a set: never over-subscribed; incomplete only as one code of one bit, and never for the code-length code"""
    return left == 0 or (left > 0 and not code_length_code and longest == 1)


def symbol(bits, table):
    code = 0
    for n in range(1, 16):
        code |= bits.get(1)
        if (n, code) in table:
            return table[(n, code)]
        code <<= 1
    return -1


def dynamic(bits):
    nlen, ndist, ncode = bits.get(5) + 257, bits.get(5) + 1, bits.get(4) + 4
    if nlen > 286 or ndist > 30:
        raise Refused(CODELEN)
    cl = [0] * 19
    for i in range(ncode):
        cl[ORDER[i]] = bits.get(3)
    table, left, longest = code_of(cl)
    if longest == 0 or not accepted(left, longest, True):
        raise Refused(CODELEN)
    lengths = []
    while len(lengths) < nlen + ndist:
        s = symbol(bits, table)
        if s < 0:
            raise Refused(CODELEN)
        if s < 16:
            lengths.append(s)
            continue
        if s == 16:
            if not lengths:
                raise Refused(CODELEN)
            v, rep = lengths[-1], 3 + bits.get(2)
        elif s == 17:
            v, rep = 0, 3 + bits.get(3)
        else:
            v, rep = 0, 11 + bits.get(7)
        if len(lengths) + rep > nlen + ndist:
            raise Refused(CODELEN)
        lengths += [v] * rep
    if lengths[256] == 0:
        raise Refused(CODELEN)
    dt, left, longest = code_of(lengths[nlen:])
    if not accepted(left, longest):
        raise Refused(CODELEN)
    lt, left, longest = code_of(lengths[:nlen])
    if not accepted(left, longest):
        raise Refused(CODELEN)
    return lt, dt


FIXED = (code_of([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8)[0], code_of([5] * 30)[0])


def inflate(data, isize):
    """(output, types, largest distance, largest match length) of one raw deflate stream that must fill `data` and give isize bytes"""
    bits, out, types, far, longest = Bits(data), bytearray(), [], 0, 0
    last = 0
    while not last:
        last, kind = bits.get(1), bits.get(2)
        types.append(kind)
        if kind == 3:
            raise Refused(BTYPE)
        if kind == 0:
            bits.buf = bits.cnt = 0
            if bits.pos + 4 > len(data):
                raise Refused(INPUT)
            n, c = int.from_bytes(data[bits.pos:bits.pos + 2], "little"), int.from_bytes(data[bits.pos + 2:bits.pos + 4], "little")
            if n ^ 0xffff != c:
                raise Refused(STORED)
            bits.pos += 4
            if bits.pos + n > len(data):
                raise Refused(INPUT)
            if len(out) + n > isize:
                raise Refused(OVERFLOW)
            out += data[bits.pos:bits.pos + n]
            bits.pos += n
            continue
        lt, dt = FIXED if kind == 1 else dynamic(bits)
        while True:
            s = symbol(bits, lt)
            if s < 0:
                raise Refused(SYMBOL)
            if s < 256:
                if len(out) >= isize:
                    raise Refused(OVERFLOW)
                out.append(s)
                continue
            if s == 256:
                break
            if s > 285:
                raise Refused(SYMBOL)
            n = LBASE[s - 257] + bits.get(LEXT[s - 257])
            d = symbol(bits, dt)
            if d < 0 or d > 29:
                raise Refused(SYMBOL)
            dist = DBASE[d] + bits.get(DEXT[d])
            if dist > len(out):
                raise Refused(DISTANCE)
            if len(out) + n > isize:
                raise Refused(OVERFLOW)
            for _ in range(n):
                out.append(out[-dist])
            far, longest = max(far, dist), max(longest, n)
    if bits.pos != len(data):
        raise Refused(TRAILING)
    if len(out) != isize:
        raise Refused(LENGTH)
    return bytes(out), types, far, longest


def header(data, at):
    """(header bytes, total bytes) of the block at `at`, or the reason it has none"""
    h = data[at:at + 12]
    if len(h) < 12 or h[:4] != b"\x1f\x8b\x08\x04":
        return HEADER
    end = 12 + int.from_bytes(h[10:12], "little")
    x = data[at:at + end]
    if len(x) < end:
        return HEADER
    q, bsize = 12, None
    while q + 4 <= end:
        slen = int.from_bytes(x[q + 2:q + 4], "little")
        if q + 4 + slen > end:
            return HEADER
        if x[q:q + 2] == b"BC" and slen == 2 and bsize is None:
            bsize = int.from_bytes(x[q + 4:q + 6], "little")
        q += 4 + slen
    if q != end or bsize is None or bsize + 1 < end + 8:
        return HEADER
    if at + bsize + 1 > len(data):
        return BSIZE
    return end, bsize + 1


def is_gzip(data):
    return data[:2] == b"\x1f\x8b"


def is_bgzf(data):
    return header(data, 0) not in (HEADER,)


def inflate_file(data):
    text, blocks, at = bytearray(), [], 0
    while at < len(data):
        h = header(data, at)
        if isinstance(h, str):
            raise Bad(at, h)
        hdr, total = h
        isize = int.from_bytes(data[at + total - 4:at + total], "little")
        if isize > 65536:
            raise Bad(at, ISIZE)
        try:
            out, types, far, longest = inflate(data[at + hdr:at + total - 8], isize)
        except Refused as e:
            raise Bad(at, e.args[0])
        if zlib.crc32(out) != int.from_bytes(data[at + total - 8:at + total - 4], "little"):
            raise Bad(at, CRC)
        blocks.append(dict(offset=at, total=total, isize=isize, types=types, distance=far, length=longest))
        text += out
        at += total
    return bytes(text), blocks
