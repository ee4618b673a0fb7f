"""data.read_representation.npy as m6a_prep_sites_write_read_representation writes it (include/m6a.h), stated in plain Python: the
header's bytes, where a row lies, and how the sites are cut into rounds.  m6anet_amd/csrc/m6a_npy.h is the same in C++."""
import struct

N_COLS = 32
DESCR = {"float32": "<f4", "float16": "<f2"}
ITEMSIZE = {"float32": 4, "float16": 2}
GROWTH_AXIS_MAX_DIGITS = 21                 # numpy/lib/format.py: room for the first axis to grow without moving the data
DEFAULT_ROUND_KB = 131072                   # M6A_REPR_ROUND_KB


def header_bytes(n_rows, dtype="float32"):
    """What np.lib.format.open_memmap(path, mode="w+", dtype=dtype, shape=(n_rows, 32)) puts in front of the rows (.npy 1.0)."""
    text = "{'descr': '%s', 'fortran_order': False, 'shape': (%d, %d), }" % (DESCR[dtype], n_rows, N_COLS)
    text += " " * (GROWTH_AXIS_MAX_DIGITS - len(str(n_rows)))
    hlen = len(text) + 1                                            # and the newline
    pad = 64 - ((6 + 2 + 2 + hlen) % 64)                            # 1..64: magic, version and length are 10 bytes
    return b"\x93NUMPY" + b"\x01\x00" + struct.pack("<H", hlen + pad) + text.encode("latin1") + b" " * pad + b"\n"


def row_offset(n_rows, dtype, row):
    return len(header_bytes(n_rows, dtype)) + row * N_COLS * ITEMSIZE[dtype]


def cut_rounds(off, n_sites, round_kb=DEFAULT_ROUND_KB, dtype="float32"):
    """[cut[0] = 0, ..., cut[-1] = n_sites]: round k is sites [cut[k], cut[k + 1]).  A round takes as many sites as together have at
    most max(1, round_kb * 1024 // (32 * itemsize)) rows, and at least one: a site with more rows is a round of its own."""
    per = max(1, round_kb * 1024 // (N_COLS * ITEMSIZE[dtype]))
    cut = [0]
    while cut[-1] < n_sites:
        a = b = cut[-1]
        b += 1
        while b < n_sites and off[b + 1] - off[a] <= per:
            b += 1
        cut.append(b)
    return cut


def n_rounds(off, n_sites, round_kb=DEFAULT_ROUND_KB, dtype="float32"):
    """What the writer reports: the rounds of cut_rounds, or 0 when the sites hold no row."""
    return len(cut_rounds(off, n_sites, round_kb, dtype)) - 1 if off[n_sites] else 0
