"""ctypes binding of libm6a_io.so (include/m6a_io.h): native loader + CSV writers."""
import ctypes as C
import os

import numpy as np

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("M6A_IO_LIB") or os.path.join(_PKG, "libm6a_io.so")   # M6A_IO_LIB: e.g. the sanitizer build (tests/sanitize.sh)
SYMBOLS = ["m6a_io_last_error", "m6a_io_load_sites", "m6a_io_free", "m6a_io_n_sites", "m6a_io_n_reads",
           "m6a_io_n_replicates", "m6a_io_X", "m6a_io_site_kmers", "m6a_io_off", "m6a_io_tx_pos",
           "m6a_io_read_ids", "m6a_io_read_rep", "m6a_io_tx_id", "m6a_io_kmer5", "m6a_io_write_csv", "m6a_io_write_csv_n", "m6a_io_csv_shard_size", "m6a_io_csv_shard_write", "m6a_io_csv_header_bytes", "m6a_io_format_f16", "m6a_io_py_repr", "m6a_io_repr_rounded", "m6a_io_repr_core",
           "m6a_io_save_store", "m6a_io_open_store", "m6a_io_store_tag", "m6a_io_dataprep", "m6a_io_dataprep_rows", "m6a_io_rows_table",
           "m6a_io_rows_free", "m6a_io_dataprep_write", "m6a_io_runs_rows", "m6a_io_sites_from_arrays", "m6a_io_sites_from_arrays_rep", "m6a_io_sites_set_read_names", "m6a_io_uuid_parse", "m6a_io_uuid_format", "m6a_io_bgzf_inflate", "m6a_io_bgzf_deflate", "m6a_io_bgzf_deflate_level",
           "m6a_io_info_open", "m6a_io_info_get", "m6a_io_info_free", "m6a_io_info_rows", "m6a_io_json_walk",
           "m6a_io_norm_factors", "m6a_io_norm_partials", "m6a_io_site_ranksum", "m6a_io_site_signal_ranksum", "m6a_io_site_ks",
           "m6a_io_site_signal_ks", "m6a_io_ks_exact"]
_lib = None


class PrepTable(C.Structure):
    """m6a_io_prep_table (include/m6a_io.h): the runs and candidate rows of a dataprep, as plain arrays."""
    _fields_ = [("n_neighbors", C.c_int), ("n_tx", C.c_int64), ("tx_blob", C.c_void_p), ("tx_off", C.c_void_p),
                ("n_runs", C.c_int64), ("run_tx", C.c_void_p), ("run_read", C.c_void_p), ("run_start", C.c_void_p),
                ("run_end", C.c_void_p), ("run_npos", C.c_void_p), ("run_status", C.c_void_p), ("row_off", C.c_void_p),
                ("n_rows", C.c_int64), ("row_pos", C.c_void_p), ("row_kmer", C.c_void_p), ("row_feat", C.c_void_p)]


class InfoTable(C.Structure):
    """m6a_io_info_table (include/m6a_io.h): data.info after the min_reads filter."""
    _fields_ = [("n_sites", C.c_int64), ("n_reads", C.c_int64), ("n_tx", C.c_int64), ("site_tx", C.c_void_p), ("pos", C.c_void_p),
                ("start", C.c_void_p), ("end", C.c_void_p), ("site_reads", C.c_void_p), ("tx_blob", C.c_void_p), ("tx_off", C.c_void_p)]


def table_arrays(t):
    """Copies of a PrepTable's arrays as numpy: names, runs (tx, read, start, end, npos, status), row_off, rows (pos, kmer, feat)."""
    def arr(ptr, ctype, n):
        return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(ctype)), shape=(n,)).copy() if n else np.zeros(0, np.dtype(ctype))
    nt, nr, nrow = t.n_tx, t.n_runs, t.n_rows
    K, NF = 5 + 2 * t.n_neighbors, 3 * (2 * t.n_neighbors + 1)
    tx_off = arr(t.tx_off, C.c_int64, nt + 1)
    blob = C.string_at(t.tx_blob, int(tx_off[-1])) if nt else b""
    return dict(names=[blob[tx_off[i]:tx_off[i + 1]].decode() for i in range(nt)],
                run_tx=arr(t.run_tx, C.c_uint32, nr), run_read=arr(t.run_read, C.c_int64, nr), run_start=arr(t.run_start, C.c_int64, nr),
                run_end=arr(t.run_end, C.c_int64, nr), run_npos=arr(t.run_npos, C.c_int64, nr), run_status=arr(t.run_status, C.c_int32, nr),
                row_off=arr(t.row_off, C.c_int64, nr + 1) if nr else np.zeros(1, np.int64), row_pos=arr(t.row_pos, C.c_int64, nrow),
                row_kmer=arr(t.row_kmer, C.c_uint8, nrow * K).reshape(nrow, K), row_feat=arr(t.row_feat, C.c_double, nrow * NF).reshape(nrow, NF))


class M6AIOError(RuntimeError):
    """`code` = the M6A_IO_E* value the call returned (include/m6a_io.h: -1 EINVAL, -2 ENOMEM, -3 EIO, -4 EFORMAT)."""

    def __init__(self, msg, code=None):
        super().__init__(msg)
        self.code = code


def load():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError("libm6a_io.so is not built: run `python -m m6anet_amd.build`")
    L = C.CDLL(LIB_PATH)
    vp, i64, i32 = C.c_void_p, C.c_int64, C.c_int
    L.m6a_io_last_error.restype = C.c_char_p
    L.m6a_io_load_sites.argtypes = [C.POINTER(C.c_char_p), i32, i32, C.c_char_p, vp, vp, i32, i32, C.POINTER(vp)]
    L.m6a_io_free.argtypes = [vp]
    L.m6a_io_free.restype = None
    for name, rt in (("m6a_io_n_sites", i64), ("m6a_io_n_reads", i64), ("m6a_io_n_replicates", i32)):
        getattr(L, name).argtypes = [vp]
        getattr(L, name).restype = rt
    for name in ("m6a_io_X", "m6a_io_site_kmers", "m6a_io_off", "m6a_io_tx_pos", "m6a_io_read_ids", "m6a_io_read_rep"):
        getattr(L, name).argtypes = [vp]
        getattr(L, name).restype = vp
    for name in ("m6a_io_tx_id", "m6a_io_kmer5"):
        getattr(L, name).argtypes = [vp, i64]
        getattr(L, name).restype = C.c_char_p
    L.m6a_io_write_csv.argtypes = [vp, C.c_char_p, vp, vp, vp, i32, i32]
    L.m6a_io_write_csv_n.argtypes = [vp, C.c_char_p, vp, vp, vp, i32, i32, i64]
    L.m6a_io_csv_shard_size.argtypes = [vp, vp, vp, vp, i64, i64, i32, C.POINTER(i64), C.POINTER(i64)]
    L.m6a_io_csv_shard_write.argtypes = [vp, C.c_char_p, vp, vp, vp, i64, i64, i32, i64, i64, i32, i64, i64]
    L.m6a_io_csv_header_bytes.argtypes = [i32]
    L.m6a_io_csv_header_bytes.restype = i64
    L.m6a_io_format_f16.argtypes = [C.c_double, C.c_char_p]
    L.m6a_io_format_f16.restype = i32
    L.m6a_io_py_repr.argtypes = [C.c_double, C.c_char_p]
    L.m6a_io_py_repr.restype = i32
    L.m6a_io_repr_rounded.argtypes = [C.c_double, i32, C.c_char_p]
    L.m6a_io_repr_rounded.restype = i32
    L.m6a_io_repr_core.argtypes = [C.c_double, i32, C.c_char_p]
    L.m6a_io_repr_core.restype = i32
    L.m6a_io_save_store.argtypes = [vp, C.c_char_p, C.c_char_p]
    L.m6a_io_open_store.argtypes = [C.c_char_p, C.POINTER(vp)]
    L.m6a_io_store_tag.argtypes = [vp]
    L.m6a_io_store_tag.restype = C.c_char_p
    L.m6a_io_dataprep.argtypes = [C.c_char_p, C.c_char_p, i32, i32, i32, i32, i32, i32, i32]
    L.m6a_io_dataprep_rows.argtypes = [C.c_char_p, C.c_char_p, i32, i32, C.POINTER(vp)]
    L.m6a_io_rows_table.argtypes = [vp]
    L.m6a_io_rows_table.restype = C.POINTER(PrepTable)
    L.m6a_io_rows_free.argtypes = [vp]
    L.m6a_io_rows_free.restype = None
    L.m6a_io_dataprep_write.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(PrepTable), i32, i32, i32, i32, i32, i32]
    L.m6a_io_runs_rows.argtypes = [C.c_char_p, i64, vp, vp, vp, i32, i32, C.POINTER(vp)]
    L.m6a_io_sites_from_arrays.argtypes = [i64, vp, vp, C.c_char_p, vp, i64, vp, C.c_char_p, vp, C.POINTER(vp)]
    L.m6a_io_sites_from_arrays_rep.argtypes = [i64, vp, vp, C.c_char_p, vp, i64, vp, C.c_char_p, vp, vp, i32, C.POINTER(vp)]
    L.m6a_io_sites_set_read_names.argtypes = [vp, vp, vp, i32]
    L.m6a_io_uuid_parse.argtypes = [C.c_char_p, i64, vp]
    L.m6a_io_uuid_format.argtypes = [vp, vp]
    L.m6a_io_uuid_format.restype = None
    L.m6a_io_bgzf_inflate.argtypes = [C.c_char_p, vp, i64, C.POINTER(i64)]
    L.m6a_io_bgzf_deflate.argtypes = [C.c_char_p, i64, vp, i64, C.POINTER(i64), C.POINTER(i64)]
    L.m6a_io_bgzf_deflate_level.argtypes = [C.c_char_p, i64, i32, vp, i64, C.POINTER(i64), C.POINTER(i64)]
    L.m6a_io_info_open.argtypes = [C.c_char_p, i32, C.POINTER(vp)]
    L.m6a_io_info_get.argtypes = [vp]
    L.m6a_io_info_get.restype = C.POINTER(InfoTable)
    L.m6a_io_info_free.argtypes = [vp]
    L.m6a_io_info_free.restype = None
    L.m6a_io_info_rows.argtypes = [vp, vp, i64, C.c_char_p, vp, vp, i32, i32, vp, vp, vp, vp]
    L.m6a_io_json_walk.argtypes = [C.c_char_p, i64, C.c_char_p, i64, i64, C.c_char_p, i32, vp, C.c_char_p]
    L.m6a_io_norm_factors.argtypes = [C.c_char_p, i64, vp, vp, vp, vp, vp, vp, i32, vp, vp, vp, vp, vp, vp, C.POINTER(i64), vp]
    L.m6a_io_norm_partials.argtypes = [C.c_char_p, i64, vp, vp, vp, vp, vp, vp, vp, i64, i32, vp, vp, vp]
    L.m6a_io_site_ranksum.argtypes = [vp, vp, i64, vp, vp, i64, vp, vp, i64, vp, vp, vp, vp, i32]
    L.m6a_io_site_signal_ranksum.argtypes = [vp, vp, i64, vp, vp, i64, vp, vp, i64, vp, vp, vp, vp, i32]
    L.m6a_io_site_ks.argtypes = [vp, vp, i64, vp, vp, i64, vp, vp, i64, vp, vp, vp, vp, i32]
    L.m6a_io_site_signal_ks.argtypes = [vp, vp, i64, vp, vp, i64, vp, vp, i64, vp, vp, vp, vp, i32]
    L.m6a_io_ks_exact.argtypes = [vp, vp, vp, i64, vp]
    _lib = L
    return L


def usable_cpus():
    """CPUs this process may really use: the affinity mask cut by the cgroup quota (the GPU boxes lease 16 of 256)."""
    try:
        n = len(os.sched_getaffinity(0))
    except (AttributeError, OSError):
        n = os.cpu_count() or 1
    try:
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if q != "max":
            n = min(n, max(1, int(float(q) / float(per) + 0.999)))
    except (OSError, ValueError):
        pass
    return max(1, n)


def _chk(rc):
    if rc != 0:
        raise M6AIOError("m6a_io error %d: %s" % (rc, load().m6a_io_last_error().decode()), rc)


def ks_exact(n, m, h):
    """m6a_io_ks_exact: the exact two-sided Kolmogorov-Smirnov p-value of every item (n, m, h) on the host, the bits m6a_ks_exact gives
    on a device (include/m6a.h states the recurrence and what is undefined, NaN).  Integer arrays of one size -> float64 of their shape."""
    shape = np.shape(n)
    n, m, h = (np.ascontiguousarray(np.asarray(x).ravel(), np.int64) for x in (n, m, h))
    if not n.size == m.size == h.size:
        raise ValueError("n, m and h must have one entry per item")
    p = np.empty(n.size, np.float64)
    _chk(load().m6a_io_ks_exact(n.ctypes.data, m.ctypes.data, h.ctypes.data, n.size, p.ctypes.data))
    return p.reshape(shape)


def dataprep(eventalign, out_dir, n_threads=0, readcount_min=1, readcount_max=1000, min_segment_count=20,
             n_neighbors=1, compress=False, skip_index=False, device="cpu", device_id=0, writer="host", stats=None):
    """Native `m6anet dataprep` (m6anet/scripts/dataprep.py:54-70).  device="gpu": the line scan, parse, combine and windows run
    in HIP (m6a_prep_eventalign, include/m6a.h) and the host writes the same four files from their table
    (m6a_io_dataprep_write); a file larger than the device budget is an error, never a silent host run.
    writer="device" (with device="gpu", n_neighbors=1 and no skip_index; anything else is a ValueError before a file is touched):
    m6a_prep_dataprep_write -- the back half runs on the device as well and the four files are formatted there, byte for byte the
    host writer's.  Where the device's number printer declines a value (include/m6a.h) nothing has been written: one line goes to
    stderr and the files are written by the writer="host" route from the start.  `stats`: a dict that receives the
    m6a_dataprep_stats fields and `writer`, "device" or "host" -- which one wrote the files; M6A_DATAPREP_TIMES=1 prints them as one
    `M6A_TIMES {json}` line on stderr."""
    if device not in ("cpu", "gpu"):
        raise ValueError("device must be 'cpu' or 'gpu', not %r" % (device,))
    if writer not in ("host", "device"):
        raise ValueError("writer must be 'host' or 'device', not %r" % (writer,))
    if writer == "device":
        conflict = dataprep_writer_conflict(device, skip_index, n_neighbors)
        if conflict:
            raise ValueError(conflict)
    os.makedirs(out_dir, exist_ok=True)
    if device == "cpu":
        _chk(load().m6a_io_dataprep(os.fsencode(eventalign), os.fsencode(out_dir), int(n_threads), int(readcount_min),
                                    int(readcount_max), int(min_segment_count), int(n_neighbors), 1 if compress else 0,
                                    1 if skip_index else 0))
        return
    if writer == "device":
        st = _dataprep_on_device(eventalign, out_dir, n_threads, readcount_min, readcount_max, min_segment_count, compress, device_id)
        if st["writer"] == "host":
            import sys
            print("dataprep: --writer device declined %d values; writing on the host" % st["n_declined"], file=sys.stderr)
        if stats is not None:
            stats.update(st)
        if os.environ.get("M6A_DATAPREP_TIMES") == "1":
            import json
            import sys
            print("M6A_TIMES " + json.dumps(st), file=sys.stderr)
        if st["writer"] == "device":
            return
    with prep_on_device(eventalign, n_neighbors, os.path.join(out_dir, "eventalign.index") if skip_index else None, device_id) as table:
        write_table(eventalign, out_dir, table, n_threads, readcount_min, readcount_max, min_segment_count, compress, not skip_index)


def dataprep_writer_conflict(device, skip_index, n_neighbors):
    """What `--writer device` cannot be combined with: the text of the argument error, naming the flag, or None."""
    if device != "gpu":
        return "--writer device formats the files on the GPU and conflicts with --device cpu: give --device gpu"
    if skip_index:
        return "--writer device writes eventalign.index itself and conflicts with --skip_index"
    if int(n_neighbors) != 1:
        return "--writer device prints one neighbour either side and conflicts with --n_neighbors %d: only --n_neighbors 1" % int(n_neighbors)
    return None


def _dataprep_on_device(eventalign, out_dir, n_threads, readcount_min, readcount_max, min_segment_count, compress, device_id):
    """m6a_prep_dataprep_write: the statistics as a dict, with `writer` = "device", or "host" where values were declined (nothing
    written then).  Errors are M6AIOError with the host path's code."""
    from . import _lib
    L, io = _lib.load(), load()
    host = _lib.HostHalf(C.cast(io.m6a_io_runs_rows, C.c_void_p), C.cast(io.m6a_io_rows_table, C.c_void_p),
                         C.cast(io.m6a_io_rows_free, C.c_void_p), C.cast(io.m6a_io_last_error, C.c_void_p))
    st = _lib.DataprepStats()
    rc = L.m6a_prep_dataprep_write(int(device_id), os.fsencode(eventalign), os.fsencode(out_dir), int(readcount_min), int(readcount_max),
                                   int(min_segment_count), 1 if compress else 0, C.byref(host), int(n_threads), C.byref(st))
    out = {k: getattr(st, k) for k, _ in st._fields_}
    out["writer"] = "host" if rc == _lib.M6A_EDECLINED else "device"
    if rc not in (0, _lib.M6A_EDECLINED):
        raise M6AIOError("m6a_prep error %d: %s" % (rc, L.m6a_prep_last_error().decode()), prep_on_device._CODES.get(rc, rc))
    return out


def repr_format(values, round3=False, device_id=0):
    """m6a_repr_format (libm6a_hip.so): repr(float) of every value -- of np.round(v, 3) with round3 -- printed on the device by the
    core the data.json writer uses.  Returns (text, off, n_declined): value i is text[off[i]:off[i + 1]], empty where declined."""
    from . import _lib
    L = _lib.load()
    v = np.ascontiguousarray(values, np.float64)
    off, nd = np.zeros(v.size + 1, np.int64), C.c_int64()

    def call(buf, cap):
        rc = L.m6a_repr_format(int(device_id), v.ctypes.data, v.size, 1 if round3 else 0, buf, cap, off.ctypes.data, C.byref(nd))
        if rc != 0:
            raise M6AIOError("m6a_prep error %d: %s" % (rc, L.m6a_prep_last_error().decode()), prep_on_device._CODES.get(rc, rc))
    call(None, 0)
    buf = C.create_string_buffer(max(1, int(off[-1])))
    call(buf, int(off[-1]))
    return buf.raw[:int(off[-1])], off, nd.value


def write_table(eventalign, out_dir, table, n_threads=0, readcount_min=1, readcount_max=1000, min_segment_count=20, compress=False,
                write_index=True):
    """m6a_io_dataprep_write: the four files from a PrepTable (a pointer to one, or the structure)."""
    os.makedirs(out_dir, exist_ok=True)
    ptr = table if isinstance(table, C._Pointer) else C.pointer(table)
    _chk(load().m6a_io_dataprep_write(os.fsencode(eventalign), os.fsencode(out_dir), ptr, int(n_threads), int(readcount_min),
                                      int(readcount_max), int(min_segment_count), 1 if compress else 0, 1 if write_index else 0))


class host_rows:
    """m6a_io_dataprep_rows as a context manager: yields the table (a pointer to PrepTable), freed on exit."""

    def __init__(self, eventalign, n_neighbors=1, index_path=None, n_threads=0):
        L = load()
        self._h = C.c_void_p()
        _chk(L.m6a_io_dataprep_rows(os.fsencode(eventalign), None if index_path is None else os.fsencode(index_path), int(n_threads),
                                    int(n_neighbors), C.byref(self._h)))
        self.table = L.m6a_io_rows_table(self._h)

    def __enter__(self):
        return self.table

    def __exit__(self, *exc):
        load().m6a_io_rows_free(self._h)
        self._h = None


class prep_on_device:
    """m6a_prep_eventalign (libm6a_hip.so) as a context manager: yields the device-made table, freed on exit.  Errors are
    M6AIOError with the m6a_io code of the same failure on the host path (EFORMAT for a short line, EIO for a missing index)."""
    _CODES = {-1: -1, -2: -2, -7: -4, -8: -3}       # M6A_EFORMAT -> M6A_IO_EFORMAT, M6A_EIO -> M6A_IO_EIO

    def __init__(self, eventalign, n_neighbors=1, index_path=None, device_id=0):
        from . import _lib
        L = _lib.load()
        self._L, self._h = L, C.c_void_p()
        rc = L.m6a_prep_eventalign(int(device_id), os.fsencode(eventalign), int(n_neighbors),
                                   None if index_path is None else os.fsencode(index_path), C.byref(self._h))
        if rc != 0:
            raise M6AIOError("m6a_prep error %d: %s" % (rc, L.m6a_prep_last_error().decode()), self._CODES.get(rc, rc))
        self.table = C.cast(L.m6a_prep_table(self._h), C.POINTER(PrepTable))

    def __enter__(self):
        return self.table

    def __exit__(self, *exc):
        self._L.m6a_prep_free(self._h)
        self._h = None


def is_bgzf(path):
    """True when the file's first bytes are a BGZF block header (by content, never by name); `eventalign_inference` inflates such a
    file on the device."""
    from . import bgzf
    return bgzf.is_bgzf(path)


def bgzf_inflate_host(path):
    """m6a_io_bgzf_inflate: the text of a BGZF file, inflated on the host by the decode core the HIP kernels compile.  M6AIOError
    (EFORMAT) names the first bad block in file order: `<path>: BGZF block at byte <offset>: <reason>`."""
    L, n = load(), C.c_int64()
    _chk(L.m6a_io_bgzf_inflate(os.fsencode(path), None, 0, C.byref(n)))
    buf = C.create_string_buffer(max(1, n.value))
    _chk(L.m6a_io_bgzf_inflate(os.fsencode(path), buf, n.value, C.byref(n)))
    return buf.raw[:n.value]


def bgzf_inflate(path, device_id=0, stats=None):
    """m6a_bgzf_inflate (libm6a_hip.so): the text of a BGZF file, inflated and CRC-checked by the HIP kernels.  Errors as
    bgzf_inflate_host's.  `stats`: a dict that receives the m6a_bgzf_stats fields."""
    from . import _lib
    L, n, st = _lib.load(), C.c_int64(), _lib.BgzfStats()

    def call(buf, cap):
        rc = L.m6a_bgzf_inflate(int(device_id), os.fsencode(path), buf, cap, C.byref(n), C.byref(st))
        if rc != 0:
            raise M6AIOError("m6a_prep error %d: %s" % (rc, L.m6a_prep_last_error().decode()), prep_on_device._CODES.get(rc, rc))
    call(None, 0)
    buf = C.create_string_buffer(max(1, n.value))
    call(buf, n.value)
    if stats is not None:
        stats.update({k: getattr(st, k) for k, _ in st._fields_})
    return buf.raw[:n.value]


def bgzf_deflate_host(data, stats=None, level=1):
    """m6a_io_bgzf_deflate: `data` as BGZF (blocks of at most 65 280 bytes and the end-of-file marker), written on the host by the
    deflate core the HIP kernels compile -- the bytes bgzf_deflate gives.  `stats`: a dict that receives n_stored.
    level: 1 (fixed Huffman codes) through that symbol; anything else goes to m6a_io_bgzf_deflate_level, where 2 is dynamic codes,
    and `stats` receives n_by_type, the blocks of deflate block type 0, 1 and 2, as well."""
    L, n, ns = load(), C.c_int64(), C.c_int64()
    data = bytes(data)
    if level != 1:
        by = (C.c_int64 * 3)()
        _chk(L.m6a_io_bgzf_deflate_level(data, len(data), int(level), None, 0, C.byref(n), None))
        buf = C.create_string_buffer(n.value)
        _chk(L.m6a_io_bgzf_deflate_level(data, len(data), int(level), buf, n.value, C.byref(n), by))
        if stats is not None:
            stats.update(n_stored=by[0], n_by_type=list(by))
        return buf.raw[:n.value]
    _chk(L.m6a_io_bgzf_deflate(data, len(data), None, 0, C.byref(n), None))
    buf = C.create_string_buffer(n.value)
    _chk(L.m6a_io_bgzf_deflate(data, len(data), buf, n.value, C.byref(n), C.byref(ns)))
    if stats is not None:
        stats.update(n_stored=ns.value)
    return buf.raw[:n.value]


def bgzf_deflate(data, device_id=0, stats=None, level=1):
    """m6a_bgzf_deflate (libm6a_hip.so): `data` as BGZF, deflated by the HIP kernels; byte for byte what bgzf_deflate_host gives.
    `stats`: a dict that receives the m6a_deflate_stats fields.  level other than 1: m6a_bgzf_deflate_level (2: dynamic Huffman
    codes), and `stats` receives n_by_type as well."""
    from . import _lib
    L, n, st = _lib.load(), C.c_int64(), _lib.DeflateStats()
    data = bytes(data)
    by = (C.c_int64 * 3)()

    def call(buf, cap):
        if level != 1:
            rc = L.m6a_bgzf_deflate_level(int(device_id), data, len(data), int(level), buf, cap, C.byref(n), C.byref(st), by)
        else:
            rc = L.m6a_bgzf_deflate(int(device_id), data, len(data), buf, cap, C.byref(n), C.byref(st))
        if rc != 0:
            raise M6AIOError("m6a_prep error %d: %s" % (rc, L.m6a_prep_last_error().decode()), prep_on_device._CODES.get(rc, rc))
    call(None, 0)
    buf = C.create_string_buffer(n.value)
    call(buf, n.value)
    if stats is not None:
        stats.update({k: getattr(st, k) for k, _ in st._fields_})
        if level != 1:
            stats.update(n_by_type=list(by))
    return buf.raw[:n.value]


def norm_arrays(norm):
    """Normalisation factors (dict kmer -> (mean[3], std[3]), or None) in m6a_io_load_sites' form: (kmers blob, mean, std, n)."""
    if not norm:
        return None, None, None, 0
    kmers = sorted(norm)
    mean = np.ascontiguousarray([norm[k][0] for k in kmers], np.float64)
    std = np.ascontiguousarray([norm[k][1] for k in kmers], np.float64)
    return "".join(kmers).encode(), mean, std, len(kmers)


class prep_sites:
    """m6a_prep_sites_build (libm6a_hip.so): eventalign.txt -> the loader's arrays with X, site_kmers and off left on the device.
    `eventalign` is one path, or a list of paths that are replicates (m6a_prep_sites_build_multi: pooled on the device as the loader
    pools several input directories; a list of one is a list -- `<id>_0`).  `info` is the m6a_prep_sites_info; host copies are numpy
    arrays (off, site_tx, tx_pos, kmer7, read_ids, read_rep) and `names` (per transcript); n_replicates and peak_bytes as reported.
    window_kb: parse each file in windows of that many KB instead of keeping it resident (m6a_prep_sites_build_windows; the arrays
    are the same), 0 for resident, None for what M6A_PREP_WINDOW_KB says; n_windows and window_bytes say what was done.  A file that
    is BGZF (by content) is inflated on the device and gives the arrays of its text; n_bgzf_blocks, compressed_bytes and ms_inflate
    say so (0 for plain files), and windows over such a file are refused.  read_names=True (m6a_prep_sites_build_names): field 4 of
    every file is the read's UUID (nanopolish / f5c --print-read-names), not an index; the arrays are those of the twin file whose
    names are replaced by 0, 1, ... in order of first appearance, read_ids holds those indices, and `read_names` is (names, offsets):
    names uint8 [n][16] -- the UUIDs' bytes, file f's in index order at rows [offsets[f], offsets[f + 1]) -- and offsets int64
    [n_replicates + 1]; None without the flag.  n_read_names and ms_intern count the names and the interning.  A path `-` is the
    standard input, and any path that is not a regular file (a FIFO, /dev/fd/N) is a stream: it is read once, in order, always in
    windows (window_kb, M6A_PREP_WINDOW_KB, or 256 MB), and gives the arrays, n_windows and window_bytes of a regular file with the
    same bytes at the same window size; stream_bytes and n_streams say so (0 for regular files).  Nothing here asks a path for its
    size or whether it exists: the library opens it.  Errors are M6AIOError with the code of the same failure on the two-step path; close() frees the device arrays."""
    _CODES = prep_on_device._CODES

    def __init__(self, eventalign, readcount_min=1, readcount_max=1000, min_segment_count=20, norm=None, n_threads=0, device_id=0,
                 window_kb=None, read_names=False):
        if window_kb is not None and window_kb < 0:
            raise ValueError("window_kb must be 0 or more, not %r" % (window_kb,))
        from . import _lib
        L, io = _lib.load(), load()
        self._L, self._h = L, C.c_void_p()
        blob, mean, std, n = norm_arrays(norm)
        host = _lib.HostHalf(C.cast(io.m6a_io_runs_rows, C.c_void_p), C.cast(io.m6a_io_rows_table, C.c_void_p),
                             C.cast(io.m6a_io_rows_free, C.c_void_p), C.cast(io.m6a_io_last_error, C.c_void_p))
        tail = (int(readcount_min), int(readcount_max), int(min_segment_count), blob, None if mean is None else mean.ctypes.data,
                None if std is None else std.ctypes.data, n, C.byref(host), int(n_threads))
        if isinstance(eventalign, (str, bytes, os.PathLike)) and window_kb is None and not read_names:
            rc = L.m6a_prep_sites_build(int(device_id), os.fsencode(eventalign), *tail, C.byref(self._h))
        else:                                # one path with a window size: the one-file job, asked through the list's entry point
            one = isinstance(eventalign, (str, bytes, os.PathLike))
            paths = [os.fsencode(e) for e in ([eventalign] if one else eventalign)]
            head = (int(device_id), (C.c_char_p * len(paths))(*paths), len(paths), *tail, -1 if window_kb is None else int(window_kb) << 10)
            rc = L.m6a_prep_sites_build_names(*head, 1, C.byref(self._h)) if read_names else L.m6a_prep_sites_build_windows(*head, C.byref(self._h))
        if rc != 0:
            raise M6AIOError("m6a_prep error %d: %s" % (rc, L.m6a_prep_last_error().decode()), self._CODES.get(rc, rc))
        self._adopt()

    def _adopt(self):
        """the host copies and counters of the handle in self._h"""
        L = self._L
        i = self.info = L.m6a_prep_sites_get(self._h).contents
        S, R, T = i.n_sites, i.n_reads, i.n_tx

        def arr(ptr, ctype, n):
            return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(ctype)), shape=(n,)).copy() if n else np.zeros(0, np.dtype(ctype))
        self.n_sites, self.n_reads = S, R
        self.off = arr(i.off_host, C.c_int64, S + 1)
        self.site_tx = arr(i.site_tx, C.c_uint32, S)
        self.tx_pos = arr(i.site_pos, C.c_int64, S)
        self.kmer7 = arr(i.site_kmer7, C.c_uint8, 7 * S).reshape(S, 7)
        self.read_ids = arr(i.read_ids, C.c_double, R)
        self.read_rep = arr(i.read_rep, C.c_int32, R)
        self.n_replicates, self.peak_bytes = int(i.n_rep), int(i.peak_bytes)
        self.n_windows, self.window_bytes = int(i.n_windows), int(i.window_bytes)
        self.n_bgzf_blocks, self.compressed_bytes, self.ms_inflate = int(i.n_bgzf_blocks), int(i.compressed_bytes), float(i.ms_inflate)
        self.n_declined_sites = int(i.n_declined_sites)      # json_sites: sites that went through the host half
        # streams (`-`, a FIFO, /dev/fd/N): the bytes read from them, and how many of the files were streams; 0 for regular files
        self.stream_bytes, self.n_streams = int(L.m6a_prep_sites_stream_bytes(self._h)), int(L.m6a_prep_sites_n_streams(self._h))
        tx_off = arr(i.tx_off, C.c_int64, T + 1)
        self.tx_blob = C.string_at(i.tx_blob, int(tx_off[-1])) if T else b""
        self.tx_off = tx_off
        self.names = [self.tx_blob[tx_off[t]:tx_off[t + 1]].decode() for t in range(T)]
        names16, name_off, n_tab = C.c_void_p(), C.c_void_p(), C.c_int()
        L.m6a_prep_sites_read_names(self._h, C.byref(names16), C.byref(name_off), C.byref(n_tab))
        self.read_names, self.n_read_names, self.ms_intern = None, 0, float(L.m6a_prep_sites_intern_ms(self._h))
        if n_tab.value:
            offsets = arr(name_off, C.c_int64, n_tab.value + 1)
            self.n_read_names = int(offsets[-1])
            self.read_names = (arr(names16, C.c_uint8, 16 * self.n_read_names).reshape(self.n_read_names, 16), offsets)

    def times(self):
        """Phase milliseconds (include/m6a.h) and the device-to-host bytes so far."""
        keys = ("upload", "newlines", "parse_combine_windows", "back_half", "host", "read_ids_and_fetch_d2h", "upload_GBps", "total")
        return dict(zip(keys, list(self.info.ms))), int(self.info.d2h_bytes)

    def fetch(self):
        """(read_prob, site_prob, mod_ratio) from the device outputs m6a_infer wrote."""
        rp = np.empty(self.n_reads, np.float32)
        sp = np.empty(self.n_sites, np.float32)
        mr = np.empty(self.n_sites, np.float64)
        rc = self._L.m6a_prep_sites_fetch(self._h, rp.ctypes.data, sp.ctypes.data, mr.ctypes.data)
        if rc != 0:
            raise M6AIOError("m6a_prep error %d: %s" % (rc, self._L.m6a_prep_last_error().decode()), self._CODES.get(rc, rc))
        return rp, sp, mr

    def inputs(self):
        """Host copies of the device arrays (X [R, 9], site_kmers [S, 3], off [S + 1]), for inspection."""
        X = np.empty((self.n_reads, 9), np.float32)
        km = np.empty((self.n_sites, 3), np.uint8)
        off = np.empty(self.n_sites + 1, np.int64)
        rc = self._L.m6a_prep_sites_inputs(self._h, X.ctypes.data, km.ctypes.data, off.ctypes.data)
        if rc != 0:
            raise M6AIOError("m6a_prep error %d: %s" % (rc, self._L.m6a_prep_last_error().decode()), self._CODES.get(rc, rc))
        return X, km, off

    def writer(self):
        """The sites as an m6a_sites for the CSV writers (NativeSites.from_arrays)."""
        k5 = np.ascontiguousarray(self.kmer7[:, 1:6])
        rep = (self.read_rep, self.n_replicates) if self.n_replicates > 1 else (None, 1)
        w = NativeSites.from_arrays(self.off, self.tx_pos, self.tx_blob, self.tx_off, self.site_tx, k5, self.read_ids, *rep)
        if self.read_names is not None:
            w.set_read_names(*self.read_names)
        return w

    def write_csv(self, out_dir, write_header=True, n_threads=0, n_sites=None, compress=False, level=1):
        """m6a_prep_sites_write_csv: both CSV files formatted on the device from the handle's arrays (after the engine has filled
        read_prob / site_prob / mod_ratio) and pwritten from pinned rounds.  Returns the statistics as a dict.  Raises CsvDeclined
        (nothing opened, nothing written) when a value is outside what the kernels format: write through writer() then.
        compress=True: m6a_prep_sites_write_csv_bgzf -- the text is deflated on the device and the files are data.site_proba.csv.gz
        and data.indiv_proba.csv.gz (BGZF); the plain files are not created, and the dict is the m6a_csv_bgzf_stats.
        level (with compress): 1 is that symbol; anything else goes to m6a_prep_sites_write_csv_bgzf_level, where 2 is dynamic Huffman
        codes, and the dict holds n_by_type, the blocks of deflate block type 0, 1 and 2, as well."""
        from . import _lib
        if level != 1 and not compress:
            raise ValueError("level=%r needs compress=True" % (level,))
        st = _lib.CsvBgzfStats() if compress else _lib.CsvStats()
        head = (self._h, os.fsencode(out_dir), 1 if write_header else 0, -1 if n_sites is None else int(n_sites), int(n_threads))
        by = (C.c_int64 * 3)()
        if compress and level != 1:
            rc = self._L.m6a_prep_sites_write_csv_bgzf_level(*head, int(level), C.byref(st), by)
        else:
            rc = (self._L.m6a_prep_sites_write_csv_bgzf if compress else self._L.m6a_prep_sites_write_csv)(*head, C.byref(st))
        self.peak_bytes = int(self.info.peak_bytes)
        stats = {k: getattr(st, k) for k, _ in st._fields_}
        if compress and level != 1:
            stats["n_by_type"] = list(by)
        if rc == _lib.M6A_EDECLINED:
            raise CsvDeclined("m6a_prep error %d: %s" % (rc, self._L.m6a_prep_last_error().decode()), rc, stats["n_declined"])
        if rc != 0:
            raise M6AIOError("m6a_prep error %d: %s" % (rc, self._L.m6a_prep_last_error().decode()), self._CODES.get(rc, rc))
        return stats

    def write_read_representation(self, engine, path, dtype="float32", n_sites=None):
        """m6a_prep_sites_write_read_representation: the .npy file `path`, [off[n_sites]][32] float32 or float16 ("float32" |
        "float16", or M6A_REPR_F32 | M6A_REPR_F16), the rows of the first n_sites sites (None: all), computed by `engine` (an
        M6ANetEngine on the handle's device) from the handle's device arrays in rounds of M6A_REPR_ROUND_KB and pwritten from
        pinned buffers.  Returns the m6a_repr_write_stats as a dict.  A call that raises leaves no file."""
        from . import _lib
        st = _lib.ReprWriteStats()
        code = _lib.REPR_DTYPES.get(dtype, dtype) if isinstance(dtype, str) else dtype
        if isinstance(code, str):
            raise ValueError("dtype must be 'float32' or 'float16', not %r" % (dtype,))
        rc = self._L.m6a_prep_sites_write_read_representation(self._h, getattr(engine, "_h", engine), None if path is None else os.fsencode(path),
                                                              int(code), -1 if n_sites is None else int(n_sites), C.byref(st))
        if self.info is not None:
            self.peak_bytes = int(self.info.peak_bytes)
        if rc != 0:
            raise M6AIOError("m6a_prep error %d: %s" % (rc, self._L.m6a_prep_last_error().decode()), self._CODES.get(rc, rc))
        return {k: getattr(st, k) for k, _ in st._fields_}

    def close(self):
        if getattr(self, "_h", None):
            self._L.m6a_prep_sites_free(self._h)
            self._h = None
            self.info = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class prep_sites_grouped:
    """m6a_prep_group (libm6a_hip.so, include/m6a.h: grouped input): one eventalign file -- a path, `-`, a FIFO -- whose transcripts
    each form one stretch, delivered as an iterator of prep_sites handles, batch after batch as transcripts complete; their arrays, one
    after the other, are prep_sites(eventalign, ...)'s (every batch numbers its transcripts itself: compare through `names`).  The
    text is always parsed in windows (window_kb, else M6A_PREP_WINDOW_KB, else 256 MB); a batch is taken when the closed runs and rows
    reach group_kb (None: M6A_PREP_GROUP_KB, default 262144); every batch but the last ends on a flush boundary of (batch_size,
    save_per_batch), and first_site -- the sites of the batches before the one at hand -- is what engine.set_job_offset takes.
    Only one batch is alive at a time: the iterator closes the batch at hand before it asks for the next.  Input that is not grouped
    raises M6AIOError (M6A_EFORMAT) with the statement's text when the offending run is met.  counts() is m6a_prep_group_counts."""
    _CODES = prep_on_device._CODES

    def __init__(self, eventalign, readcount_min=1, readcount_max=1000, min_segment_count=20, norm=None, n_threads=0, device_id=0,
                 window_kb=None, group_kb=None, batch_size=16, save_per_batch=2):
        from . import _lib
        L, io = _lib.load(), load()
        self._L, self._g, self._batch, self.first_site = L, C.c_void_p(), None, 0
        blob, mean, std, n = norm_arrays(norm)
        host = _lib.HostHalf(C.cast(io.m6a_io_runs_rows, C.c_void_p), C.cast(io.m6a_io_rows_table, C.c_void_p),
                             C.cast(io.m6a_io_rows_free, C.c_void_p), C.cast(io.m6a_io_last_error, C.c_void_p))
        rc = L.m6a_prep_group_open(int(device_id), os.fsencode(eventalign), int(readcount_min), int(readcount_max), int(min_segment_count), blob,
                                   None if mean is None else mean.ctypes.data, None if std is None else std.ctypes.data, n, C.byref(host),
                                   int(n_threads), -1 if not window_kb else int(window_kb) << 10, -1 if not group_kb else int(group_kb) << 10,
                                   int(batch_size), int(save_per_batch), C.byref(self._g))
        if rc != 0:
            self._g = None
            self._fail(rc)

    def _fail(self, rc):
        raise M6AIOError("m6a_prep error %d: %s" % (rc, self._L.m6a_prep_last_error().decode()), self._CODES.get(rc, rc))

    def __iter__(self):
        return self

    def __next__(self):
        if self._batch is not None:
            self._batch.close()
            self._batch = None
        if not self._g:
            raise StopIteration
        h = C.c_void_p()
        rc = self._L.m6a_prep_group_next(self._g, C.byref(h))
        if rc != 0:
            self._fail(rc)
        if not h:
            raise StopIteration
        p = prep_sites.__new__(prep_sites)
        p._L, p._h = self._L, h
        p._adopt()
        self._batch, self.first_site = p, self.counts()["first_site"]
        return p

    def counts(self):
        from . import _lib
        c = _lib.PrepGroupCounts()
        rc = self._L.m6a_prep_group_info(self._g, C.byref(c))
        if rc != 0:
            self._fail(rc)
        return {k: int(getattr(c, k)) for k, _ in c._fields_}

    def close(self):
        if getattr(self, "_batch", None) is not None:
            self._batch.close()
            self._batch = None
        if getattr(self, "_g", None):
            self._L.m6a_prep_group_close(self._g)
            self._g = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def json_sites(input_dir, min_reads=20, norm=None, n_threads=0, device=0):
    """m6a_json_sites_build (libm6a_hip.so): one directory of data.info + data.json -> the arrays NativeSites([input_dir], ...) holds,
    parsed by HIP kernels, with X, site_kmers and off left on the device -- a prep_sites, as prep_sites() returns for eventalign.txt
    (info, off, site_tx, tx_pos, kmer7, read_ids, names, times(), fetch(), inputs(), writer(), write_csv(), close()).  Sites the
    kernels decline are parsed by the host loader's own code (n_declined_sites counts them); its errors are raised as M6AIOError with
    its code and text.  `input_dir` may be a list: more than one directory, or a site store, is refused (ValueError)."""
    from . import _lib
    dirs = [input_dir] if isinstance(input_dir, (str, bytes, os.PathLike)) else list(input_dir)
    L, io = _lib.load(), load()
    self = prep_sites.__new__(prep_sites)
    self._L, self._h = L, C.c_void_p()
    blob, mean, std, n = norm_arrays(norm)
    host = _lib.JsonHostHalf(*(C.cast(f, C.c_void_p) for f in (io.m6a_io_info_open, io.m6a_io_info_get, io.m6a_io_info_rows, io.m6a_io_info_free,
                                                                io.m6a_io_last_error)))
    paths = [os.fsencode(d) for d in dirs]
    rc = L.m6a_json_sites_build(int(device), (C.c_char_p * len(paths))(*paths), len(paths), int(min_reads), blob,
                                None if mean is None else mean.ctypes.data, None if std is None else std.ctypes.data, n, C.byref(host),
                                int(n_threads), C.byref(self._h))
    if rc != 0:
        self._h = None
        text = L.m6a_prep_last_error().decode()
        if rc == -1 and (len(dirs) != 1 or str(os.fsdecode(dirs[0])).endswith(".m6astore")):
            raise ValueError(text)
        code = prep_sites._CODES.get(rc, rc)
        # M6A_EFORMAT / M6A_EIO carry the host loader's own text: raised as NativeSites raises it
        raise M6AIOError(("m6a_io error %d: %s" if rc in (-7, -8) else "m6a_prep error %d: %s") % (code if rc in (-7, -8) else rc, text), code)
    self._adopt()
    return self


def _norm_table(tx, pos, start, end, n_reads):
    names = [os.fsencode(t) if not isinstance(t, bytes) else t for t in tx]
    tx_off = np.zeros(len(names) + 1, np.int64)
    np.cumsum([len(t) for t in names], out=tx_off[1:])
    cols = [np.ascontiguousarray(a, np.int64) for a in (pos, start, end, n_reads)]
    if any(a.shape != (len(names),) for a in cols):
        raise ValueError("the site table's columns differ in length")
    return b"".join(names) + b"\0", tx_off, cols


def norm_partials(json_path, tx, pos, start, end, n_reads, sites=None, n_threads=0):
    """m6a_io_norm_partials (libm6a_io.so): (s [n][9], s2 [n][9], 7-mers) of the table's rows `sites` (ascending; None: all)."""
    L = load()
    blob, tx_off, (pos, start, end, n_reads) = _norm_table(tx, pos, start, end, n_reads)
    sel = None if sites is None else np.ascontiguousarray(sites, np.int64)
    n = len(pos) if sel is None else len(sel)
    s, s2, k7 = np.zeros((n, 9)), np.zeros((n, 9)), np.zeros((n, 7), np.uint8)
    _chk(L.m6a_io_norm_partials(os.fsencode(json_path), len(pos), blob, tx_off.ctypes.data, pos.ctypes.data, start.ctypes.data, end.ctypes.data,
                                n_reads.ctypes.data, None if sel is None else sel.ctypes.data, n, int(n_threads), s.ctypes.data, s2.ctypes.data,
                                k7.ctypes.data))
    return s, s2, [bytes(k).decode("latin-1") for k in k7]


def norm_factors(json_path, tx, pos, start, end, n_reads, device="cpu", n_threads=0):
    """The per-5-mer sums and factors of `compute_norm_factors` (include/m6a.h states the operation at m6a_norm_factors_build) over
    the table's rows in their order: device "cpu" is m6a_io_norm_factors (libm6a_io.so), an integer the HIP device of
    m6a_norm_factors_build (libm6a_hip.so); both return the same bits.  -> dict: kmers (list of str, bytewise order), N [K], S, S2,
    mean, std [K][3], kmer7 (list of str); the device route adds status [n_sites] (0, or the reason the kernels declined the site
    for) and stats (phase times in ms, n_sites, n_reads, n_kmers, n_declined, d2h_bytes, peak_bytes).  The loader's errors are raised
    as M6AIOError with its code and text on both routes."""
    io = load()
    blob, tx_off, (pos, start, end, n_reads) = _norm_table(tx, pos, start, end, n_reads)
    n, cap = len(pos), max(1, 3 * len(pos))
    kmers, N, k7 = np.zeros((cap, 5), np.uint8), np.zeros(cap, np.int64), np.zeros((max(1, n), 7), np.uint8)
    S, S2, mean, std = (np.zeros((cap, 3)) for _ in range(4))
    K = C.c_int64(0)
    out = {}
    if device == "cpu":
        _chk(io.m6a_io_norm_factors(os.fsencode(json_path), n, blob, tx_off.ctypes.data, pos.ctypes.data, start.ctypes.data, end.ctypes.data,
                                    n_reads.ctypes.data, int(n_threads), kmers.ctypes.data, N.ctypes.data, S.ctypes.data, S2.ctypes.data,
                                    mean.ctypes.data, std.ctypes.data, C.byref(K), k7.ctypes.data))
    else:
        from . import _lib
        L = _lib.load()
        host = _lib.NormHostHalf(C.cast(io.m6a_io_norm_partials, C.c_void_p), C.cast(io.m6a_io_last_error, C.c_void_p))
        status, st = np.zeros(max(1, n), np.uint8), _lib.NormStats()
        rc = L.m6a_norm_factors_build(int(device), os.fsencode(json_path), n, blob, tx_off.ctypes.data, pos.ctypes.data, start.ctypes.data,
                                      end.ctypes.data, n_reads.ctypes.data, C.byref(host), int(n_threads), kmers.ctypes.data, N.ctypes.data,
                                      S.ctypes.data, S2.ctypes.data, mean.ctypes.data, std.ctypes.data, C.byref(K), status.ctypes.data,
                                      k7.ctypes.data, C.byref(st))
        if rc != 0:
            code = prep_sites._CODES.get(rc, rc)
            text = L.m6a_prep_last_error().decode()
            # M6A_EFORMAT / M6A_EIO carry the host loader's own text: raised as the host route raises it
            raise M6AIOError(("m6a_io error %d: %s" if rc in (-7, -8) else "m6a_prep error %d: %s") % (code if rc in (-7, -8) else rc, text), code)
        out["status"] = status[:n]
        out["stats"] = {f: getattr(st, f) for f, _ in st._fields_}
    k = K.value
    out.update(kmers=[bytes(x).decode("latin-1") for x in kmers[:k]], N=N[:k], S=S[:k], S2=S2[:k], mean=mean[:k], std=std[:k],
               kmer7=[bytes(x).decode("latin-1") for x in k7[:n]])
    return out


class CsvDeclined(M6AIOError):
    """The device CSV writer met `n_declined` values it does not format (M6A_EDECLINED, include/m6a.h); nothing was written."""

    def __init__(self, msg, code, n_declined):
        super().__init__(msg, code)
        self.n_declined = int(n_declined)


def csv_format(off, tx_pos, tx_blob, tx_off, site_tx, kmer5, read_ids, read_prob, site_prob, mod_ratio, read_rep=None, n_rep=1,
               site_begin=0, site_end=None, device_id=0):
    """m6a_csv_format (libm6a_hip.so): the rows of sites [site_begin, site_end) of data.site_proba.csv and data.indiv_proba.csv,
    formatted on the device from host arrays (NativeSites.from_arrays' set plus the three outputs).  Returns
    (site_bytes, indiv_bytes, n_declined); with n_declined > 0 both texts are None (the device wrote none)."""
    from . import _lib
    L = _lib.load()
    S = len(tx_pos)
    k5 = np.ascontiguousarray(np.frombuffer(b"".join(kmer5), np.uint8) if isinstance(kmer5, (list, tuple)) else kmer5, np.uint8)
    keep = [np.ascontiguousarray(off, np.int64), np.ascontiguousarray(site_tx, np.uint32), np.ascontiguousarray(tx_pos, np.int64), k5,
            np.ascontiguousarray(tx_off, np.int64), np.ascontiguousarray(read_ids, np.float64),
            None if read_rep is None else np.ascontiguousarray(read_rep, np.int32), np.ascontiguousarray(read_prob, np.float32),
            np.ascontiguousarray(site_prob, np.float32), np.ascontiguousarray(mod_ratio, np.float64)]
    o, tx, pos, k5, txo, ids, rep, rp, sp, mr = keep
    assert o.size == S + 1 and tx.size == S and k5.size == 5 * S and sp.size == S and mr.size == S
    assert ids.size == rp.size == int(o[-1]) and (rep is None or rep.size == ids.size)
    blob = bytes(tx_blob)
    a = _lib.CsvArrays(S, len(txo) - 1, o.ctypes.data, tx.ctypes.data, pos.ctypes.data, k5.ctypes.data, blob, txo.ctypes.data, ids.ctypes.data,
                       None if rep is None else rep.ctypes.data, int(n_rep), rp.ctypes.data, sp.ctypes.data, mr.ctypes.data)
    b, e = int(site_begin), S if site_end is None else int(site_end)
    ns, ni, nd = C.c_int64(), C.c_int64(), C.c_int64()

    def call(site_buf, indiv_buf):
        rc = L.m6a_csv_format(int(device_id), C.byref(a), b, e, site_buf, ns.value if site_buf else 0, indiv_buf, ni.value if indiv_buf else 0,
                              C.byref(ns), C.byref(ni), C.byref(nd))
        if rc not in (0, _lib.M6A_EDECLINED):
            raise M6AIOError("m6a_prep error %d: %s" % (rc, L.m6a_prep_last_error().decode()), prep_on_device._CODES.get(rc, rc))
        return rc
    if call(None, None) == _lib.M6A_EDECLINED:
        return None, None, nd.value
    site_buf, indiv_buf = C.create_string_buffer(max(1, ns.value)), C.create_string_buffer(max(1, ni.value))
    call(site_buf, indiv_buf)
    return site_buf.raw[:ns.value], indiv_buf.raw[:ni.value], nd.value


def _weakrefable(x):
    try:
        import weakref
        weakref.ref(x)
        return True
    except TypeError:
        return False


class NativeSites:
    """Owns an m6a_sites handle; exposes its arrays as zero-copy numpy views."""

    def __init__(self, input_dirs=None, min_reads=20, norm=None, n_threads=0, store=None, _arrays=None):
        """Either parses `input_dirs` (data.info + data.json per directory) or maps a binary site `store` file."""
        L = load()
        h = C.c_void_p()
        if _arrays is not None:
            off, tx_pos, blob, tx_off, site_tx, k5, ids, rep, n_rep = _arrays
            head = (len(tx_pos), off.ctypes.data, tx_pos.ctypes.data, blob, tx_off.ctypes.data, len(tx_off) - 1, site_tx.ctypes.data,
                    k5.tobytes(), ids.ctypes.data)
            if rep is None:
                _chk(L.m6a_io_sites_from_arrays(*head, C.byref(h)))
            else:
                _chk(L.m6a_io_sites_from_arrays_rep(*head, rep.ctypes.data, int(n_rep), C.byref(h)))
        elif store is not None:
            _chk(L.m6a_io_open_store(os.fsencode(store), C.byref(h)))
        else:
            dirs = (C.c_char_p * len(input_dirs))(*[os.fsencode(d) for d in input_dirs])
            if norm:
                kmers = sorted(norm)
                blob = "".join(kmers).encode()
                mean = np.ascontiguousarray([norm[k][0] for k in kmers], np.float64)
                std = np.ascontiguousarray([norm[k][1] for k in kmers], np.float64)
                args = (blob, mean.ctypes.data, std.ctypes.data, len(kmers))
            else:
                args = (None, None, None, 0)
            _chk(L.m6a_io_load_sites(dirs, len(input_dirs), int(min_reads), *args, int(n_threads), C.byref(h)))
        self._h, self._L = h, L
        self.tag = L.m6a_io_store_tag(h).decode()
        S, R = L.m6a_io_n_sites(h), L.m6a_io_n_reads(h)
        self.n_replicates = L.m6a_io_n_replicates(h)

        def view(fn, ctype, shape):
            n = int(np.prod(shape))
            if n == 0:                                   # an empty array may have no address (sites from arrays, S = 0)
                return np.zeros(shape, np.dtype(ctype))
            arr = np.ctypeslib.as_array(C.cast(fn(h), C.POINTER(ctype)), shape=(n,)).reshape(shape)
            arr.flags.writeable = False
            return arr
        self.X = view(L.m6a_io_X, C.c_float, (R, 9)) if _arrays is None else None         # from_arrays: sites for the writers only
        self.site_kmers = view(L.m6a_io_site_kmers, C.c_uint8, (S, 3)) if _arrays is None else None
        self.off = view(L.m6a_io_off, C.c_int64, (S + 1,))
        self.tx_pos = view(L.m6a_io_tx_pos, C.c_int64, (S,))
        self.read_id_values = view(L.m6a_io_read_ids, C.c_double, (R,))
        self.read_rep = view(L.m6a_io_read_rep, C.c_int32, (R,)) if _arrays is None or _arrays[7] is not None else None

    @classmethod
    def from_arrays(cls, off, tx_pos, tx_blob, tx_off, site_tx, kmer5, read_ids, read_rep=None, n_rep=1):
        """m6a_io_sites_from_arrays: sites without X for the writers.  tx_blob / tx_off: the transcript names; site_tx [S] indexes them;
        kmer5 [S][5] uint8 (or bytes-like rows); read_ids [R] float64.  read_rep [R] int32 with n_rep: pooled replicates
        (m6a_io_sites_from_arrays_rep), read ids printed `<id>_<replicate>` when n_rep > 1."""
        k5 = np.ascontiguousarray(np.frombuffer(b"".join(kmer5), np.uint8) if isinstance(kmer5, (list, tuple)) else kmer5, np.uint8)
        arrays = (np.ascontiguousarray(off, np.int64), np.ascontiguousarray(tx_pos, np.int64), bytes(tx_blob), np.ascontiguousarray(tx_off, np.int64),
                  np.ascontiguousarray(site_tx, np.uint32), k5, np.ascontiguousarray(read_ids, np.float64),
                  None if read_rep is None else np.ascontiguousarray(read_rep, np.int32), n_rep)
        return cls(_arrays=arrays)

    def set_read_names(self, names16, name_off):
        """m6a_io_sites_set_read_names, on sites made by from_arrays: names16 uint8 [n][16] and name_off int64 [n_replicates + 1]
        (prep_sites.read_names).  The writers then print the UUID of row read_ids[r] of read r's replicate's table, `_<replicate>`
        behind it with several replicates; a read id that is no index into its table is M6AIOError (EINVAL)."""
        names = np.ascontiguousarray(names16, np.uint8)
        off = np.ascontiguousarray(name_off, np.int64)
        if off.size != self.n_replicates + 1 or names.size != 16 * int(off[-1]):
            raise ValueError("name_off must hold n_replicates + 1 offsets and names16 16 bytes per name")
        _chk(self._L.m6a_io_sites_set_read_names(self._h, names.ctypes.data, off.ctypes.data, int(self.n_replicates)))

    def tx_id(self, i):
        return self._L.m6a_io_tx_id(self._h, i).decode()

    def kmer5(self, i):
        return self._L.m6a_io_kmer5(self._h, i).decode()

    def save_store(self, path, tag=""):
        """Writes everything this handle holds as one binary site store (include/m6a_io.h)."""
        _chk(self._L.m6a_io_save_store(self._h, os.fsencode(path), tag.encode()[:63]))

    def write_csv(self, out_dir, read_prob, site_prob, mod_ratio, write_header=False, n_threads=0, n_sites=None):
        self._drop_shard_kept()
        rp = np.ascontiguousarray(read_prob, np.float32)
        sp = np.ascontiguousarray(site_prob, np.float32)
        mr = np.ascontiguousarray(mod_ratio, np.float64)
        assert rp.size == int(self.off[-1]) and sp.size == self.tx_pos.size == mr.size
        _chk(self._L.m6a_io_write_csv_n(self._h, os.fsencode(out_dir), rp.ctypes.data, sp.ctypes.data, mr.ctypes.data,
                                        1 if write_header else 0, int(n_threads), -1 if n_sites is None else int(n_sites)))

    def _shard_args(self, a, b, read_prob, site_prob, mod_ratio):
        rp = np.ascontiguousarray(read_prob, np.float32)
        sp = np.ascontiguousarray(site_prob, np.float32)
        mr = np.ascontiguousarray(mod_ratio, np.float64)
        assert sp.size == mr.size == b - a and rp.size == int(self.off[b] - self.off[a])
        return rp, sp, mr

    def _drop_shard_kept(self):
        self._shard_kept = None

    def csv_shard_size(self, a, b, read_prob, site_prob, mod_ratio, n_threads=0):
        """Bytes the rows of sites [a, b) take in (data.site_proba.csv, data.indiv_proba.csv); the arrays hold that range only."""
        import weakref
        self._drop_shard_kept()                      # an earlier size call that was never followed by its write
        rp, sp, mr = self._shard_args(a, b, read_prob, site_prob, mod_ratio)
        ns, ni = C.c_int64(), C.c_int64()
        _chk(self._L.m6a_io_csv_shard_size(self._h, rp.ctypes.data, sp.ctypes.data, mr.ctypes.data, int(a), int(b), int(n_threads),
                                           C.byref(ns), C.byref(ni)))        # raises: nothing is kept
        # The library keeps the text it formatted for the csv_shard_write that follows, keyed on the arrays' addresses (and a
        # checksum).  Kept here until then: CONVERTED temporaries (strongly -- nobody else holds them, and the write must pass the
        # same addresses), and only weak references to the caller's own objects (read_prob is 4 bytes per read and
        # can reach GBs; a size call that is never followed by its write must not pin it for the life of this handle).  If a
        # caller array is gone by then, or another csv_* call came between, the write formats again -- correct, just slower.
        def keep(conv, orig):
            return (weakref.ref(orig), None) if conv is orig else (weakref.ref(orig) if _weakrefable(orig) else None, conv)
        self._shard_kept = ((int(a), int(b)), tuple(keep(c_, o_) for c_, o_ in zip((rp, sp, mr), (read_prob, site_prob, mod_ratio))))
        return ns.value, ni.value

    def csv_shard_write(self, out_dir, a, b, read_prob, site_prob, mod_ratio, site_offset, indiv_offset, header_and_totals=None, n_threads=0):
        """pwrite()s the rows of sites [a, b) at the given byte offsets; `header_and_totals` = (site_total, indiv_total) on the
        one rank that also writes the header lines and sets the files' final sizes."""
        kept, self._shard_kept = getattr(self, "_shard_kept", None), None
        arrs = None
        if kept is not None and kept[0] == (int(a), int(b)):
            same = [r is not None and r() is o for (r, _), o in zip(kept[1], (read_prob, site_prob, mod_ratio))]
            if all(same):                            # the very arrays csv_shard_size formatted: the kept text is reused
                arrs = tuple(conv if conv is not None else o for (_, conv), o in zip(kept[1], (read_prob, site_prob, mod_ratio)))
        del kept
        rp, sp, mr = arrs if arrs is not None else self._shard_args(a, b, read_prob, site_prob, mod_ratio)
        st, it = header_and_totals if header_and_totals is not None else (-1, -1)
        _chk(self._L.m6a_io_csv_shard_write(self._h, os.fsencode(out_dir), rp.ctypes.data, sp.ctypes.data, mr.ctypes.data, int(a), int(b),
                                            int(n_threads), int(site_offset), int(indiv_offset), 1 if header_and_totals is not None else 0,
                                            int(st), int(it)))

    def csv_header_bytes(self):
        return int(self._L.m6a_io_csv_header_bytes(0)), int(self._L.m6a_io_csv_header_bytes(1))

    def close(self):
        self._shard_kept = None
        if getattr(self, "_h", None):
            for name in ("X", "site_kmers", "off", "tx_pos", "read_id_values", "read_rep"):
                setattr(self, name, None)
            self._L.m6a_io_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
