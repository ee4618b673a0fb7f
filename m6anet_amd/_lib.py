"""ctypes binding of libm6a_hip.so (include/m6a.h).  No CPU fallback: if the HIP library is
missing or a call fails, this raises."""
import ctypes as C
import os

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("M6A_HIP_LIB") or os.path.join(_PKG, "libm6a_hip.so")   # M6A_HIP_LIB: an experimental build

M6A_OK = 0
ERRORS = {-1: "M6A_EINVAL", -2: "M6A_ENOMEM", -3: "M6A_EHIP", -4: "M6A_ESTREAM", -5: "M6A_ENODEV",
          -6: "M6A_EUNSUPPORTED", -7: "M6A_EFORMAT", -8: "M6A_EIO", -9: "M6A_EDECLINED"}
M6A_EDECLINED = -9
RNG_NUMPY = 0
REPR_DTYPES = {"float32": 0, "float16": 1}           # M6A_REPR_F32, M6A_REPR_F16

# every symbol include/m6a.h declares (tests check the .so exports exactly these)
SYMBOLS = ["m6a_create", "m6a_destroy", "m6a_last_error", "m6a_set_stream", "m6a_set_job_offset", "m6a_set_scan_driver", "m6a_set_table_variant", "m6a_set_encoder_variant", "m6a_last_encoder_variant", "m6a_last_encoder_kernel", "m6a_sync", "m6a_set_host_offsets", "m6a_prepare_host_io", "m6a_host_alloc", "m6a_host_free", "m6a_host_is_pinned",
           "m6a_encode_reads", "m6a_read_representation", "m6a_read_representation_dtype", "m6a_site_pool", "m6a_site_expectation", "m6a_site_ranksum", "m6a_site_signal_ranksum", "m6a_site_ks", "m6a_site_signal_ks", "m6a_ks_exact", "m6a_set_site_mode", "m6a_infer", "m6a_job_begin", "m6a_job_feed", "m6a_job_feed_collated", "m6a_job_size", "m6a_job_end", "m6a_job_abort", "m6a_bag_forward", "m6a_validate_pool", "m6a_validate", "m6a_flush_groups",
           "m6a_reference_written_sites",
           "m6a_shard_plan", "m6a_comm_unique_id", "m6a_comm_init", "m6a_gather", "m6a_gather_reads", "m6a_device_count", "m6a_random_stream", "m6a_comm_destroy", "m6a_comm_count", "m6a_comm_info", "m6a_device_link", "m6a_profile_enable", "m6a_profile_read", "m6a_profile_clock", "m6a_last_pool_variant",
           "m6a_version", "m6a_prep_eventalign", "m6a_prep_table", "m6a_prep_times", "m6a_prep_free", "m6a_prep_last_error",
           "m6a_prep_sites_build", "m6a_prep_sites_build_multi", "m6a_prep_sites_build_windows", "m6a_prep_sites_build_names", "m6a_prep_sites_read_names", "m6a_prep_sites_intern_ms", "m6a_prep_sites_stream_bytes", "m6a_prep_sites_n_streams", "m6a_prep_sites_get", "m6a_prep_sites_fetch", "m6a_prep_sites_inputs", "m6a_prep_sites_free",
           "m6a_prep_group_open", "m6a_prep_group_next", "m6a_prep_group_info", "m6a_prep_group_close",
           "m6a_csv_format", "m6a_prep_sites_write_csv", "m6a_bgzf_inflate", "m6a_bgzf_deflate", "m6a_prep_sites_write_csv_bgzf",
           "m6a_bgzf_deflate_level", "m6a_prep_sites_write_csv_bgzf_level", "m6a_prep_sites_write_read_representation", "m6a_json_sites_build", "m6a_norm_factors_build", "m6a_repr_format", "m6a_prep_dataprep_write",
           "m6a_train_create", "m6a_train_destroy", "m6a_train_step", "m6a_train_epoch", "m6a_train_sample", "m6a_train_grads", "m6a_train_weights", "m6a_train_stats",
           "m6a_train_set_clip", "m6a_train_last_norm", "m6a_train_state_get", "m6a_train_state_set",
           "m6a_train_set_weights", "m6a_train_forward", "m6a_train_running_stats", "m6a_train_backward"]

_lib = None


class HostHalf(C.Structure):
    """m6a_prep_host_half (include/m6a.h): the libm6a_io.so functions that combine the runs the device declines."""
    _fields_ = [("rows", C.c_void_p), ("table", C.c_void_p), ("free", C.c_void_p), ("error", C.c_void_p)]


class JsonHostHalf(C.Structure):
    """m6a_json_host_half (include/m6a.h): the libm6a_io.so functions behind `inference --loader device`."""
    _fields_ = [("open", C.c_void_p), ("table", C.c_void_p), ("rows", C.c_void_p), ("free", C.c_void_p), ("error", C.c_void_p)]


class NormHostHalf(C.Structure):
    """m6a_norm_host_half (include/m6a.h): the libm6a_io.so functions behind `compute_norm_factors --device gpu`."""
    _fields_ = [("partials", C.c_void_p), ("error", C.c_void_p)]


class NormStats(C.Structure):
    """m6a_norm_stats (include/m6a.h)."""
    _fields_ = [("ms_upload", C.c_double), ("ms_kernels", C.c_double), ("ms_host", C.c_double), ("ms_fold", C.c_double),
                ("ms_total", C.c_double), ("n_sites", C.c_int64), ("n_reads", C.c_int64), ("n_kmers", C.c_int64),
                ("n_declined", C.c_int64), ("d2h_bytes", C.c_int64), ("peak_bytes", C.c_int64)]


class PrepSitesInfo(C.Structure):
    """m6a_prep_sites_info (include/m6a.h)."""
    _fields_ = [("n_sites", C.c_int64), ("n_reads", C.c_int64), ("n_tx", C.c_int64), ("X", C.c_void_p), ("site_kmers", C.c_void_p),
                ("off", C.c_void_p), ("read_prob", C.c_void_p), ("site_prob", C.c_void_p), ("mod_ratio", C.c_void_p),
                ("off_host", C.c_void_p), ("site_tx", C.c_void_p), ("site_pos", C.c_void_p), ("site_kmer7", C.c_void_p),
                ("tx_blob", C.c_void_p), ("tx_off", C.c_void_p), ("read_ids", C.c_void_p), ("ms", C.c_double * 8),
                ("d2h_bytes", C.c_int64), ("n_rep", C.c_int), ("read_rep", C.c_void_p), ("peak_bytes", C.c_int64),
                ("n_windows", C.c_int64), ("window_bytes", C.c_int64),
                ("n_bgzf_blocks", C.c_int64), ("compressed_bytes", C.c_int64), ("ms_inflate", C.c_double),
                ("n_declined_sites", C.c_int64)]


class PrepGroupCounts(C.Structure):
    """m6a_prep_group_counts (include/m6a.h)."""
    _fields_ = [(k, C.c_int64) for k in ("n_batches", "n_sites", "n_reads", "first_site", "max_kept_runs", "max_kept_rows", "total_runs",
                                         "total_rows", "peak_bytes", "d2h_bytes", "n_windows", "window_bytes", "stream_bytes", "group_bytes")]


class BgzfStats(C.Structure):
    """m6a_bgzf_stats (include/m6a.h)."""
    _fields_ = [("n_blocks", C.c_int64), ("compressed_bytes", C.c_int64), ("ms_upload", C.c_double), ("ms_inflate", C.c_double),
                ("ms_crc", C.c_double), ("ms_copy", C.c_double), ("d2h_bytes", C.c_int64)]


class DeflateStats(C.Structure):
    """m6a_deflate_stats (include/m6a.h)."""
    _fields_ = [("n_blocks", C.c_int64), ("n_stored", C.c_int64), ("ms_deflate", C.c_double), ("ms_copy", C.c_double), ("d2h_bytes", C.c_int64)]


class CsvBgzfStats(C.Structure):
    """m6a_csv_bgzf_stats (include/m6a.h)."""
    _fields_ = [("ms_format", C.c_double), ("ms_deflate", C.c_double), ("ms_copy", C.c_double), ("ms_write", C.c_double),
                ("site_bytes", C.c_int64), ("indiv_bytes", C.c_int64), ("site_compressed", C.c_int64), ("indiv_compressed", C.c_int64),
                ("n_blocks", C.c_int64), ("n_stored", C.c_int64), ("n_declined", C.c_int64), ("d2h_bytes", C.c_int64), ("n_rounds", C.c_int64)]


class CsvArrays(C.Structure):
    """m6a_csv_arrays (include/m6a.h): host arrays for m6a_csv_format."""
    _fields_ = [("n_sites", C.c_int64), ("n_tx", C.c_int64), ("off", C.c_void_p), ("site_tx", C.c_void_p), ("site_pos", C.c_void_p),
                ("kmer5", C.c_void_p), ("tx_blob", C.c_char_p), ("tx_off", C.c_void_p), ("read_ids", C.c_void_p), ("read_rep", C.c_void_p),
                ("n_rep", C.c_int), ("read_prob", C.c_void_p), ("site_prob", C.c_void_p), ("mod_ratio", C.c_void_p)]


class CsvStats(C.Structure):
    """m6a_csv_stats (include/m6a.h)."""
    _fields_ = [("ms_format", C.c_double), ("ms_copy", C.c_double), ("ms_write", C.c_double), ("site_bytes", C.c_int64),
                ("indiv_bytes", C.c_int64), ("n_declined", C.c_int64), ("d2h_bytes", C.c_int64), ("n_rounds", C.c_int64)]


class ReprWriteStats(C.Structure):
    """m6a_repr_write_stats (include/m6a.h)."""
    _fields_ = [("ms_kernel", C.c_double), ("ms_copy", C.c_double), ("ms_write", C.c_double), ("n_rounds", C.c_int64), ("n_rows", C.c_int64),
                ("bytes", C.c_int64), ("round_bytes", C.c_int64), ("d2h_bytes", C.c_int64)]


class DataprepStats(C.Structure):
    """m6a_dataprep_stats (include/m6a.h)."""
    _fields_ = [("ms_front", C.c_double), ("ms_back", C.c_double), ("ms_format", C.c_double), ("ms_copy", C.c_double), ("ms_write", C.c_double),
                ("json_bytes", C.c_int64), ("index_bytes", C.c_int64), ("n_sites", C.c_int64), ("n_runs", C.c_int64), ("n_declined", C.c_int64),
                ("n_rounds", C.c_int64), ("d2h_bytes", C.c_int64), ("peak_bytes", C.c_int64)]


class TrainConfig(C.Structure):
    """m6a_train_config (include/m6a.h)."""
    _fields_ = [("lr", C.c_float), ("beta1", C.c_float), ("beta2", C.c_float), ("eps", C.c_float), ("weight_decay", C.c_float)]


class M6AError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("%s (%d): %s" % (ERRORS.get(code, "M6A_E?"), code, msg))
        self.code = code


def _preload_hip_runtime():
    """One HIP runtime per process: PyTorch-ROCm ships its own libamdhip64.so.7 and refuses to
    see the GPU if another copy (e.g. /opt/rocm's) was mapped first.  When torch is installed,
    map ITS runtime before libm6a_hip.so so both bind to the same one, whichever is imported
    first.  (torch itself is not imported here.)"""
    import importlib.util
    # (HSA_ENABLE_IPC_MODE_LEGACY=0, which multi-process RCCL work needs on these boxes, is NOT set here any more: the library
    # binding must not edit the environment of whatever application imports it.  The package's own multi-process
    # entry points set it for their processes -- `python -m m6anet_amd` (m6anet_amd/_early.py) and bench.py; a host application
    # that drives m6a_comm_* itself exports it, as INTEGRATION.md says.)
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec and spec.submodule_search_locations:
        libdir = os.path.join(list(spec.submodule_search_locations)[0], "lib")
        rt = os.path.join(libdir, "libamdhip64.so")
        if os.path.exists(rt):
            C.CDLL(rt, mode=C.RTLD_GLOBAL)
        # the same goes for RCCL (m6a_gather binds it at run time): PyTorch's copy is linked to PyTorch's HIP runtime
        rccl = os.path.join(libdir, "librccl.so")
        if os.path.exists(rccl):
            os.environ.setdefault("M6A_RCCL_LIB", rccl)


def load():
    """Loads the in-tree HIP library.  Raises if it has not been built (python -m m6anet_amd.build)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError("libm6a_hip.so is not built: run `python -m m6anet_amd.build` "
                          "(or __graft_entry__.build()); there is no CPU fallback")
    _preload_hip_runtime()
    L = C.CDLL(LIB_PATH)
    vp, i64, i32, u32, f32, sz = C.c_void_p, C.c_int64, C.c_int, C.c_uint32, C.c_float, C.c_size_t
    L.m6a_create.argtypes = [C.POINTER(vp), vp, sz, i32]
    L.m6a_destroy.argtypes = [vp]
    L.m6a_destroy.restype = None
    L.m6a_last_error.argtypes = [vp]
    L.m6a_last_error.restype = C.c_char_p
    L.m6a_set_stream.argtypes = [vp, vp]
    L.m6a_sync.argtypes = [vp]
    L.m6a_set_host_offsets.argtypes = [vp, vp]
    L.m6a_prepare_host_io.argtypes = [vp]
    L.m6a_set_job_offset.argtypes = [vp, i64]
    L.m6a_set_scan_driver.argtypes = [vp, i32]
    L.m6a_set_table_variant.argtypes = [vp, i32]
    L.m6a_set_encoder_variant.argtypes = [vp, i32]
    L.m6a_last_encoder_variant.argtypes = [vp]
    L.m6a_last_encoder_variant.restype = C.c_char_p
    L.m6a_host_alloc.argtypes = [C.c_size_t, C.POINTER(vp)]
    L.m6a_host_free.argtypes = [vp]
    L.m6a_host_is_pinned.argtypes = [vp, C.c_size_t]
    L.m6a_last_encoder_kernel.argtypes = [vp]
    L.m6a_last_encoder_kernel.restype = C.c_char_p
    L.m6a_encode_reads.argtypes = [vp, vp, vp, vp, i64, vp]
    L.m6a_read_representation.argtypes = [vp, vp, vp, vp, i64, vp, vp]
    L.m6a_read_representation_dtype.argtypes = [vp, vp, vp, vp, i64, vp, i32, vp]
    L.m6a_site_pool.argtypes = [vp, vp, vp, i64, i32, i32, f32, u32, i32, i64, i64, vp, vp]
    L.m6a_site_expectation.argtypes = [vp, vp, vp, i64, i32, f32, vp, vp, vp]
    L.m6a_site_ranksum.argtypes = [vp, vp, vp, i64, vp, vp, i64, vp, vp, i64, vp, vp, vp, vp]
    L.m6a_site_signal_ranksum.argtypes = [vp, vp, vp, i64, vp, vp, i64, vp, vp, i64, vp, vp, vp, vp]
    L.m6a_site_ks.argtypes = [vp, vp, vp, i64, vp, vp, i64, vp, vp, i64, vp, vp, vp, vp]
    L.m6a_site_signal_ks.argtypes = [vp, vp, vp, i64, vp, vp, i64, vp, vp, i64, vp, vp, vp, vp]
    L.m6a_ks_exact.argtypes = [vp, vp, vp, vp, i64, vp]
    L.m6a_set_site_mode.argtypes = [vp, i32]
    L.m6a_infer.argtypes = [vp, vp, vp, vp, i64, i32, i32, f32, u32, i32, i64, i64, vp, vp, vp]
    L.m6a_job_begin.argtypes = [vp, i32, i32, f32, u32, i32, i64, i64, i64, i64]
    L.m6a_job_feed.argtypes = [vp, vp, vp, vp, i64]
    L.m6a_job_feed_collated.argtypes = [vp, vp, vp, vp, i64]
    L.m6a_job_size.argtypes = [vp, C.POINTER(i64), C.POINTER(i64)]
    L.m6a_job_end.argtypes = [vp, vp, vp, vp]
    L.m6a_job_abort.argtypes = [vp]
    L.m6a_bag_forward.argtypes = [vp, vp, vp, i64, i32, vp]
    L.m6a_validate_pool.argtypes = [vp, vp, vp, i64, i32, i32, C.c_uint32, vp, vp]
    L.m6a_validate.argtypes = [vp, vp, vp, vp, i64, i32, i32, C.c_uint32, vp, vp, vp]
    L.m6a_flush_groups.argtypes = [i64, i64, i64, vp, i64]
    L.m6a_flush_groups.restype = i64
    L.m6a_reference_written_sites.argtypes = [i64, i64, i64]
    L.m6a_reference_written_sites.restype = i64
    L.m6a_shard_plan.argtypes = [vp, i64, i64, i64, i32, vp]
    L.m6a_comm_unique_id.argtypes = [vp]
    L.m6a_comm_init.argtypes = [vp, vp, i32, i32]
    L.m6a_gather.argtypes = [vp, vp, vp, vp, i32, vp, vp]
    L.m6a_gather_reads.argtypes = [vp, vp, vp, i32, vp]
    L.m6a_device_count.argtypes = []
    L.m6a_random_stream.argtypes = [vp, u32, i64, vp]
    L.m6a_comm_destroy.argtypes = [vp]
    pi = C.POINTER(i32)
    L.m6a_comm_count.argtypes = [vp, pi]
    L.m6a_comm_info.argtypes = [vp, pi, pi, pi]
    L.m6a_device_link.argtypes = [i32, i32, pi, pi, pi]
    L.m6a_profile_enable.argtypes = [vp, i32]
    L.m6a_profile_read.argtypes = [vp, i32, C.POINTER(C.c_double), C.POINTER(i64)]
    L.m6a_profile_clock.argtypes = [vp, i32] + [C.POINTER(C.c_double)] * 4 + [C.POINTER(i32)]
    L.m6a_last_pool_variant.argtypes = [vp]
    L.m6a_last_pool_variant.restype = C.c_char_p
    L.m6a_version.restype = C.c_char_p
    L.m6a_prep_eventalign.argtypes = [i32, C.c_char_p, i32, C.c_char_p, C.POINTER(vp)]
    L.m6a_prep_table.argtypes = [vp]
    L.m6a_prep_table.restype = vp
    L.m6a_prep_times.argtypes = [vp, C.POINTER(C.c_double)]
    L.m6a_prep_free.argtypes = [vp]
    L.m6a_prep_free.restype = None
    L.m6a_prep_sites_build.argtypes = [i32, C.c_char_p, i32, i32, i32, C.c_char_p, vp, vp, i32, C.POINTER(HostHalf), i32, C.POINTER(vp)]
    L.m6a_prep_sites_build_multi.argtypes = [i32, C.POINTER(C.c_char_p), i32, i32, i32, i32, C.c_char_p, vp, vp, i32, C.POINTER(HostHalf), i32,
                                             C.POINTER(vp)]
    L.m6a_prep_sites_build_windows.argtypes = [i32, C.POINTER(C.c_char_p), i32, i32, i32, i32, C.c_char_p, vp, vp, i32, C.POINTER(HostHalf), i32,
                                               i64, C.POINTER(vp)]
    L.m6a_prep_sites_build_names.argtypes = [i32, C.POINTER(C.c_char_p), i32, i32, i32, i32, C.c_char_p, vp, vp, i32, C.POINTER(HostHalf), i32,
                                             i64, i32, C.POINTER(vp)]
    L.m6a_prep_sites_read_names.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(i32)]
    L.m6a_prep_sites_intern_ms.argtypes = [vp]
    L.m6a_prep_sites_intern_ms.restype = C.c_double
    for f in (L.m6a_prep_sites_stream_bytes, L.m6a_prep_sites_n_streams):
        f.argtypes = [vp]
        f.restype = C.c_int64
    L.m6a_json_sites_build.argtypes = [i32, C.POINTER(C.c_char_p), i32, i32, C.c_char_p, vp, vp, i32, C.POINTER(JsonHostHalf), i32, C.POINTER(vp)]
    L.m6a_norm_factors_build.argtypes = [i32, C.c_char_p, i64, vp, vp, vp, vp, vp, vp, C.POINTER(NormHostHalf), i32, vp, vp, vp, vp, vp, vp,
                                         C.POINTER(i64), vp, vp, C.POINTER(NormStats)]
    L.m6a_prep_sites_get.argtypes = [vp]
    L.m6a_prep_sites_get.restype = C.POINTER(PrepSitesInfo)
    L.m6a_prep_sites_fetch.argtypes = [vp, vp, vp, vp]
    L.m6a_prep_sites_inputs.argtypes = [vp, vp, vp, vp]
    L.m6a_prep_sites_free.argtypes = [vp]
    L.m6a_prep_sites_free.restype = None
    L.m6a_prep_group_open.argtypes = [i32, C.c_char_p, i32, i32, i32, C.c_char_p, vp, vp, i32, C.POINTER(HostHalf), i32, i64, i64, i64, i64,
                                      C.POINTER(vp)]
    L.m6a_prep_group_next.argtypes = [vp, C.POINTER(vp)]
    L.m6a_prep_group_info.argtypes = [vp, C.POINTER(PrepGroupCounts)]
    L.m6a_prep_group_close.argtypes = [vp]
    L.m6a_prep_group_close.restype = None
    pl = C.POINTER(i64)
    L.m6a_csv_format.argtypes = [i32, C.POINTER(CsvArrays), i64, i64, vp, i64, vp, i64, pl, pl, pl]
    L.m6a_prep_sites_write_csv.argtypes = [vp, C.c_char_p, i32, i64, i32, C.POINTER(CsvStats)]
    L.m6a_bgzf_inflate.argtypes = [i32, C.c_char_p, vp, i64, pl, C.POINTER(BgzfStats)]
    L.m6a_bgzf_deflate.argtypes = [i32, C.c_char_p, i64, vp, i64, pl, C.POINTER(DeflateStats)]
    L.m6a_prep_sites_write_csv_bgzf.argtypes = [vp, C.c_char_p, i32, i64, i32, C.POINTER(CsvBgzfStats)]
    L.m6a_bgzf_deflate_level.argtypes = [i32, C.c_char_p, i64, i32, vp, i64, pl, C.POINTER(DeflateStats), pl]
    L.m6a_prep_sites_write_csv_bgzf_level.argtypes = [vp, C.c_char_p, i32, i64, i32, i32, C.POINTER(CsvBgzfStats), pl]
    L.m6a_prep_sites_write_read_representation.argtypes = [vp, vp, C.c_char_p, i32, i64, C.POINTER(ReprWriteStats)]
    L.m6a_repr_format.argtypes = [i32, vp, i64, i32, vp, i64, vp, pl]
    L.m6a_prep_dataprep_write.argtypes = [i32, C.c_char_p, C.c_char_p, i32, i32, i32, i32, C.POINTER(HostHalf), i32, C.POINTER(DataprepStats)]
    L.m6a_train_create.argtypes = [vp, vp, sz, C.POINTER(TrainConfig), C.POINTER(vp)]
    L.m6a_train_destroy.argtypes = [vp]
    L.m6a_train_destroy.restype = None
    L.m6a_train_step.argtypes = [vp, vp, vp, vp, i64, i32, vp, vp]
    L.m6a_train_epoch.argtypes = [vp, vp, vp, vp, vp, i64, vp, i64, i64, i32, C.c_uint64, vp, vp]
    L.m6a_train_sample.argtypes = [vp, vp, i64, i32, C.c_uint64, vp]
    L.m6a_train_grads.argtypes = [vp, vp]
    L.m6a_train_weights.argtypes = [vp, vp, pl]
    L.m6a_train_stats.argtypes = [vp, pl, pl, pl]
    L.m6a_train_set_clip.argtypes = [vp, C.c_float]
    L.m6a_train_last_norm.argtypes = [vp, vp]
    L.m6a_train_state_get.argtypes = [vp, vp, vp, pl]
    L.m6a_train_state_set.argtypes = [vp, vp, vp, i64]
    L.m6a_train_set_weights.argtypes = [vp, vp]
    L.m6a_train_forward.argtypes = [vp, vp, vp, i64, i32, i32, vp, pl]
    L.m6a_train_running_stats.argtypes = [vp, vp]
    L.m6a_train_backward.argtypes = [vp, i64, vp, vp]
    L.m6a_prep_last_error.argtypes = []
    L.m6a_prep_last_error.restype = C.c_char_p
    for name in SYMBOLS:
        fn = getattr(L, name)
        if fn.restype is C.c_int and name not in ("m6a_flush_groups", "m6a_reference_written_sites"):
            fn.restype = C.c_int
    _lib = L
    return L
