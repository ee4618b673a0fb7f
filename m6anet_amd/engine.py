"""Host-side mirror of the reference's operator interface for the inference hot path, on top of
the C ABI (include/m6a.h).  Names follow the reference:

  M6ANetEngine.get_read_probability(X, site_kmers, off)
      == model.get_read_representation({'X','kmer'}) + model.pooling_filter.probability_layer(.)
         (m6anet/utils/inference_utils.py:35-37)
  M6ANetEngine.get_read_representation(X, site_kmers, off)
      == model.get_read_representation({'X','kmer'}) itself: float32 [R, 32] (m6anet/model/model.py:85-97)
  M6ANetEngine.calculate_site_proba(read_probs, off, n_iters, n_samples, ...)
      == calculate_site_proba(read_probs, n_iters, n_samples, n_processes=1) + mod_ratio
         (m6anet/utils/inference_utils.py:53-54,90-104)
  M6ANetEngine.infer(...)     == one whole run_inference job minus text I/O (inference_utils.py:14-71)
  M6ANetEngine.forward(X, kmer)  == MILModel.forward on fixed bags (m6anet/model/model.py:155-164)

Arrays may be numpy arrays (host pointers: the library stages them and the call is synchronous)
or torch tensors on the context's GPU (device pointers: zero-copy, stream-ordered).  PyTorch is
only plumbing here (device memory + streams); nothing in this file computes.
"""
import ctypes as C

import numpy as np

from . import _lib
from .constants import (DEFAULT_PRETRAINED_MODEL, DEFAULT_READ_THRESHOLD, N_REPR, N_SAMPLES, N_WEIGHT_FLOATS,
                        PRETRAINED_CONFIGS, asset_path)


def load_weights(pretrained_model=DEFAULT_PRETRAINED_MODEL):
    """Flat float32 weight blob (layout in include/m6a.h) of a bundled pretrained model."""
    if pretrained_model not in PRETRAINED_CONFIGS:
        raise ValueError("Invalid pretrained model {}, must be one of {}".format(
            pretrained_model, list(PRETRAINED_CONFIGS)))
    w = np.fromfile(asset_path(PRETRAINED_CONFIGS[pretrained_model][0]), np.float32)
    assert w.size == N_WEIGHT_FLOATS
    return w


def weights_from_state_dict(sd):
    """Flat blob from a reference checkpoint's state_dict (m6anet/model/model_states/*.pt,
    keys as built by m6anet/model/model.py:40-69)."""
    order = ["read_level_encoder.1.embedding_layer.weight", "read_level_encoder.3.layers.0.weight",
             "read_level_encoder.3.layers.0.bias", "read_level_encoder.3.layers.1.weight",
             "read_level_encoder.3.layers.1.bias", "read_level_encoder.3.layers.1.running_mean",
             "read_level_encoder.3.layers.1.running_var", "read_level_encoder.4.layers.0.weight",
             "read_level_encoder.4.layers.0.bias", "pooling_filter.probability_layer.0.weight",
             "pooling_filter.probability_layer.0.bias"]
    w = np.concatenate([np.asarray(sd[k].detach().cpu().numpy() if hasattr(sd[k], "detach") else sd[k],
                                   np.float32).ravel() for k in order])
    if w.size != N_WEIGHT_FLOATS:
        raise ValueError("state_dict does not have the m6anet.toml topology (%d floats)" % w.size)
    return w


STATE_DICT_KEYS = [("read_level_encoder.1.embedding_layer.weight", (66, 2)), ("read_level_encoder.3.layers.0.weight", (150, 15)),
                   ("read_level_encoder.3.layers.0.bias", (150,)), ("read_level_encoder.3.layers.1.weight", (150,)),
                   ("read_level_encoder.3.layers.1.bias", (150,)), ("read_level_encoder.3.layers.1.running_mean", (150,)),
                   ("read_level_encoder.3.layers.1.running_var", (150,)), ("read_level_encoder.4.layers.0.weight", (32, 150)),
                   ("read_level_encoder.4.layers.0.bias", (32,)), ("pooling_filter.probability_layer.0.weight", (1, 32)),
                   ("pooling_filter.probability_layer.0.bias", (1,))]


def state_dict_from_weights(w, num_batches_tracked=0):
    """The inverse of weights_from_state_dict: the reference's keys -> NumPy arrays in the shapes of m6anet/model/model.py:40-69,
    plus the batch norm's num_batches_tracked (int64 scalar).  No torch."""
    w = np.ascontiguousarray(w, np.float32)
    if w.size != N_WEIGHT_FLOATS:
        raise ValueError("weights must have %d floats" % N_WEIGHT_FLOATS)
    sd, o = {}, 0
    for key, shape in STATE_DICT_KEYS:
        n = int(np.prod(shape))
        sd[key] = w[o:o + n].reshape(shape).copy()
        o += n
        if key.endswith("running_var"):
            sd[key[:-len("running_var")] + "num_batches_tracked"] = np.array(int(num_batches_tracked), np.int64)
    return sd


def init_weights(seed):
    """A fresh blob by torch's default initialisation RULE, in NumPy: U(-1/sqrt(fan_in), 1/sqrt(fan_in)) for the weights and biases
    of the three linear layers, N(0, 1) for the embedding, gamma = 1, beta = 0, running statistics 0 and 1.  The rule, not torch's
    draws: MILModel(...) under torch.manual_seed(seed) holds other numbers."""
    g = np.random.Generator(np.random.PCG64(int(seed)))
    lin = lambda fan_out, fan_in: (g.uniform(-1, 1, (fan_out, fan_in)) / np.sqrt(fan_in), g.uniform(-1, 1, fan_out) / np.sqrt(fan_in))
    E = g.standard_normal((66, 2))
    W1, b1 = lin(150, 15)
    W2, b2 = lin(32, 150)
    W3, b3 = lin(1, 32)
    parts = [E, W1, b1, np.ones(150), np.zeros(150), np.zeros(150), np.ones(150), W2, b2, W3, b3]
    return np.concatenate([np.asarray(p, np.float64).ravel() for p in parts]).astype(np.float32)


_libc = None


def _hint_huge_pages(a):
    """A fresh output array is first touched by the library's copy threads; with 4 KB pages that is tens of
    thousands of page faults (80 MB of read probabilities per million sites).  Ask for transparent huge pages on
    its 2 MB-aligned interior -- best effort, any failure is ignored."""
    global _libc
    if a.nbytes < (8 << 20):
        return
    try:
        if _libc is None:
            _libc = C.CDLL(None, use_errno=True)
            _libc.madvise.argtypes = [C.c_void_p, C.c_size_t, C.c_int]
        lo = (a.ctypes.data + (1 << 21) - 1) & ~((1 << 21) - 1)
        hi = (a.ctypes.data + a.nbytes) & ~((1 << 21) - 1)
        if hi > lo:
            _libc.madvise(lo, hi - lo, 14)          # MADV_HUGEPAGE
    except Exception:
        pass


def _is_torch(x):
    return type(x).__module__.startswith("torch")


def pinned_empty(shape, dtype=np.float32):
    """A NumPy array in page-locked host memory (m6a_host_alloc): what the host-pointer calls DMA in place instead of copying
    through the staging ring -- for callers without torch.  Freed when the array (and every view of it) is gone."""
    import weakref
    L = _lib.load()
    dt = np.dtype(dtype)
    n = int(np.prod(shape)) * dt.itemsize
    p = C.c_void_p()
    rc = L.m6a_host_alloc(max(n, 1), C.byref(p))
    if rc != 0:
        raise _lib.M6AError(rc, "m6a_host_alloc(%d bytes)" % n)
    buf = (C.c_char * max(n, 1)).from_address(p.value)
    weakref.finalize(buf, L.m6a_host_free, C.c_void_p(p.value))
    return np.frombuffer(buf, dtype=dt, count=int(np.prod(shape))).reshape(shape)


class _Arg:
    """Pointer + keep-alive for one array argument."""

    def __init__(self, x, dtype, torch_dtype_name):
        self.is_dev = False
        if _is_torch(x):
            import torch
            want = getattr(torch, torch_dtype_name)
            if x.dtype != want or not x.is_contiguous():
                raise TypeError("tensor must be contiguous %s" % torch_dtype_name)
            self.keep = x
            self.ptr = x.data_ptr()
            self.is_dev = x.is_cuda
            self.size = x.numel()
        else:
            a = np.ascontiguousarray(x, dtype)
            self.keep = a
            self.ptr = a.ctypes.data
            self.size = a.size


# the four outputs of the calls on pairs of sites (_site_pairs): gt, eq, tie, z and d_pos, d_neg, med_a, med_b
_RANKSUM_OUT = ((np.int64, "int64"),) * 3 + ((np.float64, "float64"),)
_KS_OUT = ((np.int64, "int64"),) * 2 + ((np.float64, "float64"),) * 2


class M6ANetEngine:
    def __init__(self, weights=None, pretrained_model=DEFAULT_PRETRAINED_MODEL, device=0):
        self._L = _lib.load()
        if weights is None:
            weights = load_weights(pretrained_model)
        w = np.ascontiguousarray(weights, np.float32)
        if w.size != N_WEIGHT_FLOATS:
            raise ValueError("weights must have %d floats" % N_WEIGHT_FLOATS)
        if isinstance(device, str):
            device = int(device.split(":")[1]) if ":" in device else 0
        self.device = int(device)
        h = C.c_void_p()
        rc = self._L.m6a_create(C.byref(h), w.ctypes.data, w.size, self.device)
        if rc != 0:
            raise _lib.M6AError(rc, self._L.m6a_last_error(None).decode())
        self._h = h

    # -- plumbing ---------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None):
            self._L.m6a_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc != 0:
            raise _lib.M6AError(rc, self._L.m6a_last_error(self._h).decode())

    def set_stream(self, stream_handle):
        self._chk(self._L.m6a_set_stream(self._h, C.c_void_p(stream_handle or 0)))
        self._torch_stream = None

    def use_torch_stream(self):
        import torch
        st = torch.cuda.current_stream(self.device)
        self.set_stream(st.cuda_stream)
        self._torch_stream = st.cuda_stream

    def set_job_offset(self, first_site):
        """The sites given to calculate_site_proba/infer are sites [first_site, ...) of a larger
        job (multi-GPU shards): flush groups and RNG restarts follow the job's batch indices."""
        self._chk(self._L.m6a_set_job_offset(self._h, int(first_site)))

    def set_encoder_variant(self, mode):
        """0 auto = the 16-slot kernels (the reference's operation order, its bits), 1 the same said explicitly, 2 the 12-slot
        kernel (opt-in; needs every bag >= 16 reads), 3 the 16-slot arithmetic behind the per-lane walk of off[] even when the
        scalar site chain would do (A/B, tests), 4 fast: the 12-slot kernel where every bag has >= 16 reads, 16-slot elsewhere."""
        self._chk(self._L.m6a_set_encoder_variant(self._h, int(mode)))

    @property
    def last_encoder_variant(self):
        return self._L.m6a_last_encoder_variant(self._h).decode()

    @property
    def last_encoder_kernel(self):
        """Name of the __global__ function the last encode launched (enc_kernel | enc_site16_kernel | enc_csite_kernel | enc_repr_kernel)."""
        return self._L.m6a_last_encoder_kernel(self._h).decode()

    def set_scan_driver(self, mode):
        """Ragged bags: 0 auto, 1 one wavefront per flush group, 2 counting pass + one wavefront per site, 3 index tables."""
        self._chk(self._L.m6a_set_scan_driver(self._h, int(mode)))

    def set_table_variant(self, mode):
        """Uniform bags: 0 auto, 1 LDS-gather kernel, 2 register kernel."""
        self._chk(self._L.m6a_set_table_variant(self._h, int(mode)))

    def sync(self):
        self._chk(self._L.m6a_sync(self._h))

    def set_host_offsets(self, off_host):
        """For the NEXT call with device tensors: the host copy (numpy int64 [S+1]) of its CSR offsets.  The call then
        takes the bag statistics from it, does not block on the stream, and only checks the device array against it
        (a mismatch is reported by the next `sync()`).  include/m6a.h: m6a_set_host_offsets."""
        if off_host is None:
            self._chk(self._L.m6a_set_host_offsets(self._h, None))
            return
        a = np.ascontiguousarray(off_host, dtype=np.int64)
        self._host_off_keepalive = a                      # read inside the next call
        self._chk(self._L.m6a_set_host_offsets(self._h, a.ctypes.data))

    # -- the multi-GPU exchange on the library's own RCCL communicator (include/m6a.h: m6a_gather) --------
    def comm_init(self, unique_id, rank, world_size):
        """unique_id: the 128 bytes rank 0 got from `comm_unique_id()`, handed to every rank by the launcher."""
        buf = (C.c_char * 128).from_buffer_copy(bytes(unique_id))
        self._chk(self._L.m6a_comm_init(self._h, buf, int(rank), int(world_size)))
        self._comm = (int(rank), int(world_size))

    def comm_info(self):
        """What the communicator itself reports: {'ranks_seen': ncclCommCount, 'rank', 'device', 'rccl_version'}."""
        n, r, d, v = C.c_int(0), C.c_int(-1), C.c_int(-1), C.c_int(0)
        self._chk(self._L.m6a_comm_count(self._h, C.byref(n)))
        self._chk(self._L.m6a_comm_info(self._h, C.byref(r), C.byref(d), C.byref(v)))
        return {"ranks_seen": n.value, "rank": r.value, "device": d.value, "rccl_version": v.value}

    def comm_destroy(self):
        self._chk(self._L.m6a_comm_destroy(self._h))

    def gather(self, site, mod, cuts, dst=0, out=None):
        """site_prob / mod_ratio of this rank's shard to rank `dst` in ONE grouped RCCL exchange on the context's
        stream; returns (site_all, mod_all) on dst, (None, None) elsewhere.  torch tensors on the context's GPU
        (stream-ordered: `sync()` before reading) or numpy arrays (staged by the library, synchronous)."""
        rank, world = self._comm
        cuts = np.ascontiguousarray(cuts, np.int64)
        assert cuts.size == world + 1
        aS, aM = _Arg(site, np.float32, "float32"), _Arg(mod, np.float64, "float64")
        total = int(cuts[-1] - cuts[0])
        sa = ma = None
        if rank == dst:
            sa, ma = out if out is not None else (self._out(aS.is_dev, total, np.float32, "float32"),
                                                  self._out(aS.is_dev, total, np.float64, "float64"))
        oS = _Arg(sa, np.float32, "float32") if sa is not None else None
        oM = _Arg(ma, np.float64, "float64") if ma is not None else None
        self._chk(self._L.m6a_gather(self._h, aS.ptr, aM.ptr, cuts.ctypes.data, int(dst),
                                     oS.ptr if oS else None, oM.ptr if oM else None))
        return sa, ma

    def gather_reads(self, read_prob, read_cuts, dst=0, out=None):
        """The per-read output of this rank's shard to rank `dst` (include/m6a.h: m6a_gather_reads); read_cuts [world+1]
        = off[site cuts] of the job's CSR offsets.  Returns read_all on dst, None elsewhere."""
        rank, world = self._comm
        cuts = np.ascontiguousarray(read_cuts, np.int64)
        assert cuts.size == world + 1
        aP = _Arg(read_prob, np.float32, "float32")
        ra = None
        if rank == dst:
            ra = out if out is not None else self._out(aP.is_dev, int(cuts[-1] - cuts[0]), np.float32, "float32")
        oP = _Arg(ra, np.float32, "float32") if ra is not None else None
        self._chk(self._L.m6a_gather_reads(self._h, aP.ptr, cuts.ctypes.data, int(dst), oP.ptr if oP else None))
        return ra

    def random_stream(self, seed, n_words):
        """First n_words uint32 outputs of NumPy's legacy generator after np.random.seed(seed), generated on the GPU
        (include/m6a.h: m6a_random_stream): np.frombuffer(np.random.RandomState(seed).bytes(4 * n), np.uint32)."""
        out = np.empty(int(n_words), np.uint32)
        self._chk(self._L.m6a_random_stream(self._h, int(seed) & 0xffffffff, int(n_words), out.ctypes.data))
        return out

    def prepare_host_io(self):
        """Pin the staging ring of the host-pointer path now (otherwise the first numpy-array call does it)."""
        self._chk(self._L.m6a_prepare_host_io(self._h))

    def profile(self, on=True):
        """HIP-event timing of the launches: False off, True both kernels, 'encoder' / 'pooling' one kind."""
        self._chk(self._L.m6a_profile_enable(self._h, {False: 0, True: 1, 'encoder': 2, 'pooling': 3}[on]))

    def profile_read(self, kind):
        ms, n = C.c_double(), C.c_int64()
        self._chk(self._L.m6a_profile_read(self._h, kind, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def profile_clock(self, kind):
        """The shader clock the last PROFILED launch of `kind` (0 encoder, 1 pooling) ran at, from in-kernel stamps of up to 64
        waves (m6a_profile_clock): {'ghz': median, 'ghz_min', 'ghz_max', 'span_ms', 'waves'}; None if nothing was stamped."""
        g, lo, hi, span, n = C.c_double(), C.c_double(), C.c_double(), C.c_double(), C.c_int32()
        self._chk(self._L.m6a_profile_clock(self._h, kind, C.byref(g), C.byref(lo), C.byref(hi), C.byref(span), C.byref(n)))
        if n.value == 0:
            return None
        return {"ghz": g.value, "ghz_min": lo.value, "ghz_max": hi.value, "span_ms": span.value, "waves": n.value}

    @property
    def last_pool_variant(self):
        return self._L.m6a_last_pool_variant(self._h).decode()

    def _out(self, like_dev, n, np_dtype, torch_name):
        if like_dev:
            import torch
            return torch.empty(n, dtype=getattr(torch, torch_name), device="cuda:%d" % self.device)
        a = np.empty(n, np_dtype)
        _hint_huge_pages(a)
        return a

    # -- the path ---------------------------------------------------------------------------
    def get_read_probability(self, X, site_kmers, off, out=None):
        aX, aK, aO = _Arg(X, np.float32, "float32"), _Arg(site_kmers, np.uint8, "uint8"), _Arg(off, np.int64, "int64")
        S = aO.size - 1
        R = aX.size // 9
        if aK.size != 3 * S:
            raise ValueError("site_kmers must be [n_sites, 3]")
        rp = out if out is not None else self._out(aX.is_dev, R, np.float32, "float32")
        aP = _Arg(rp, np.float32, "float32")
        if aP.size != R:
            raise ValueError("read_prob must have one float per read")
        self._chk(self._L.m6a_encode_reads(self._h, aX.ptr, aK.ptr, aO.ptr, S, aP.ptr))
        return rp

    def get_read_representation(self, X, site_kmers, off, out=None, want_read_probs=False, dtype="float32"):
        """MILModel.get_read_representation (m6anet/model/model.py:85-97): layer 2 after its ReLU, float32 [R, 32], the
        reference's bits whatever encoder variant is selected (include/m6a.h: m6a_read_representation).  `out` = a
        preallocated [R, 32] array or tensor, or the pair (repr, read_prob).  Returns repr, or
        (repr, read_prob [R]) with want_read_probs.  dtype="float16" (m6a_read_representation_dtype, M6A_REPR_F16): repr is
        np.float16 / torch.half, exactly the float32 result's .astype(np.float16), converted in the kernel; read_prob stays
        float32."""
        if dtype not in _lib.REPR_DTYPES:
            raise ValueError("dtype must be 'float32' or 'float16', not %r" % (dtype,))
        np_dt = np.float16 if dtype == "float16" else np.float32
        aX, aK, aO = _Arg(X, np.float32, "float32"), _Arg(site_kmers, np.uint8, "uint8"), _Arg(off, np.int64, "int64")
        S = aO.size - 1
        R = aX.size // 9
        if aK.size != 3 * S:
            raise ValueError("site_kmers must be [n_sites, 3]")
        rep, rp = out if isinstance(out, (tuple, list)) else (out, None)
        if rep is None:
            rep = self._out(aX.is_dev, R * N_REPR, np_dt, dtype).reshape(R, N_REPR)
        if want_read_probs and rp is None:
            rp = self._out(aX.is_dev, R, np.float32, "float32")
        for o, dt, name in ((rep, np_dt, dtype), (rp, np.float32, "float32")):   # an output the binding would have to copy is an error, not a copy
            if o is not None and not _is_torch(o) and not (isinstance(o, np.ndarray) and o.dtype == dt and o.flags.c_contiguous):
                raise TypeError("out must be C-contiguous %s" % name)
        aH = _Arg(rep, np_dt, dtype)
        aP = _Arg(rp, np.float32, "float32") if rp is not None else None
        if aH.size != R * N_REPR:
            raise ValueError("repr must be [n_reads, %d]" % N_REPR)
        if aP is not None and aP.size != R:
            raise ValueError("read_prob must have one float per read")
        if dtype == "float32":
            self._chk(self._L.m6a_read_representation(self._h, aX.ptr, aK.ptr, aO.ptr, S, aH.ptr, aP.ptr if aP else None))
        else:
            self._chk(self._L.m6a_read_representation_dtype(self._h, aX.ptr, aK.ptr, aO.ptr, S, aH.ptr, _lib.REPR_DTYPES[dtype],
                                                            aP.ptr if aP else None))
        return (rep, rp) if want_read_probs else rep

    def read_representation_ptrs(self, X, site_kmers, off, n_sites, repr, dtype="float32", read_prob=None):
        """m6a_read_representation_dtype on raw addresses (ints) the caller owns, as infer_ptrs is m6a_infer on them: all host or
        all device; repr holds [R][32] of `dtype` ("float32" | "float16", or M6A_REPR_F32 | M6A_REPR_F16 -- any other number is
        passed on and refused by the library), read_prob [R] float32 or None.  With device pointers the call is queued on the
        context's stream: `sync()` before repr is read; `set_host_offsets` first spares the read-back of off."""
        code = _lib.REPR_DTYPES[dtype] if isinstance(dtype, str) else int(dtype)
        self._chk(self._L.m6a_read_representation_dtype(self._h, X, site_kmers, off, int(n_sites), repr, code, read_prob))

    def calculate_site_proba(self, read_probs, off, n_iters, n_samples=N_SAMPLES,
                             read_proba_threshold=DEFAULT_READ_THRESHOLD, seed=0, batch_size=16,
                             save_per_batch=2):
        """Returns (site_probs float32 [S], mod_ratios float64 [S])."""
        aP, aO = _Arg(read_probs, np.float32, "float32"), _Arg(off, np.int64, "int64")
        S = aO.size - 1
        site = self._out(aP.is_dev, S, np.float32, "float32")
        mod = self._out(aP.is_dev, S, np.float64, "float64")
        aS, aM = _Arg(site, np.float32, "float32"), _Arg(mod, np.float64, "float64")
        self._chk(self._L.m6a_site_pool(self._h, aP.ptr, aO.ptr, S, int(n_iters), int(n_samples),
                                        float(np.float32(read_proba_threshold)), int(seed) & 0xffffffff,
                                        _lib.RNG_NUMPY, int(batch_size), int(save_per_batch), aS.ptr, aM.ptr))
        return site, mod

    SITE_MODES = {"sampled": 0, "expected": 1}            # M6A_SITE_SAMPLED / M6A_SITE_EXPECTED (include/m6a.h)

    def set_site_mode(self, mode):
        """What site_probs means in calculate_site_proba / infer / job_end on this engine.  "sampled" (the default): the replay of
        the reference's random draws.  "expected": the closed form those draws estimate, 1 - mean(1 - p)^n_samples -- n_iters,
        seed, batch_size and save_per_batch are still checked and otherwise have no effect (include/m6a.h: m6a_set_site_mode)."""
        if mode not in self.SITE_MODES:
            raise ValueError("site mode must be 'sampled' or 'expected', not %r" % (mode,))
        self._chk(self._L.m6a_set_site_mode(self._h, self.SITE_MODES[mode]))

    def site_expectation(self, read_probs, off, n_samples=N_SAMPLES, want_sigma=False, read_proba_threshold=DEFAULT_READ_THRESHOLD):
        """The closed-form site probability (include/m6a.h: m6a_site_expectation), whatever the engine's site mode.  Returns
        (site_probs float32 [S], mod_ratios float64 [S]) or, with want_sigma, (site_probs, mod_ratios, mc_sigma float64 [S]):
        mc_sigma / sqrt(n_iters) is the standard error of the sampled mode's site probability."""
        aP, aO = _Arg(read_probs, np.float32, "float32"), _Arg(off, np.int64, "int64")
        S = aO.size - 1
        site = self._out(aP.is_dev, S, np.float32, "float32")
        mod = self._out(aP.is_dev, S, np.float64, "float64")
        sigma = self._out(aP.is_dev, S, np.float64, "float64") if want_sigma else None
        aS, aM = _Arg(site, np.float32, "float32"), _Arg(mod, np.float64, "float64")
        aG = _Arg(sigma, np.float64, "float64") if want_sigma else None
        self._chk(self._L.m6a_site_expectation(self._h, aP.ptr, aO.ptr, S, int(n_samples), float(np.float32(read_proba_threshold)),
                                               aS.ptr, aM.ptr, aG.ptr if aG else None))
        return (site, mod, sigma) if want_sigma else (site, mod)

    def site_ranksum(self, read_probs_a, off_a, read_probs_b, off_b, pair_a=None, pair_b=None):
        """The rank-sum test between two sets of sites (include/m6a.h: m6a_site_ranksum): pair k compares the reads of site pair_a[k]
        of the first set with those of site pair_b[k] of the second; without the two index arrays site k is compared with site k.
        NumPy arrays (synchronous) or torch tensors on the GPU (queued: `sync()` before reading), all of one kind.  Returns
        (gt, eq, tie int64 [P], z float64 [P]); an undefined pair -- an empty bag, a NaN, more than 2^20 pooled reads -- is
        (-1, -1, -1, NaN).  m6anet_amd/ranksum.py turns them into p, q and the AUC."""
        return self._site_pairs(1, self.site_ranksum_ptrs, _RANKSUM_OUT, read_probs_a, off_a, read_probs_b, off_b, pair_a, pair_b)

    def site_ranksum_ptrs(self, prob_a, off_a, n_sites_a, prob_b, off_b, n_sites_b, pair_a, pair_b, n_pairs, gt, eq, tie, z):
        """m6a_site_ranksum on raw addresses (ints) the caller owns, as infer_ptrs is m6a_infer on them -- e.g. the read_prob and off
        of two m6a_prep_sites handles after infer_ptrs has filled them: all host or all device; pair_a / pair_b and gt / eq / tie may
        be None.  With device pointers the call is queued on the context's stream: `sync()` before the outputs are read."""
        self._chk(self._L.m6a_site_ranksum(self._h, prob_a, off_a, int(n_sites_a), prob_b, off_b, int(n_sites_b), pair_a, pair_b,
                                           int(n_pairs), gt, eq, tie, z))

    def site_signal_ranksum(self, X_a, off_a, X_b, off_b, pair_a=None, pair_b=None):
        """The rank-sum test on each of the nine signal features (include/m6a.h: m6a_site_signal_ranksum): site_ranksum on every
        column of X_a [Ra, 9] and X_b [Rb, 9] -- dwell_time, norm_std, norm_mean at positions -1, 0, +1 -- with off_* in rows.  NumPy
        arrays (synchronous) or torch tensors on the GPU (queued: `sync()` before reading), all of one kind.  Returns (gt, eq, tie
        int64 [P, 9], z float64 [P, 9]); a NaN leaves its own column of the pair undefined, an empty bag or more than 2^20 pooled
        reads all nine.  m6anet_amd/ranksum.py (signal_rows) turns them into p, q and the AUC."""
        return self._site_pairs(9, self.site_signal_ranksum_ptrs, _RANKSUM_OUT, X_a, off_a, X_b, off_b, pair_a, pair_b)

    def site_signal_ranksum_ptrs(self, X_a, off_a, n_sites_a, X_b, off_b, n_sites_b, pair_a, pair_b, n_pairs, gt, eq, tie, z):
        """m6a_site_signal_ranksum on raw addresses (ints) the caller owns, as site_ranksum_ptrs is m6a_site_ranksum on them -- e.g. the
        X and off of two m6a_prep_sites handles: all host or all device; pair_a / pair_b and gt / eq / tie may be None; the outputs
        hold nine values per pair.  With device pointers the call is queued on the context's stream: `sync()` before they are read."""
        self._chk(self._L.m6a_site_signal_ranksum(self._h, X_a, off_a, int(n_sites_a), X_b, off_b, int(n_sites_b), pair_a, pair_b,
                                                  int(n_pairs), gt, eq, tie, z))

    def _site_pairs(self, cols, call, out_dtypes, v_a, off_a, v_b, off_b, pair_a, pair_b):
        """The four calls on pairs of sites: a bag's element is `cols` float32 (1: a value, 9: a row of X), `call` the *_ptrs method and
        out_dtypes its four outputs' (NumPy dtype, name); [P] for cols == 1, [P, cols] otherwise."""
        if (pair_a is None) != (pair_b is None):
            raise ValueError("pair_a and pair_b are given together or not at all")
        aVa, aOa = _Arg(v_a, np.float32, "float32"), _Arg(off_a, np.int64, "int64")
        aVb, aOb = _Arg(v_b, np.float32, "float32"), _Arg(off_b, np.int64, "int64")
        if aVa.size % cols or aVb.size % cols:                   # (cols is 1 or 9)
            raise ValueError("X_a and X_b hold nine float32 per read")
        Sa, Sb = aOa.size - 1, aOb.size - 1
        aIa = _Arg(pair_a, np.int64, "int64") if pair_a is not None else None
        aIb = _Arg(pair_b, np.int64, "int64") if pair_b is not None else None
        if aIa is not None and aIa.size != aIb.size:
            raise ValueError("pair_a and pair_b must have one entry per pair")
        if aIa is None and Sa != Sb:
            raise ValueError("without pair_a / pair_b the two sets must have the same number of sites")
        P = aIa.size if aIa is not None else Sa
        out = [self._out(aVa.is_dev, P * cols, dt, name) for dt, name in out_dtypes]
        ptrs = [_Arg(o, dt, name).ptr for o, (dt, name) in zip(out, out_dtypes)]
        call(aVa.ptr, aOa.ptr, Sa, aVb.ptr, aOb.ptr, Sb, aIa.ptr if aIa else None, aIb.ptr if aIb else None, P, *ptrs)
        return tuple(out) if cols == 1 else tuple(o.reshape(P, cols) for o in out)

    def site_ks(self, read_probs_a, off_a, read_probs_b, off_b, pair_a=None, pair_b=None):
        """The Kolmogorov-Smirnov integers and the medians of pairs of sites (include/m6a.h: m6a_site_ks), shaped like site_ranksum:
        NumPy arrays (synchronous) or torch tensors on the GPU (queued: `sync()` before reading), all of one kind.  Returns (d_pos,
        d_neg int64 [P], med_a, med_b float64 [P]); an undefined pair -- an empty bag, a NaN, more than 2^20 pooled reads -- is
        (-1, -1, NaN, NaN).  m6anet_amd/ranksum.py turns them into D, its sign, p and q."""
        return self._site_pairs(1, self.site_ks_ptrs, _KS_OUT, read_probs_a, off_a, read_probs_b, off_b, pair_a, pair_b)

    def site_ks_ptrs(self, prob_a, off_a, n_sites_a, prob_b, off_b, n_sites_b, pair_a, pair_b, n_pairs, d_pos, d_neg, med_a, med_b):
        """m6a_site_ks on raw addresses (ints) the caller owns, as site_ranksum_ptrs is m6a_site_ranksum on them: all host or all device;
        pair_a / pair_b and med_a / med_b may be None.  With device pointers the call is queued on the context's stream: `sync()`
        before the outputs are read."""
        self._chk(self._L.m6a_site_ks(self._h, prob_a, off_a, int(n_sites_a), prob_b, off_b, int(n_sites_b), pair_a, pair_b,
                                      int(n_pairs), d_pos, d_neg, med_a, med_b))

    def site_signal_ks(self, X_a, off_a, X_b, off_b, pair_a=None, pair_b=None):
        """site_ks on each of the nine signal features (include/m6a.h: m6a_site_signal_ks), shaped like site_signal_ranksum: X_a [Ra, 9]
        and X_b [Rb, 9] with off_* in rows.  Returns (d_pos, d_neg int64 [P, 9], med_a, med_b float64 [P, 9]), the medians in the
        normalised units of X; a NaN leaves its own column of the pair undefined, an empty bag or more than 2^20 pooled reads all nine."""
        return self._site_pairs(9, self.site_signal_ks_ptrs, _KS_OUT, X_a, off_a, X_b, off_b, pair_a, pair_b)

    def site_signal_ks_ptrs(self, X_a, off_a, n_sites_a, X_b, off_b, n_sites_b, pair_a, pair_b, n_pairs, d_pos, d_neg, med_a, med_b):
        """m6a_site_signal_ks on raw addresses (ints) the caller owns, as site_ks_ptrs is m6a_site_ks on them; the outputs hold nine
        values per pair."""
        self._chk(self._L.m6a_site_signal_ks(self._h, X_a, off_a, int(n_sites_a), X_b, off_b, int(n_sites_b), pair_a, pair_b,
                                             int(n_pairs), d_pos, d_neg, med_a, med_b))

    def ks_exact(self, n, m, h):
        """The exact two-sided Kolmogorov-Smirnov p-value of every item (include/m6a.h: m6a_ks_exact): n and m the two bag sizes and
        h = max(d_pos, d_neg) of site_ks / site_signal_ks (m6anet_amd/ranksum.py: ks_h), the statistic in units of 1 / (n m) -- what
        scipy.stats.ks_2samp(method="exact") returns.  int64 NumPy arrays (synchronous) or torch tensors on the GPU (queued: `sync()`
        before reading), all of one kind and one size.  Returns p float64 of n's shape; NaN where the item is undefined: an empty bag,
        h < 0 (the undefined pair of site_ks), min(n, m) > 2047 or n m > 10^8."""
        aN, aM, aH = (_Arg(x, np.int64, "int64") for x in (n, m, h))
        if not aN.size == aM.size == aH.size:
            raise ValueError("n, m and h must have one entry per item")
        p = self._out(aN.is_dev, aN.size, np.float64, "float64")
        self.ks_exact_ptrs(aN.ptr, aM.ptr, aH.ptr, aN.size, _Arg(p, np.float64, "float64").ptr)
        return p.reshape(tuple(aN.keep.shape))

    def ks_exact_ptrs(self, n, m, h, count, p):
        """m6a_ks_exact on raw addresses (ints) the caller owns: all host or all device.  With device pointers the call is queued on
        the context's stream: `sync()` before p is read."""
        self._chk(self._L.m6a_ks_exact(self._h, n, m, h, int(count), p))

    def infer(self, X, site_kmers, off, n_iters, n_samples=N_SAMPLES,
              read_proba_threshold=DEFAULT_READ_THRESHOLD, seed=0, batch_size=16, save_per_batch=2,
              want_read_probs=True, out=None):
        """Returns (read_probs or None, site_probs, mod_ratios).  `out` = preallocated
        (read_probs|None, site_probs, mod_ratios) to reuse buffers across calls."""
        aX, aK, aO = _Arg(X, np.float32, "float32"), _Arg(site_kmers, np.uint8, "uint8"), _Arg(off, np.int64, "int64")
        S = aO.size - 1
        R = aX.size // 9
        if out is not None:
            rp, site, mod = out
        else:
            rp = self._out(aX.is_dev, R, np.float32, "float32") if want_read_probs else None
            site = self._out(aX.is_dev, S, np.float32, "float32")
            mod = self._out(aX.is_dev, S, np.float64, "float64")
        aP = _Arg(rp, np.float32, "float32") if rp is not None else None
        aS, aM = _Arg(site, np.float32, "float32"), _Arg(mod, np.float64, "float64")
        self.infer_ptrs(aX.ptr, aK.ptr, aO.ptr, S, n_iters, n_samples, read_proba_threshold, seed, batch_size, save_per_batch,
                        aP.ptr if aP else None, aS.ptr, aM.ptr)
        return rp, site, mod

    def infer_ptrs(self, X, site_kmers, off, n_sites, n_iters, n_samples=N_SAMPLES, read_proba_threshold=DEFAULT_READ_THRESHOLD,
                   seed=0, batch_size=16, save_per_batch=2, read_prob=None, site_prob=None, mod_ratio=None):
        """m6a_infer on raw addresses (ints) the caller owns -- e.g. the device arrays of m6a_prep_sites_build: all host or all
        device, as include/m6a.h says.  With device pointers the call is queued on the context's stream: `sync()` before the
        outputs are read; `set_host_offsets` first spares the read-back of off."""
        self._chk(self._L.m6a_infer(self._h, X, site_kmers, off, int(n_sites), int(n_iters), int(n_samples),
                                    float(np.float32(read_proba_threshold)), int(seed) & 0xffffffff,
                                    _lib.RNG_NUMPY, int(batch_size), int(save_per_batch), read_prob, site_prob, mod_ratio))

    # -- the same job, streamed: run_inference's batch loop (inference_utils.py:33-54) feeds as the loader produces --------
    def job_begin(self, n_iters, n_samples=N_SAMPLES, read_proba_threshold=DEFAULT_READ_THRESHOLD, seed=0, batch_size=16,
                  save_per_batch=2, expect_sites=0, expect_reads=0):
        """Opens a streaming job (include/m6a.h: m6a_job_begin); feed batches with `job_feed`, finish with `job_end`."""
        self._chk(self._L.m6a_job_begin(self._h, int(n_iters), int(n_samples), float(np.float32(read_proba_threshold)),
                                        int(seed) & 0xffffffff, _lib.RNG_NUMPY, int(batch_size), int(save_per_batch),
                                        int(expect_sites), int(expect_reads)))
        self._job_dev = False
        self._job_keep = []                                  # device tensors fed to the open job (released by job_end / job_abort)

    def job_feed(self, X, site_kmers, off):
        """One batch: X [r,9], site_kmers [n,3] (numpy or torch-on-GPU), off [n+1] batch-local CSR offsets (host).
        Asynchronous.  HOST arrays are copied into the pinned ring: they are the caller's again on return.  DEVICE tensors
        are read in place by the encoder queued on the context's stream, possibly after this call has returned
        (include/m6a.h): the engine keeps them referenced until job_end / job_abort, so the caching allocator cannot hand
        their memory to the next batch, and -- unless the context runs on the very stream torch is producing on
        (use_torch_stream) -- waits for torch's current stream first, so whatever wrote them is done before the encoder
        reads."""
        aX, aK = _Arg(X, np.float32, "float32"), _Arg(site_kmers, np.uint8, "uint8")
        if aX.is_dev or aK.is_dev:
            import torch
            cur = torch.cuda.current_stream(self.device)
            if getattr(self, "_torch_stream", None) != cur.cuda_stream:
                cur.synchronize()
            self._job_keep.append((aX.keep, aK.keep))
        o = off if (isinstance(off, np.ndarray) and off.dtype == np.int64 and off.flags.c_contiguous) else \
            np.ascontiguousarray(off.cpu().numpy() if _is_torch(off) else off, dtype=np.int64)
        n = o.size - 1
        if aK.size != 3 * n or aX.size != 9 * int(o[-1]):
            raise ValueError("batch shapes disagree: X [off[-1], 9], site_kmers [n_sites, 3], off [n_sites + 1]")
        self._job_dev = self._job_dev or aX.is_dev
        self._chk(self._L.m6a_job_feed(self._h, aX.ptr, aK.ptr, o.ctypes.data, n))

    def job_feed_collated(self, features, kmers, n_reads):
        """One batch exactly as the reference's inference_collate builds it (m6anet/utils/data_utils.py:498-506): features
        [r,9] float32, kmers [r,3] int64 (per READ), n_reads [n] int64 -- host tensors or arrays; nothing is converted here."""
        aX, aK, aN = _Arg(features, np.float32, "float32"), _Arg(kmers, np.int64, "int64"), _Arg(n_reads, np.int64, "int64")
        if aX.is_dev or aK.is_dev or aN.is_dev:
            raise TypeError("job_feed_collated takes the collate's host tensors")
        if aK.size * 3 != aX.size:
            raise ValueError("batch shapes disagree: features [r, 9], kmers [r, 3]")
        self._chk(self._L.m6a_job_feed_collated(self._h, aX.ptr, aK.ptr, aN.ptr, aN.size))

    def job_size(self):
        S, R = C.c_int64(), C.c_int64()
        self._chk(self._L.m6a_job_size(self._h, C.byref(S), C.byref(R)))
        return S.value, R.value

    def job_end(self, want_read_probs=True, device_outputs=None):
        """Pools everything fed and returns (read_probs or None, site_probs, mod_ratios) -- numpy arrays, or torch
        tensors on the GPU when the job was fed device tensors (or device_outputs=True)."""
        S, R = self.job_size()
        dev = self._job_dev if device_outputs is None else bool(device_outputs)
        rp = self._out(dev, R, np.float32, "float32") if want_read_probs else None
        site = self._out(dev, S, np.float32, "float32")
        mod = self._out(dev, S, np.float64, "float64")
        aP = _Arg(rp, np.float32, "float32") if rp is not None else None
        aS, aM = _Arg(site, np.float32, "float32"), _Arg(mod, np.float64, "float64")
        try:
            self._chk(self._L.m6a_job_end(self._h, aP.ptr if aP else None, aS.ptr, aM.ptr))     # synchronises: every encoder has read its rows
        finally:
            self._job_keep = []
        return rp, site, mod

    def job_abort(self):
        try:
            self._chk(self._L.m6a_job_abort(self._h))
            self.sync()                                      # queued encoders may still be reading device batches
        finally:
            self._job_keep = []

    def forward(self, X, kmer, bag=N_SAMPLES):
        """Site probability of fixed-size bags: X [B, bag, 9], kmer [B, 3] -> [B]."""
        aX, aK = _Arg(X, np.float32, "float32"), _Arg(kmer, np.uint8, "uint8")
        B = aK.size // 3
        if aX.size != B * bag * 9:
            raise ValueError("X must be [B, bag, 9]")
        site = self._out(aX.is_dev, B, np.float32, "float32")
        aS = _Arg(site, np.float32, "float32")
        self._chk(self._L.m6a_bag_forward(self._h, aX.ptr, aK.ptr, B, int(bag), aS.ptr))
        return site


    def trainer(self, weights=None, lr=4e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, clip_grad=None):
        """A Trainer on this engine's device and stream (include/m6a.h: m6a_train_create), starting from `weights` (a 7 997-float
        blob; None = init_weights(0)).  The engine's own weights are not touched.  clip_grad: Trainer.set_clip's max_norm."""
        t = Trainer(self, init_weights(0) if weights is None else weights, lr, betas, eps, weight_decay)
        if clip_grad is not None:
            try:
                t.set_clip(clip_grad)
            except Exception:
                t.close()
                raise
        return t

    def validate_pool(self, read_probs, off, n_iterations=1, n_samples=N_SAMPLES, seed=0):
        """The prediction part of the reference's `validate` (training_utils.py:233-253) from read
        probabilities: each pass samples n_samples reads per site without replacement
        (data_utils.py:213-214).  Returns (y_pred float32 [n_iterations, S], y_pred_avg float32 [S])."""
        aP, aO = _Arg(read_probs, np.float32, "float32"), _Arg(off, np.int64, "int64")
        S = aO.size - 1
        y = self._out(aP.is_dev, int(n_iterations) * S, np.float32, "float32")
        avg = self._out(aP.is_dev, S, np.float32, "float32")
        aY, aA = _Arg(y, np.float32, "float32"), _Arg(avg, np.float32, "float32")
        self._chk(self._L.m6a_validate_pool(self._h, aP.ptr, aO.ptr, S, int(n_iterations), int(n_samples),
                                            int(seed) & 0xffffffff, aY.ptr, aA.ptr))
        return y.reshape(int(n_iterations), S), avg

    def validate_forward(self, X, site_kmers, off, n_iterations=1, n_samples=N_SAMPLES, seed=0, want_read_probs=False):
        """Encoder + validate_pool in one call.  Returns (y_pred, y_pred_avg[, read_probs])."""
        aX, aK, aO = _Arg(X, np.float32, "float32"), _Arg(site_kmers, np.uint8, "uint8"), _Arg(off, np.int64, "int64")
        S = aO.size - 1
        R = aX.size // 9
        y = self._out(aX.is_dev, int(n_iterations) * S, np.float32, "float32")
        avg = self._out(aX.is_dev, S, np.float32, "float32")
        rp = self._out(aX.is_dev, R, np.float32, "float32") if want_read_probs else None
        aY, aA = _Arg(y, np.float32, "float32"), _Arg(avg, np.float32, "float32")
        aP = _Arg(rp, np.float32, "float32") if rp is not None else None
        self._chk(self._L.m6a_validate(self._h, aX.ptr, aK.ptr, aO.ptr, S, int(n_iterations), int(n_samples),
                                       int(seed) & 0xffffffff, aP.ptr if aP else None, aY.ptr, aA.ptr))
        y = y.reshape(int(n_iterations), S)
        return (y, avg, rp) if want_read_probs else (y, avg)


class Trainer:
    """Training-mode forward, backward and Adam of the m6anet.toml model on the GPU (include/m6a.h: m6a_train_*).  Arrays are numpy
    arrays or torch tensors on the engine's GPU, all of a kind per call; with device tensors a call is queued on the engine's
    stream (`engine.sync()` before the outputs are read)."""

    def __init__(self, engine, weights, lr=4e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0):
        self._engine, self._L = engine, engine._L               # the context must outlive the trainer
        w = np.ascontiguousarray(weights, np.float32)
        if w.size != N_WEIGHT_FLOATS:
            raise ValueError("weights must have %d floats" % N_WEIGHT_FLOATS)
        cfg = _lib.TrainConfig(float(lr), float(betas[0]), float(betas[1]), float(eps), float(weight_decay))
        h = C.c_void_p()
        engine._chk(self._L.m6a_train_create(engine._h, w.ctypes.data, w.size, C.byref(cfg), C.byref(h)))
        self._h = h

    def close(self):
        if getattr(self, "_h", None) and getattr(self._engine, "_h", None):
            self._L.m6a_train_destroy(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def step(self, X, site_kmers, y, bag=N_SAMPLES):
        """One step on X [B * bag, 9], site_kmers [B, 3], y [B] (0 / 1).  Returns (loss, y_pred [B]): loss is a float for numpy
        inputs, a one-element tensor for device tensors."""
        aX, aK, aY = _Arg(X, np.float32, "float32"), _Arg(site_kmers, np.uint8, "uint8"), _Arg(y, np.float32, "float32")
        B = aY.size
        if aK.size != 3 * B or aX.size != B * int(bag) * 9:
            raise ValueError("X must be [B * bag, 9], site_kmers [B, 3], y [B]")
        loss, pred = self._engine._out(aX.is_dev, 1, np.float32, "float32"), self._engine._out(aX.is_dev, B, np.float32, "float32")
        aL, aP = _Arg(loss, np.float32, "float32"), _Arg(pred, np.float32, "float32")
        self._engine._chk(self._L.m6a_train_step(self._h, aX.ptr, aK.ptr, aY.ptr, B, int(bag), aL.ptr, aP.ptr))
        return (loss if aX.is_dev else float(loss[0])), pred

    def epoch(self, X, site_kmers, off, y, order, batch_size, bag=N_SAMPLES, seed=0):
        """One pass over `order` (site numbers, repeats allowed) in batches of batch_size, every position drawing `bag` reads of its
        site.  Returns (loss [ceil(len(order) / batch_size)], y_pred [len(order)])."""
        aX, aK, aO = _Arg(X, np.float32, "float32"), _Arg(site_kmers, np.uint8, "uint8"), _Arg(off, np.int64, "int64")
        aY, aR = _Arg(y, np.float32, "float32"), _Arg(order, np.int64, "int64")
        S = aO.size - 1
        if aK.size != 3 * S or aY.size != S:
            raise ValueError("site_kmers must be [n_sites, 3] and y [n_sites]")
        bs = int(batch_size)
        n_steps = (aR.size + bs - 1) // bs if bs > 0 else 0
        loss, pred = self._engine._out(aX.is_dev, n_steps, np.float32, "float32"), self._engine._out(aX.is_dev, aR.size, np.float32, "float32")
        aL, aP = _Arg(loss, np.float32, "float32"), _Arg(pred, np.float32, "float32")
        self._engine._chk(self._L.m6a_train_epoch(self._h, aX.ptr, aK.ptr, aO.ptr, aY.ptr, S, aR.ptr, aR.size, bs, int(bag),
                                                  int(seed) & 0xffffffffffffffff, aL.ptr, aP.ptr))
        return loss, pred

    def weights(self):
        """The blob as it stands, running statistics included: what M6ANetEngine(weights=...) and --model_state_dict x.bin take."""
        w, n = np.empty(N_WEIGHT_FLOATS, np.float32), C.c_int64()
        self._engine._chk(self._L.m6a_train_weights(self._h, w.ctypes.data, C.byref(n)))
        return w

    def grads(self):
        """The last step's gradient in blob order (zeros in the running-statistic slots)."""
        g = np.empty(N_WEIGHT_FLOATS, np.float32)
        self._engine._chk(self._L.m6a_train_grads(self._h, g.ctypes.data))
        return g

    def stats(self):
        """{'n_steps', 'n_launches', 'n_syncs'} (m6a_train_stats)."""
        a, b, c = C.c_int64(), C.c_int64(), C.c_int64()
        self._engine._chk(self._L.m6a_train_stats(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return {"n_steps": a.value, "n_launches": b.value, "n_syncs": c.value}

    def set_clip(self, max_norm):
        """Gradient clipping for every later step: torch's clip_grad_norm_(params, max_norm) between the gradient and Adam
        (include/m6a.h).  0 = off, the default."""
        self._engine._chk(self._L.m6a_train_set_clip(self._h, float(max_norm)))

    def last_norm(self):
        """The last step's total gradient norm from before the scaling (clip_grad_norm_'s return value).  Raises with clipping off."""
        v = C.c_float()
        self._engine._chk(self._L.m6a_train_last_norm(self._h, C.byref(v)))
        return float(v.value)

    def optimizer_state(self):
        """{'m', 'v', 'n_steps'}: Adam's moments in blob order (zeros in the running-statistic slots) and its step count t."""
        m, v, n = np.empty(N_WEIGHT_FLOATS, np.float32), np.empty(N_WEIGHT_FLOATS, np.float32), C.c_int64()
        self._engine._chk(self._L.m6a_train_state_get(self._h, m.ctypes.data, v.ctypes.data, C.byref(n)))
        return {"m": m, "v": v, "n_steps": int(n.value)}

    def load_optimizer_state(self, state):
        """The inverse of optimizer_state(): on a Trainer made from weights(), this is the trainer both were taken from."""
        m, v = np.ascontiguousarray(state["m"], np.float32).ravel(), np.ascontiguousarray(state["v"], np.float32).ravel()
        if m.size != N_WEIGHT_FLOATS or v.size != N_WEIGHT_FLOATS:
            raise ValueError("m and v must have %d floats" % N_WEIGHT_FLOATS)
        self._engine._chk(self._L.m6a_train_state_set(self._h, m.ctypes.data, v.ctypes.data, int(state["n_steps"])))

    # -- the step cut at s (include/m6a.h): forward gives s, backward takes dL/ds; m6anet_amd/torch_model.py puts autograd on top --
    def set_weights(self, blob):
        """The trainer's blob <- blob (7 997 floats, running statistics included; numpy, or a tensor on the engine's GPU: copied on
        the stream without a wait).  Adam's state is untouched."""
        a = _Arg(blob, np.float32, "float32")
        if a.size != N_WEIGHT_FLOATS:
            raise ValueError("weights must have %d floats" % N_WEIGHT_FLOATS)
        self._engine._chk(self._L.m6a_train_set_weights(self._h, a.ptr))

    def forward(self, X, site_kmers, bag=N_SAMPLES):
        """The first half of step(): X [B * bag, 9], site_kmers [B, 3] -> (s [B], ticket).  s and the running statistics are step()'s
        bits; no loss, no gradient, Adam's state does not move.  The ticket names the activations kept for backward()."""
        aX, aK = _Arg(X, np.float32, "float32"), _Arg(site_kmers, np.uint8, "uint8")
        B = aK.size // 3
        if aK.size != 3 * B or aX.size != B * int(bag) * 9:
            raise ValueError("X must be [B * bag, 9] and site_kmers [B, 3]")
        s, ticket = self._engine._out(aX.is_dev, B, np.float32, "float32"), C.c_int64()
        aS = _Arg(s, np.float32, "float32")
        self._engine._chk(self._L.m6a_train_forward(self._h, aX.ptr, aK.ptr, B, int(bag), 1, aS.ptr, C.byref(ticket)))
        self._kept = (int(ticket.value), B)
        return s, int(ticket.value)

    def backward(self, ticket, grad_s, out=None):
        """The backward half from the activations `ticket` names under grad_s [B] = dL/ds -> the gradient, 7 997 floats in blob order
        (zeros in the running-statistic slots).  Only the latest forward's ticket is good; the same one may be used again."""
        aG = _Arg(grad_s, np.float32, "float32")
        kept = getattr(self, "_kept", None)
        if kept and kept[0] == int(ticket) and aG.size != kept[1]:
            raise ValueError("grad_s must have one value per site of that forward (%d), not %d" % (kept[1], aG.size))
        g = self._engine._out(aG.is_dev, N_WEIGHT_FLOATS, np.float32, "float32") if out is None else out
        aO = _Arg(g, np.float32, "float32")
        if aO.size != N_WEIGHT_FLOATS:
            raise ValueError("out must have %d floats" % N_WEIGHT_FLOATS)
        self._engine._chk(self._L.m6a_train_backward(self._h, int(ticket), aG.ptr, aO.ptr))
        return g

    def running_stats(self, out=None):
        """running_mean | running_var (300 floats) out of the trainer's blob, into `out` where given (a device tensor: no wait)."""
        r = np.empty(300, np.float32) if out is None else out
        a = _Arg(r, np.float32, "float32")
        if a.size != 300:
            raise ValueError("out must have 300 floats")
        self._engine._chk(self._L.m6a_train_running_stats(self._h, a.ptr))
        return r

    def state_dict(self):
        """The reference's state_dict keys -> NumPy arrays (state_dict_from_weights), num_batches_tracked = the steps taken."""
        return state_dict_from_weights(self.weights(), self.stats()["n_steps"])


def train_sample(off, order, bag=N_SAMPLES, seed=0):
    """The global read indices [len(order) * bag] an epoch with this seed feeds, computed on the host (m6a_train_sample)."""
    off, order = np.ascontiguousarray(off, np.int64), np.ascontiguousarray(order, np.int64)
    if order.size and (order.min() < 0 or order.max() >= off.size - 1):
        raise ValueError("order holds a site outside [0, n_sites)")
    out = np.empty(order.size * int(bag), np.int64)
    rc = _lib.load().m6a_train_sample(off.ctypes.data, order.ctypes.data, order.size, int(bag), int(seed) & 0xffffffffffffffff, out.ctypes.data)
    if rc != 0:
        raise _lib.M6AError(rc, "m6a_train_sample: bag outside 1..64 or a site with fewer than bag reads")
    return out


def comm_unique_id():
    """128-byte RCCL id for `M6ANetEngine.comm_init` (call on ONE rank, broadcast to the others)."""
    buf = (C.c_char * 128)()
    L = _lib.load()
    rc = L.m6a_comm_unique_id(buf)
    if rc != 0:
        raise _lib.M6AError(rc, L.m6a_last_error(None).decode())
    return bytes(buf.raw)


LINK_TYPES = {0: "hypertransport", 1: "qpi", 2: "pcie", 3: "infiniband", 4: "xgmi"}


def device_link(dev_a, dev_b):
    """{'link': 'xgmi' | 'pcie' | ..., 'hops', 'peer_access'} between two visible HIP devices (m6a_device_link)."""
    L = _lib.load()
    lt, hc, pa = C.c_int(-1), C.c_int(-1), C.c_int(0)
    rc = L.m6a_device_link(int(dev_a), int(dev_b), C.byref(lt), C.byref(hc), C.byref(pa))
    if rc != 0:
        raise _lib.M6AError(rc, "m6a_device_link(%d, %d)" % (dev_a, dev_b))
    return {"link": "self" if dev_a == dev_b else LINK_TYPES.get(lt.value, "type %d" % lt.value), "hops": hc.value, "peer_access": bool(pa.value)}


def device_count():
    """HIP devices visible to this process (include/m6a.h: m6a_device_count)."""
    return int(_lib.load().m6a_device_count())


def flush_groups(n_sites, batch_size=16, save_per_batch=2):
    """Site offsets of the reference's flush groups (inference_utils.py:33,47)."""
    L = _lib.load()
    nb = (n_sites + batch_size - 1) // batch_size
    g = np.zeros(nb + 2, np.int64)
    G = L.m6a_flush_groups(n_sites, batch_size, save_per_batch, g.ctypes.data, g.size)
    if G < 0:
        raise _lib.M6AError(int(G), "m6a_flush_groups")
    return g[:G + 1].copy()


def reference_written_sites(n_sites, batch_size=16, save_per_batch=2):
    """How many (leading) sites the reference writes for this geometry: its inverted flush test
    (inference_utils.py:47) never writes the batches after the last flush."""
    n = _lib.load().m6a_reference_written_sites(int(n_sites), int(batch_size), int(save_per_batch))
    if n < 0:
        raise _lib.M6AError(int(n), "m6a_reference_written_sites")
    return int(n)


def shard_plan(off, n_shards, batch_size=16, save_per_batch=2):
    """Flush-group-aligned contiguous site shards balanced by read count -> int64 [n_shards+1]."""
    L = _lib.load()
    off = np.ascontiguousarray(off, np.int64)
    out = np.zeros(n_shards + 1, np.int64)
    rc = L.m6a_shard_plan(off.ctypes.data, off.size - 1, batch_size, save_per_batch, n_shards, out.ctypes.data)
    if rc != 0:
        raise _lib.M6AError(rc, "m6a_shard_plan")
    return out
