"""The pointer convention of include/m6a.h ("all host or all device"), entry point by entry point: one table, one driver.

A Row names an entry point of libm6a_hip.so, the arrays of a smallest correct call and how the call is made from their addresses.
tests/test_gpu_pointer_convention.py walks the table: the host-pointer and the device-pointer call give the same bits, and every
refusal the host decides before anything is queued -- a required pointer NULL, one pointer on the other side from the rest,
off[0] = 1, one decreasing step in a host off[] -- returns M6A_EINVAL with the library's own sentence, consumes the one-shot offsets
hint where the entry point has a hint scope, and leaves the context fit for the same correct call.  tools/pointer_convention_calls.py
makes the same correct calls once each under a tracer.

The shapes: six sites with bags of 1, 2, 15, 16, 17 and 40 reads (both sides of the encoder's 16-read choice in one call, and a bag
of one read); the trainer's rows at 4 bags of 20 reads.  No case lets a kernel read outside an array: every bad call is refused on
the host, and the wrong hint that is armed before one has the right range and total (only its histogram differs).

Run as a program -- `pointer_convention.py gather` with M6A_RCCL_LIB naming tests/stub_rccl's library -- it checks the two gather
rows in a process of its own: the library binds RCCL once per process, and the test process may have bound the real one already.
"""
import ctypes as C
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from m6anet_amd import _lib, synthetic                                            # noqa: E402
from m6anet_amd.constants import DEFAULT_READ_THRESHOLD, asset_path               # noqa: E402

BAGS = [1, 2, 15, 16, 17, 40]
S = len(BAGS)
T, K = 5, 20                  # sampled pooling
VT, VK = 3, 1                 # validation draws without replacement: n_samples cannot exceed the bag of one read
B, BAG = 4, 20                # the trainer's batch
THR = float(np.float32(DEFAULT_READ_THRESHOLD))
EINVAL = -1

NULL = "null pointer argument"
OFF0 = "off[0] must be 0"
DECREASING = "off[] must be non-decreasing"

_d = synthetic.make_sites(S, n_reads=BAGS, seed=30)
X, KM, OFF = _d["X"], _d["site_kmers"], _d["off"]
R = int(OFF[-1])
RP = (np.random.Generator(np.random.PCG64(30)).random(R, dtype=np.float32) ** 4).astype(np.float32)
WRONG_HINT = np.concatenate([[0], np.cumsum([1, 3, 14, 16, 17, 40])]).astype(np.int64)   # range 1..40 and 91 reads, another histogram
_b = synthetic.make_sites(B, BAG, seed=31)
XB, KB = _b["X"], _b["site_kmers"]
YB = np.array([0, 1, 0, 1], np.float32)
OFFB = _b["off"]
ORDER = np.arange(B, dtype=np.int64)
N_WEIGHTS = 7997


def f32(n): return np.zeros(n, np.float32)
def f64(n): return np.zeros(n, np.float64)


class Row:
    """name: the entry point.  ptrs: {argument: array}, inputs as they are, outputs zero-filled.  outs: the arguments compared.
    optional: may be NULL.  host_only: never a device pointer.  sentence: the side check's refusal.  off: the host CSR argument the
    entry point checks, or None.  hint: a refused call consumes the offsets hint.  null_text / flip_text: refusals with a sentence of
    their own.  run(env, A): the call from the addresses A -> return code (env.arm() goes right before the entry point itself)."""

    def __init__(self, name, ptrs, outs, run, sentence=None, optional=(), host_only=(), off=None, hint=True, null_text=None, flip_text=None):
        self.name, self.ptrs, self.outs, self.run, self.sentence = name, ptrs, outs, run, sentence
        self.optional, self.host_only, self.off, self.hint = optional, host_only, off, hint
        self.null_text, self.flip_text = null_text or {}, flip_text or {}

    def sided(self):
        return [n for n in self.ptrs if n not in self.host_only]


class Env:
    """One engine (and what a row needs besides: weights for a trainer, torch for the device side)."""

    def __init__(self):
        import torch
        self.torch = torch
        self.L = _lib.load()
        self.w = np.fromfile(asset_path("weights_hct116.bin"), np.float32)
        self.h = C.c_void_p()
        assert self.L.m6a_create(C.byref(self.h), self.w.ctypes.data, self.w.size, 0) == 0
        self.arm = lambda: None
        self.extra = b""

    def close(self):
        self.L.m6a_destroy(self.h)

    def error(self):
        return self.L.m6a_last_error(self.h).decode()

    def buffers(self, row, side):
        """{argument: array or tensor} of a correct call on `side` ("host" | "device"), outputs zeroed."""
        out = {}
        for n, a in row.ptrs.items():
            a = np.zeros_like(a) if n in row.outs else a.copy()
            out[n] = self.torch.from_numpy(a).to("cuda:0") if side == "device" and n not in row.host_only else a
        self.torch.cuda.synchronize()
        return out

    @staticmethod
    def address(b):
        return b.ctypes.data if isinstance(b, np.ndarray) else b.data_ptr()

    def call(self, row, side, change=None):
        """One call of the row on `side`; change(A, bufs) edits the addresses first.  -> (return code, bits of the outputs)."""
        bufs = self.buffers(row, side)
        A = {n: self.address(b) for n, b in bufs.items()}
        keep = change(A) if change else None                     # whatever the edited addresses point at stays alive
        self.extra = b""
        rc = row.run(self, A)
        if rc:
            return rc, None
        rc = self.L.m6a_sync(self.h)
        if rc:
            return rc, None
        bits = tuple(bufs[n].tobytes() if isinstance(bufs[n], np.ndarray) else bufs[n].cpu().numpy().tobytes() for n in row.outs)
        del keep
        return 0, bits + (self.extra,)

    # ---- what the trainer's rows share ----
    def trainer(self):
        t = C.c_void_p()
        assert self.L.m6a_train_create(self.h, self.w.ctypes.data, self.w.size, None, C.byref(t)) == 0, self.error()
        return t

    def weights_of(self, t):
        out = f32(N_WEIGHTS)
        assert self.L.m6a_train_weights(t, out.ctypes.data, None) == 0, self.error()
        return out.tobytes()


def ticket_ptr(addr):
    return C.cast(addr, C.POINTER(C.c_int64)) if addr else None


# ---- the calls ----------------------------------------------------------------------------------------------------------------
def run_encode(e, A):
    e.arm()
    return e.L.m6a_encode_reads(e.h, A["X"], A["km"], A["off"], S, A["rp"])


def run_repr(e, A):
    e.arm()
    return e.L.m6a_read_representation_dtype(e.h, A["X"], A["km"], A["off"], S, A["repr"], _lib.REPR_DTYPES["float32"], A["rp"])


def run_site_pool(e, A):
    e.arm()
    return e.L.m6a_site_pool(e.h, A["rp"], A["off"], S, T, K, THR, 0, _lib.RNG_NUMPY, 16, 2, A["site"], A["mod"])


def run_expectation(e, A):
    e.arm()
    return e.L.m6a_site_expectation(e.h, A["rp"], A["off"], S, K, THR, A["site"], A["mod"], A["sigma"])


def run_infer(e, A):
    e.arm()
    return e.L.m6a_infer(e.h, A["X"], A["km"], A["off"], S, T, K, THR, 0, _lib.RNG_NUMPY, 16, 2, A["rp"], A["site"], A["mod"])


def run_bag_forward(e, A):
    e.arm()
    return e.L.m6a_bag_forward(e.h, A["X"], A["km"], B, BAG, A["site"])


def run_random_stream(e, A):
    return e.L.m6a_random_stream(e.h, 7, 1000, A["words"])


def run_validate(e, A):
    e.arm()
    return e.L.m6a_validate(e.h, A["X"], A["km"], A["off"], S, VT, VK, 3, A["rp"], A["y"], A["avg"])


def run_validate_pool(e, A):
    e.arm()
    return e.L.m6a_validate_pool(e.h, A["rp"], A["off"], S, VT, VK, 3, A["y"], A["avg"])


def job_begin(e):
    assert e.L.m6a_job_begin(e.h, T, K, THR, 0, _lib.RNG_NUMPY, 16, 2, 0, 0) == 0, e.error()


def run_job_feed(e, A):
    """begin, the feed under test, end into host arrays (a refused feed's job is aborted)"""
    job_begin(e)
    rc = e.L.m6a_job_feed(e.h, A["X"], A["km"], A["off"], S)
    if rc:
        text = e.error()
        assert e.L.m6a_job_abort(e.h) == 0
        assert e.error() == text                                 # the abort leaves the refusal's text
        return rc
    rp, site, mod = f32(R), f32(S), f64(S)
    assert e.L.m6a_job_end(e.h, rp.ctypes.data, site.ctypes.data, mod.ctypes.data) == 0, e.error()
    e.extra = rp.tobytes() + site.tobytes() + mod.tobytes()
    return 0


def run_job_end(e, A):
    """begin, one host feed, the end under test (which closes the job whatever it returns)"""
    job_begin(e)
    assert e.L.m6a_job_feed(e.h, X.ctypes.data, KM.ctypes.data, OFF.ctypes.data, S) == 0, e.error()
    e.arm()
    return e.L.m6a_job_end(e.h, A["rp"], A["site"], A["mod"])


def run_gather(e, A):
    return e.L.m6a_gather(e.h, A["site"], A["mod"], A["cuts"], 0, A["site_all"], A["mod_all"])


def run_gather_reads(e, A):
    return e.L.m6a_gather_reads(e.h, A["rp"], A["cuts"], 0, A["rp_all"])


def with_trainer(body):
    """a fresh trainer per call: a step changes its weights, and the same call must give the same bits again"""
    def run(e, A):
        t = e.trainer()
        try:
            return body(e, t, A)
        finally:
            e.L.m6a_train_destroy(t)
    return run


def host_step(e, t):
    assert e.L.m6a_train_step(t, XB.ctypes.data, KB.ctypes.data, YB.ctypes.data, B, BAG, None, None) == 0, e.error()


def body_step(e, t, A):
    rc = e.L.m6a_train_step(t, A["X"], A["km"], A["y"], B, BAG, A["loss"], A["y_pred"])
    e.extra = e.weights_of(t)                                   # a refused step changes nothing either
    return rc


def body_epoch(e, t, A):
    rc = e.L.m6a_train_epoch(t, A["X"], A["km"], A["off"], A["y"], B, A["order"], B, B, BAG, 5, A["loss"], A["y_pred"])
    e.extra = e.weights_of(t)
    return rc


def body_forward(e, t, A):
    return e.L.m6a_train_forward(t, A["X"], A["km"], B, BAG, 1, A["s"], ticket_ptr(A["ticket"]))


def body_backward(e, t, A):
    s, ticket = f32(B), np.zeros(1, np.int64)
    assert e.L.m6a_train_forward(t, XB.ctypes.data, KB.ctypes.data, B, BAG, 1, s.ctypes.data, ticket_ptr(ticket.ctypes.data)) == 0, e.error()
    return e.L.m6a_train_backward(t, int(ticket[0]), A["grad_s"], A["grads"])


def body_set_weights(e, t, A):
    rc = e.L.m6a_train_set_weights(t, A["blob"])
    e.extra = e.weights_of(t)
    return rc


def body_running_stats(e, t, A):
    host_step(e, t)
    return e.L.m6a_train_running_stats(t, A["stats"])


ENC = {"X": X, "km": KM, "off": OFF}
BLOB = np.fromfile(asset_path("weights_arabidopsis.bin"), np.float32)

TABLE = [
    Row("m6a_encode_reads", dict(ENC, rp=f32(R)), ["rp"], run_encode, off="off",
        sentence="X, site_kmers, off, read_prob must be all host or all device pointers"),
    Row("m6a_read_representation_dtype", dict(ENC, repr=f32(R * 32), rp=f32(R)), ["repr", "rp"], run_repr, off="off", optional=("rp",),
        sentence="X, site_kmers, off, repr, read_prob must be all host or all device pointers",
        null_text={"repr": "repr is NULL: m6a_encode_reads is the call without the representation"}),
    Row("m6a_site_pool", {"rp": RP, "off": OFF, "site": f32(S), "mod": f64(S)}, ["site", "mod"], run_site_pool, off="off",
        sentence="read_prob, off, site_prob, mod_ratio must be all host or all device pointers"),
    Row("m6a_site_expectation", {"rp": RP, "off": OFF, "site": f32(S), "mod": f64(S), "sigma": f64(S)}, ["site", "mod", "sigma"],
        run_expectation, off="off", optional=("sigma",),
        sentence="read_prob, off, site_prob, mod_ratio, mc_sigma must be all host or all device pointers"),
    Row("m6a_infer", dict(ENC, rp=f32(R), site=f32(S), mod=f64(S)), ["rp", "site", "mod"], run_infer, off="off", optional=("rp",),
        sentence="all data pointers must be host pointers or all device pointers"),
    Row("m6a_bag_forward", {"X": XB, "km": KB, "site": f32(B)}, ["site"], run_bag_forward,
        sentence="X, site_kmers, site_prob must be all host or all device pointers"),
    Row("m6a_random_stream", {"words": np.zeros(1000, np.uint32)}, ["words"], run_random_stream, hint=False),
    Row("m6a_validate", dict(ENC, rp=f32(R), y=f32(VT * S), avg=f32(S)), ["rp", "y", "avg"], run_validate, off="off", optional=("rp", "avg"),
        sentence="X, site_kmers, off and the outputs must be all host or all device pointers"),
    Row("m6a_validate_pool", {"rp": RP, "off": OFF, "y": f32(VT * S), "avg": f32(S)}, ["y", "avg"], run_validate_pool, off="off",
        optional=("avg",), sentence="read_prob, off, y_pred, y_pred_avg must be all host or all device pointers"),
    Row("m6a_job_feed", dict(ENC), [], run_job_feed, off="off", host_only=("off",), hint=False,
        sentence="X and site_kmers must be both host or both device pointers"),
    Row("m6a_job_end", {"rp": f32(R), "site": f32(S), "mod": f64(S)}, ["rp", "site", "mod"], run_job_end, optional=("rp",),
        sentence="read_prob, site_prob, mod_ratio must be all host or all device pointers"),
    Row("m6a_train_step", {"X": XB, "km": KB, "y": YB, "loss": f32(1), "y_pred": f32(B)}, ["loss", "y_pred"], with_trainer(body_step),
        optional=("loss", "y_pred"), hint=False, sentence="X, site_kmers, y, loss, y_pred must be all host or all device pointers"),
    Row("m6a_train_epoch", {"X": XB, "km": KB, "off": OFFB, "y": YB, "order": ORDER, "loss": f32(1), "y_pred": f32(B)}, ["loss", "y_pred"],
        with_trainer(body_epoch), off="off", optional=("loss", "y_pred"), hint=False,
        sentence="X, site_kmers, off, y, order, loss, y_pred must be all host or all device pointers"),
    Row("m6a_train_forward", {"X": XB, "km": KB, "s": f32(B), "ticket": np.zeros(1, np.int64)}, ["s"], with_trainer(body_forward),
        host_only=("ticket",), hint=False, sentence="X, site_kmers, s must be all host or all device pointers"),
    Row("m6a_train_backward", {"grad_s": np.linspace(-1, 1, B).astype(np.float32), "grads": f32(N_WEIGHTS)}, ["grads"],
        with_trainer(body_backward), hint=False, sentence="grad_s, grads must be all host or all device pointers"),
    Row("m6a_train_set_weights", {"blob": BLOB}, [], with_trainer(body_set_weights), hint=False),
    Row("m6a_train_running_stats", {"stats": f32(300)}, ["stats"], with_trainer(body_running_stats), hint=False),
]

# the exchange, one rank that is its own destination (needs a communicator: see main)
GATHER = [
    Row("m6a_gather", {"site": RP[:S].copy(), "mod": np.arange(S) * 0.5, "cuts": np.array([0, S], np.int64), "site_all": f32(S), "mod_all": f64(S)},
        ["site_all", "mod_all"], run_gather, host_only=("cuts",), hint=False,
        sentence="site_prob, mod_ratio, site_all, mod_all must be all host or all device pointers",
        null_text={"cuts": "bad gather arguments", "site_all": "rank dst needs site_all and mod_all", "mod_all": "rank dst needs site_all and mod_all"}),
    Row("m6a_gather_reads", {"rp": RP, "cuts": np.array([0, R], np.int64), "rp_all": f32(R)}, ["rp_all"], run_gather_reads, host_only=("cuts",),
        hint=False, sentence="read_prob and read_all must be both host or both device pointers",
        null_text={"cuts": "bad gather arguments", "rp_all": "rank dst needs read_all"}),
]
HOST_ARRAY_TEXT = {"m6a_job_feed": "m6a_job_feed takes off[] as a HOST pointer", "m6a_gather": "shard offsets are a HOST array",
                   "m6a_gather_reads": "shard offsets are a HOST array"}


# ---- the checks ---------------------------------------------------------------------------------------------------------------
def refusals(env, row):
    """[(what, side of the call, change(A), the sentence)] -- every refusal of the row that the host decides before it queues anything"""
    out = []
    for n in row.ptrs:
        if n not in row.optional:
            out.append(("%s = NULL" % n, "host", lambda A, n=n: A.__setitem__(n, None), row.null_text.get(n, NULL)))
    sided = row.sided()
    for side, other in (("host", "device"), ("device", "host")):
        if len(sided) < 2:
            break
        for n in sided:
            def flip(A, n=n, other=other):
                b = env.buffers(row, other)[n]
                A[n] = env.address(b)
                return b
            out.append(("%s on the %s, the rest on the %s" % (n, other, side), side, flip, row.sentence))
    if row.name in HOST_ARRAY_TEXT:
        n = row.host_only[0]

        def to_device(A, n=n):
            t = env.torch.from_numpy(row.ptrs[n].copy()).to("cuda:0")
            A[n] = t.data_ptr()
            return t
        out.append(("%s on the device" % n, "host", to_device, HOST_ARRAY_TEXT[row.name]))
    if row.off:
        good = row.ptrs[row.off]
        for what, text, edit in (("off[0] = 1", OFF0, lambda o: o.__setitem__(0, 1)), ("off[2] < off[1]", DECREASING, lambda o: o.__setitem__(2, 0))):
            def bad_off(A, edit=edit):
                o = good.copy()
                edit(o)
                A[row.off] = o.ctypes.data
                return o
            out.append((what, "host", bad_off, text))
    return out


def check_row(env, row, say=None):
    """The whole of the row's contract; raises AssertionError with the row and the case in its message."""
    rc, want = env.call(row, "host")
    assert rc == 0, (row.name, "host pointers", rc, env.error())
    rc, got = env.call(row, "device")
    assert rc == 0, (row.name, "device pointers", rc, env.error())
    assert got == want, (row.name, "device pointers give other bits than host pointers")
    probe = TABLE[0]
    for what, side, change, text in refusals(env, row):
        if row.hint:
            env.arm = lambda: env.L.m6a_set_host_offsets(env.h, WRONG_HINT.ctypes.data)
        try:
            rc, _ = env.call(row, side, change)
        finally:
            env.arm = lambda: None
        if say:
            say("%-32s %-44s -> %d %s" % (row.name, what, rc, env.error()))
        assert rc == EINVAL and env.error() == text, (row.name, what, rc, env.error())
        if row.hint:
            # a hint that stayed armed would describe this device call: the next sync reports the histogram that differs
            rc, bits = env.call(probe, "device")
            assert rc == 0 and bits == PROBE_BITS[0], (row.name, what, "the offsets hint outlived the refused call", env.error())
        rc, again = env.call(row, "host")
        assert rc == 0 and again == want, (row.name, what, "the correct call after the refusal", rc, env.error())


PROBE_BITS = [None]


def prepare(env):
    rc, PROBE_BITS[0] = env.call(TABLE[0], "device")
    assert rc == 0, env.error()


def main():
    assert sys.argv[1:] == ["gather"] and os.environ.get("M6A_RCCL_LIB")
    env = Env()
    ident = C.create_string_buffer(128)
    assert env.L.m6a_comm_unique_id(ident) == 0
    assert env.L.m6a_comm_init(env.h, ident, 0, 1) == 0, env.error()
    version = C.c_int(0)
    assert env.L.m6a_comm_info(env.h, None, None, C.byref(version)) == 0 and version.value == 99999      # the stand-in, not an RCCL
    for row in GATHER:
        check_row(env, row, say=print if os.environ.get("POINTER_CONVENTION_VERBOSE") else None)
    assert env.L.m6a_comm_destroy(env.h) == 0
    env.close()
    print("gather rows ok")


if __name__ == "__main__":
    main()
