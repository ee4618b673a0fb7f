"""Builds libm6a_hip.so in-tree with hipcc for gfx950 (cross-compiles without a GPU)."""
import os
import subprocess
import sys

PKG = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(PKG, "csrc")
INCLUDE = os.path.join(os.path.dirname(PKG), "include")
LIB = os.path.join(PKG, "libm6a_hip.so")
IO_LIB = os.path.join(PKG, "libm6a_io.so")
SOURCES = ["m6a_kernels.hip", "m6a_pool_reg.hip", "m6a_pool_rtab.hip", "m6a_expect.hip", "m6a_ranksum.hip", "m6a_ks.hip", "m6a_ks_exact.hip", "m6a_api.hip", "m6a_host_ring.hip", "m6a_job.hip", "m6a_comm.hip",
           "m6a_validate.hip", "m6a_prep.hip", "m6a_train.hip"]
DEPS = SOURCES + [os.path.join(INCLUDE, "m6a_io.h"), "m6a_kernels.h", "m6a_ctx.h", "m6a_prep_kit.h", "m6a_rounds.h", "m6a_host_cpus.h", "m6a_csv.h", "m6a_npy.h", "m6a_npy_write.h", "m6a_repr.h", "m6a_dataprep.h", "m6a_bgzf.h", "m6a_deflate.h", "m6a_json.h", "m6a_norm.h", "m6a_uuid.h", "m6a_ranksum.h", "m6a_ks.h", "m6a_ks_exact.h", "m6a_pairs.h", "m6a_stream.h", "m6a_train_draw.h", os.path.join(INCLUDE, "m6a.h"), os.path.join(PKG, "assets", "mt19937_jump.bin")]


def needs_build():
    if not os.path.exists(LIB):
        return True
    t = os.path.getmtime(LIB)
    return any(os.path.getmtime(os.path.join(CSRC, d)) > t for d in DEPS)


def build(force=False, verbose=False):
    if not force and not needs_build():
        return LIB
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    # -ffp-contract=off: the pooling arithmetic must round where NumPy rounds (a fused 1 - a*b would
    # not); the encoder's FMAs are explicit fmaf()
    jump = os.path.join(PKG, "assets", "mt19937_jump.bin")      # embedded into the library (tools/make_mt_jump.py writes it)
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-fPIC", "-shared",
           '-DM6A_MT_JUMP_PATH="%s"' % jump, "-I" + INCLUDE, "-I" + CSRC] + [os.path.join(CSRC, s) for s in SOURCES] + ["-o", LIB]
    if verbose:
        print(" ".join(cmd), file=sys.stderr)
    subprocess.check_call(cmd)
    return LIB


def build_io(force=False, verbose=False):
    """libm6a_io.so: host-only C++ (loader + CSV writers, include/m6a_io.h)."""
    src = os.path.join(CSRC, "m6a_io.cpp")
    hdr = os.path.join(INCLUDE, "m6a_io.h")
    deps = [src, hdr, os.path.join(CSRC, "m6a_host_cpus.h"), os.path.join(CSRC, "m6a_bgzf.h"), os.path.join(CSRC, "m6a_deflate.h"),
            os.path.join(CSRC, "m6a_json.h"), os.path.join(CSRC, "m6a_norm.h"), os.path.join(CSRC, "m6a_uuid.h"), os.path.join(CSRC, "m6a_repr.h"), os.path.join(CSRC, "m6a_ranksum.h"), os.path.join(CSRC, "m6a_ks.h"), os.path.join(CSRC, "m6a_ks_exact.h")]
    if not force and os.path.exists(IO_LIB) and os.path.getmtime(IO_LIB) >= max(os.path.getmtime(d) for d in deps):
        return IO_LIB
    # -ffp-contract=off: m6a_norm.h's sums round every product on its own, as the kernels' build does
    cmd = [os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-pthread", "-Wall", "-Wextra",
           "-I" + INCLUDE, "-I" + CSRC, src, "-o", IO_LIB]
    if verbose:
        print(" ".join(cmd), file=sys.stderr)
    subprocess.check_call(cmd)
    return IO_LIB


if __name__ == "__main__":
    print(build_io(force="--force" in sys.argv, verbose=True))
    print(build(force="--force" in sys.argv, verbose=True))
