#!/usr/bin/env python3
"""Every call of tests/pointer_convention.py's table once with host pointers and once with device pointers on ONE fresh engine -- the
work a build queues for them, to be read off a trace -- and the comparison of two such traces.

    rocprofv3 --hip-trace --kernel-trace --memory-copy-trace -f csv json -d DIR -o NAME -- python tools/pointer_convention_calls.py
        M6A_HIP_LIB selects the build; M6A_RCCL_LIB must name tests/stub_rccl's library (the gather rows run on it, one rank).
    python tools/pointer_convention_calls.py --compare DIR_A/NAME DIR_B/NAME [--labels parent this] > profiles/<...>_trace.txt
        Per stream, the kernels (name, grid, workgroup) and the copies (direction, bytes) must be equal entry for entry, streams
        numbered in order of first use.  Per thread, the numbers of hipStreamSynchronize, hipMalloc and hipFree must be equal, threads
        in order of first appearance.  Exit status 1 if anything differs.
"""
import collections
import csv
import ctypes as C
import glob
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))
COUNTED = ("hipStreamSynchronize", "hipMalloc", "hipFree")


def make_calls():
    import pointer_convention as PC
    assert os.environ.get("M6A_RCCL_LIB"), "M6A_RCCL_LIB must name the stand-in transport (tests/stub_rccl)"
    env = PC.Env()
    ident = C.create_string_buffer(128)
    assert env.L.m6a_comm_unique_id(ident) == 0 and env.L.m6a_comm_init(env.h, ident, 0, 1) == 0, env.error()
    for row in PC.TABLE + PC.GATHER:
        bits = []
        for side in ("host", "device"):
            rc, b = env.call(row, side)
            assert rc == 0, (row.name, side, rc, env.error())
            bits.append(b)
        assert bits[0] == bits[1], row.name
        print("%-32s host and device: same bits" % row.name)
    assert env.L.m6a_comm_destroy(env.h) == 0
    env.close()


def read(prefix, what):
    files = glob.glob(prefix + "_" + what + ".csv") + glob.glob(os.path.join(os.path.dirname(prefix), "**", os.path.basename(prefix) + "_" + what + ".csv"), recursive=True)
    assert files, "no %s trace under %s" % (what, prefix)
    with open(sorted(set(files))[0], newline="") as f:
        return list(csv.DictReader(f))


def col(row, *names):
    for n in names:
        if n in row:
            return row[n]
    raise KeyError("none of %r among %r" % (names, sorted(row)))


def copy_bytes(prefix):
    """{correlation id: bytes} of the copies: the CSV has no size column, the JSON output (-f csv json) has"""
    files = glob.glob(prefix + "_results.json") + glob.glob(os.path.join(os.path.dirname(prefix), "**", os.path.basename(prefix) + "_results.json"), recursive=True)
    assert files, "no JSON output next to the CSV files: run the tracer with -f csv json"
    with open(sorted(set(files))[0]) as f:
        runs = json.load(f)["rocprofiler-sdk-tool"]
    return {int(r["correlation_id"]["internal"]): int(r["bytes"]) for run in runs for r in run["buffer_records"]["memory_copy"]}


def per_stream(prefix):
    """{stream rank: [entries in start order]}: kernels and copies together, as the stream ran them"""
    ev = []
    for r in read(prefix, "kernel_trace"):
        ev.append((int(col(r, "Start_Timestamp")), col(r, "Stream_Id"),
                   "kernel %s grid %s,%s,%s wg %s,%s,%s" % (col(r, "Kernel_Name"), col(r, "Grid_Size_X"), col(r, "Grid_Size_Y"), col(r, "Grid_Size_Z"),
                                                            col(r, "Workgroup_Size_X"), col(r, "Workgroup_Size_Y"), col(r, "Workgroup_Size_Z"))))
    nbytes = copy_bytes(prefix)
    for r in read(prefix, "memory_copy_trace"):
        ev.append((int(col(r, "Start_Timestamp")), col(r, "Stream_Id"), "copy %s %s bytes" % (col(r, "Direction"), nbytes[int(col(r, "Correlation_Id"))])))
    ev.sort()
    rank, out = {}, collections.OrderedDict()
    for _, stream, what in ev:
        out.setdefault(rank.setdefault(stream, len(rank)), []).append(what)
    return out


def per_thread(prefix):
    """[{function: count} per thread, threads in order of first appearance]"""
    rows = sorted(read(prefix, "hip_api_trace"), key=lambda r: int(col(r, "Start_Timestamp")))
    rank, out = {}, []
    for r in rows:
        t = rank.setdefault(col(r, "Thread_Id"), len(rank))
        if t == len(out):
            out.append(collections.Counter())
        out[t][col(r, "Function")] += 1
    return out


def compare(a, b, labels):
    sa, sb, ta, tb = per_stream(a), per_stream(b), per_thread(a), per_thread(b)
    bad = 0
    lines = ["== kernels and copies per stream (streams in order of first use) =="]
    for s in sorted(set(sa) | set(sb)):
        x, y = sa.get(s, []), sb.get(s, [])
        same = x == y
        bad += not same
        n_k = sum(e.startswith("kernel") for e in x)
        lines.append("-- stream %d: %s: %d kernels and %d copies on %s, %d entries on %s" % (s, "IDENTICAL entry for entry" if same else "DIFFERENT", n_k, len(x) - n_k,
                                                                                            labels[0], len(y), labels[1]))
        if not same:
            for i, (p, q) in enumerate(zip(x, y)):
                if p != q:
                    lines += ["   first difference at entry %d:" % i, "     %s: %s" % (labels[0], p), "     %s: %s" % (labels[1], q)]
                    break
        else:
            names = collections.Counter(e.split(" grid ")[0] if e.startswith("kernel") else e.rsplit(" ", 2)[0] for e in x)
            lines += ["     %6d x %s" % (n, k[:150]) for k, n in sorted(names.items(), key=lambda kv: -kv[1])]
    lines.append("== %s per thread (threads in order of first appearance) ==" % ", ".join(COUNTED))
    for t in range(max(len(ta), len(tb))):
        x = ta[t] if t < len(ta) else {}
        y = tb[t] if t < len(tb) else {}
        cx, cy = [x.get(f, 0) for f in COUNTED], [y.get(f, 0) for f in COUNTED]
        bad += cx != cy
        lines.append("-- thread %d: %s: %s %s, %s %s" % (t, "EQUAL" if cx == cy else "DIFFERENT", labels[0], cx, labels[1], cy))
    print("RESULT: %s" % ("everything compared is identical" if not bad else "%d difference(s)" % bad))
    print("\n".join(lines))
    return 1 if bad else 0


if __name__ == "__main__":
    if "--compare" in sys.argv:
        i = sys.argv.index("--compare")
        labels = sys.argv[sys.argv.index("--labels") + 1:][:2] if "--labels" in sys.argv else ["first", "second"]
        sys.exit(compare(sys.argv[i + 1], sys.argv[i + 2], labels))
    make_calls()
