#!/usr/bin/env python3
"""`dataprep --device cpu` against `--device gpu` on the reference's bundled eventalign.txt replicated to a target size (distinct
transcript ids per copy, as tools/measure_dataprep.py builds it), page-cache warm.

    python tools/measure_dataprep_gpu.py [GB=23.1] [--out profiles/r07_dataprep_gpu.json] [--timeout 900]

Each path runs in a child process of its own under `timeout` (a GPU step that hangs ends there and nothing more is started);
the files of both must be byte-identical.  Reports wall time and GB/s of each, the GPU path's phases (upload + newline count
through the pinned ring, newline offsets, parse + combine + windows, D2H, host run table, host write) and the achieved H2D rate."""
import filecmp
import gzip
import json
import os
import subprocess
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
SRC = os.path.join(REPO, "tests", "golden", "ref_tests_data", "eventalign.txt.gz")
FILES = ("eventalign.index", "data.json", "data.info", "data.log")


def cpu_child(path, out):
    from m6anet_amd import _io
    t0 = time.perf_counter()
    _io.dataprep(path, out, n_threads=0, min_segment_count=20)
    return {"device": "cpu", "s": time.perf_counter() - t0}


def gpu_child(path, out):
    """the GPU path with its phases (m6a_prep_times)"""
    import ctypes as C
    from m6anet_amd import _io, _lib
    t0 = time.perf_counter()
    p = _io.prep_on_device(path, 1)
    prep_s = time.perf_counter() - t0
    ms = (C.c_double * 6)()
    _lib.load().m6a_prep_times(p._h, ms)
    t1 = time.perf_counter()
    _io.write_table(path, out, p.table, n_threads=0, min_segment_count=20)
    write_s = time.perf_counter() - t1
    import numpy as np
    t = p.table.contents
    n_runs, n_rows = t.n_runs, t.n_rows
    declined = int(np.count_nonzero(np.ctypeslib.as_array(C.cast(t.run_status, C.POINTER(C.c_int32)), shape=(n_runs,)))) if n_runs else 0
    p.__exit__(None, None, None)
    return {"device": "gpu", "s": time.perf_counter() - t0, "prep_s": prep_s, "host_write_s": write_s, "runs": n_runs, "rows": n_rows,
            "phases_ms": {"upload_and_newline_count": ms[0], "newline_offsets": ms[1], "parse_combine_windows": ms[2], "d2h": ms[3],
                          "host_run_table": ms[4]}, "h2d_GB_per_s_through_ring": ms[5], "declined_runs": declined}


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        dev, path, out = sys.argv[2:5]
        r = gpu_child(path, out) if dev == "gpu" else cpu_child(path, out)
        print("RESULT " + json.dumps(r))
        return
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    gb = float(args[0]) if args else 23.1
    dest = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(REPO, "profiles", "r07_dataprep_gpu.json")
    limit = int(sys.argv[sys.argv.index("--timeout") + 1]) if "--timeout" in sys.argv else 900
    text = gzip.open(SRC, "rt").read()
    header, body = text.split("\n", 1)
    n = max(1, int(gb * 1e9 / len(body)))
    with tempfile.TemporaryDirectory(dir=os.environ.get("M6A_MEASURE_TMP")) as d:
        path = os.path.join(d, "eventalign.txt")
        with open(path, "w", buffering=16 << 20) as f:
            f.write(header + "\n")
            for k in range(n):
                f.write(body.replace("ENST", "C%dENST" % k) if k else body)
        size = os.path.getsize(path)
        subprocess.run(["cat", path], stdout=subprocess.DEVNULL, check=True)          # page-cache warm
        res = {"copies": n, "eventalign_GB": size / 1e9}
        for dev in ("cpu", "gpu"):
            out = os.path.join(d, dev)
            p = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--child", dev, path, out],
                               capture_output=True, text=True, cwd=REPO)
            if p.returncode != 0:
                res[dev] = {"rc": p.returncode, "stderr_tail": p.stderr[-2000:]}
                break
            r = json.loads(p.stdout.split("RESULT ", 1)[1])
            r["GB_per_s"] = size / 1e9 / r["s"]
            res[dev] = r
        if "s" in res.get("gpu", {}) and "s" in res.get("cpu", {}):
            res["files_identical"] = all(filecmp.cmp(os.path.join(d, "cpu", f), os.path.join(d, "gpu", f), shallow=False) for f in FILES)
            res["gpu_over_cpu_speed"] = res["cpu"]["s"] / res["gpu"]["s"]
    print(json.dumps(res, indent=1))
    os.makedirs(os.path.dirname(dest), exist_ok=True)
    with open(dest, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
