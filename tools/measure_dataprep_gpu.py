#!/usr/bin/env python3
"""`dataprep --device cpu` against `--device gpu` on the reference's bundled eventalign.txt replicated to a target size (distinct
transcript ids per copy, as tools/measure_dataprep.py builds it), page-cache warm.

    python tools/measure_dataprep_gpu.py [GB=23.1] [--out profiles/r07_dataprep_gpu.json] [--timeout 900]

Each path runs in a child process of its own under `timeout` (a GPU step that hangs ends there and nothing more is started);
the files of both must be byte-identical.  Reports wall time and GB/s of each, the GPU path's phases (upload + newline count
through the pinned ring, newline offsets, parse + combine + windows, D2H, host run table, host write) and the achieved H2D rate.

    python tools/measure_dataprep_gpu.py [GB ...] --writer host,device [--legs 5] [--parent DIR] [--out profiles/r17_dataprep_writer.json]

With --writer the shapes default to 24.3 GB and 3 GB, and per shape `--device cpu`, `--device gpu` and `--device gpu --writer device`
run --legs times each, interleaved, every leg the whole command in a process of its own (its wall time is the process's, the
interpreter's start included); the files of the first leg of each are compared with the CPU's once, and every leg's output is
removed behind it.  --parent DIR: a built checkout of the parent commit, whose `--device cpu` and `--device gpu` legs run in between;
the bar on either unchanged command is the parent's median plus the parent's own spread (max - min).  The device-writer leg carries
no bar: it is reported against that session's CPU and GPU-host legs, with its phases, device-to-host bytes and peak device memory."""
import filecmp
import gzip
import json
import os
import shutil
import statistics
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


def device_writer_child(path, out):
    """`--device gpu --writer device`, with its statistics (m6a_dataprep_stats)"""
    from m6anet_amd import _io
    st = {}
    t0 = time.perf_counter()
    _io.dataprep(path, out, n_threads=0, min_segment_count=20, device="gpu", writer="device", stats=st)
    return {"device": "gpu", "writer": st.get("writer"), "s": time.perf_counter() - t0, "stats": st}


def make_file(d, gb):
    text = gzip.open(SRC, "rt").read()
    header, body = text.split("\n", 1)
    n = max(1, int(gb * 1e9 / len(body)))
    path = os.path.join(d, "eventalign.txt")
    with open(path, "w", buffering=16 << 20) as f:
        f.write(header + "\n")
        for k in range(n):
            f.write(body.replace("ENST", "C%dENST" % k) if k else body)
    subprocess.run(["cat", path], stdout=subprocess.DEVNULL, check=True)          # page-cache warm
    return path, n


def run_leg(script, cwd, variant, path, out, limit):
    """One leg: the child of `script` in `cwd`; its RESULT with the process's wall time, or the failure."""
    t0 = time.perf_counter()
    p = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, script, "--child", variant, path, out], capture_output=True, text=True, cwd=cwd)
    wall = time.perf_counter() - t0
    if p.returncode != 0:
        return {"rc": p.returncode, "stderr_tail": p.stderr[-2000:]}
    r = json.loads(p.stdout.split("RESULT ", 1)[1])
    r["process_s"] = wall
    return r


def summary(legs):
    s = [l["process_s"] for l in legs]
    return {"process_s": s, "median_s": statistics.median(s), "spread_s": max(s) - min(s), "inner_s": [l["s"] for l in legs]}


def writer_main(shapes, n_legs, parent, dest, limit):
    """five interleaved legs of the three commands (and the parent's two) per shape"""
    here = os.path.abspath(__file__)
    commands = [("cpu", here, REPO, "cpu"), ("gpu_host_writer", here, REPO, "gpu"), ("gpu_device_writer", here, REPO, "gpu_device")]
    if parent:
        parent = os.path.abspath(parent)
        commands += [("parent_cpu", os.path.join(parent, "tools", "measure_dataprep_gpu.py"), parent, "cpu"),
                     ("parent_gpu_host_writer", os.path.join(parent, "tools", "measure_dataprep_gpu.py"), parent, "gpu")]
    res = {"legs": n_legs, "shapes": []}
    for gb in shapes:
        with tempfile.TemporaryDirectory(dir=os.environ.get("M6A_MEASURE_TMP")) as d:
            path, n = make_file(d, gb)
            size = os.path.getsize(path)
            shape = {"copies": n, "eventalign_GB": size / 1e9, "files_identical": {}}
            legs = {name: [] for name, _, _, _ in commands}
            failed = False
            for leg in range(n_legs):
                for name, script, cwd, variant in commands:
                    out = os.path.join(d, name)
                    r = run_leg(script, cwd, variant, path, out, limit)
                    if "rc" in r:                                  # a step that failed or hung ends the measurement: nothing more is started
                        shape[name + "_failed"] = r
                        failed = True
                        break
                    legs[name].append(r)
                    if leg == 0:
                        if name == "cpu":
                            os.rename(out, os.path.join(d, "cpu_kept"))
                        else:
                            shape["files_identical"][name] = all(filecmp.cmp(os.path.join(d, "cpu_kept", f), os.path.join(out, f), shallow=False)
                                                                 for f in FILES)
                    shutil.rmtree(out, ignore_errors=True)
                if failed:
                    break
            for name, ls in legs.items():
                if ls:
                    shape[name] = summary(ls)
                    shape[name]["GB_per_s"] = size / 1e9 / shape[name]["median_s"]
            if legs["gpu_host_writer"]:
                shape["gpu_host_writer"]["last_leg"] = legs["gpu_host_writer"][-1]
            if legs["gpu_device_writer"]:
                mid = sorted(legs["gpu_device_writer"], key=lambda l: l["process_s"])[len(legs["gpu_device_writer"]) // 2]
                shape["gpu_device_writer"]["median_leg"] = mid
                shape["gpu_device_writer"]["writers"] = [l.get("writer") for l in legs["gpu_device_writer"]]
                for other in ("cpu", "gpu_host_writer"):
                    if legs[other]:
                        shape["device_writer_speed_over_" + other] = shape[other]["median_s"] / shape["gpu_device_writer"]["median_s"]
            for name in ("cpu", "gpu_host_writer"):               # the unchanged commands against the parent's, same session
                if parent and legs[name] and legs["parent_" + name]:
                    bar = shape["parent_" + name]["median_s"] + shape["parent_" + name]["spread_s"]
                    shape[name]["bar_s"] = bar
                    shape[name]["within_bar"] = shape[name]["median_s"] <= bar
            res["shapes"].append(shape)
            if failed:
                break
    print(json.dumps(res, indent=1))
    os.makedirs(os.path.dirname(dest), exist_ok=True)
    with open(dest, "w") as f:
        json.dump(res, f, indent=1)


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        dev, path, out = sys.argv[2:5]
        r = {"gpu": gpu_child, "gpu_device": device_writer_child, "cpu": cpu_child}[dev](path, out)
        print("RESULT " + json.dumps(r))
        return
    def opt(name, default=None):
        return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default
    flags = ("--out", "--timeout", "--writer", "--legs", "--parent")
    args = [a for i, a in enumerate(sys.argv[1:], 1) if not a.startswith("--") and sys.argv[i - 1] not in flags]
    if "--writer" in sys.argv:
        if sorted(opt("--writer").split(",")) != ["device", "host"]:
            sys.exit("--writer takes host,device")
        return writer_main([float(a) for a in args] or [24.3, 3.0], int(opt("--legs", 5)), opt("--parent"),
                           opt("--out", os.path.join(REPO, "profiles", "r17_dataprep_writer.json")), int(opt("--timeout", 900)))
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
