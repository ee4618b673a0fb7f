#!/usr/bin/env python3
"""`compute_norm_factors --device gpu` against `--device cpu`, end to end, on the bundled data replicated N times (N = 1400: 141 k
sites, 913 MB of data.json -- tools/measure_loader.py's dataset) with a generated data.info.labelled (every site a Train row).  Each
leg is the command in a process of its own; the legs are interleaved (gpu, cpu, gpu, cpu, ...) so that drift of the box falls on
both.  Prints one JSON object: per leg the median, minimum and maximum wall time, the last gpu leg's phases, peak device memory and
device-to-host bytes, and whether the two .npz files hold the same bits.  --parent DIR adds one comparison of `inference --loader
device` between this checkout and another (the parent commit, built): --legs runs each, interleaved, and the bar is the parent's
median plus the parent's own spread.

    python tools/measure_norm_factors.py [N] [--legs K] [--parent DIR] [--out FILE]"""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import measure_io  # noqa: E402


def labelled(d):
    rows = open(os.path.join(d, "data.info")).read().splitlines()[1:]
    with open(os.path.join(d, "data.info.labelled"), "w") as f:
        f.write("transcript_id,transcript_position,start,end,n_reads,modification_status,set_type\n")
        for k, r in enumerate(rows):
            f.write("%s,%d,Train\n" % (r, k % 2))
    return len(rows)


def leg(d, out, device):
    args = [sys.executable, "-m", "m6anet_amd", "compute_norm_factors", "--input_dir", d, "--out_dir", out, "--device", device, "--n_processes", "16"]
    t0 = time.perf_counter()
    r = subprocess.run(args, cwd=REPO, env=dict(os.environ, M6A_NORM_TIMES="1"), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
    wall = time.perf_counter() - t0
    if r.returncode != 0:
        raise SystemExit("leg %s failed: %s" % (device, r.stderr[-2000:]))
    return {"wall_s": wall, "times": json.loads(re.search(r"^M6A_TIMES (.*)$", r.stderr, re.M).group(1))}


def loader_leg(repo, d, out):
    args = [sys.executable, "-m", "m6anet_amd", "inference", "--input_dir", d, "--out_dir", out, "--num_iterations", "1000", "--n_processes", "0",
            "--loader", "device"]
    t0 = time.perf_counter()
    r = subprocess.run(args, cwd=repo, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
    if r.returncode != 0:
        raise SystemExit("inference --loader device failed in %s: %s" % (repo, r.stderr[-2000:]))
    return time.perf_counter() - t0


def summary(w):
    return {"wall_s_median": statistics.median(w), "wall_s_min": min(w), "wall_s_max": max(w), "legs": len(w)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("copies", nargs="?", type=int, default=1400)
    ap.add_argument("--legs", type=int, default=5)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit: `inference --loader device` is compared with it")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as d:
        size = measure_io.replicate(a.copies, d)
        n_sites = labelled(d)
        runs = {"gpu": [], "cpu": []}
        leg(d, os.path.join(d, "warm"), "cpu")                   # page cache, the interpreter's files
        for k in range(a.legs):
            for n in runs:
                runs[n].append(leg(d, os.path.join(d, "out_" + n), n))
        with np.load(os.path.join(d, "out_gpu", "norm_dict_nanopolish.npz")) as g, np.load(os.path.join(d, "out_cpu", "norm_dict_nanopolish.npz")) as c:
            same = all(g[f].tobytes() == c[f].tobytes() for f in ("kmers", "mean", "std"))
        res = {"copies": a.copies, "json_MB": size / 1e6, "n_sites": n_sites, "npz_bits_equal": same, "usable_cpus": len(os.sched_getaffinity(0)),
               **{n: summary([r["wall_s"] for r in runs[n]]) for n in runs}, "gpu_last_leg": runs["gpu"][-1]["times"],
               "cpu_last_leg": runs["cpu"][-1]["times"]}
        if a.parent:
            w = {"here": [], "parent": []}
            loader_leg(REPO, d, os.path.join(d, "warm_loader"))
            for k in range(a.legs):
                w["here"].append(loader_leg(REPO, d, os.path.join(d, "out_here")))
                w["parent"].append(loader_leg(a.parent, d, os.path.join(d, "out_parent")))
            p = summary(w["parent"])
            res["loader_device"] = {"here": summary(w["here"]), "parent": p, "bar_s": p["wall_s_median"] + (p["wall_s_max"] - p["wall_s_min"])}
            res["loader_device"]["within_bar"] = res["loader_device"]["here"]["wall_s_median"] <= res["loader_device"]["bar_s"]
            res["loader_device"]["csv_bytes_equal_parent"] = all(
                open(os.path.join(d, "out_here", f), "rb").read() == open(os.path.join(d, "out_parent", f), "rb").read()
                for f in ("data.site_proba.csv", "data.indiv_proba.csv"))
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
