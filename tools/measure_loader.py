#!/usr/bin/env python3
"""`inference --loader host` against `--loader device`, end to end, on the bundled data replicated N times (N = 1400: 141 k sites,
913 MB of data.json -- tools/measure_cli.py's dataset).  Each leg is the command in a process of its own; the legs are interleaved
(host, device, host, device, ...) so that drift of the box falls on both.  Prints one JSON object: per leg the median, minimum and
maximum wall time and the load phase (host: the loader's own trace, M6A_IO_TRACE; device: m6a_json_sites_build's `total`), and
whether the two CSV files came out byte-identical.  --parent DIR adds a third leg, the default command run from another checkout
(the parent commit, built), for the default command's own before / after.

    python tools/measure_loader.py [N] [--legs K] [--parent DIR] [--out FILE]"""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import measure_io  # noqa: E402

CSVS = ("data.site_proba.csv", "data.indiv_proba.csv")


def leg(repo, d, out, loader):
    args = [sys.executable, "-m", "m6anet_amd", "inference", "--input_dir", d, "--out_dir", out, "--num_iterations", "1000", "--n_processes", "0"]
    if loader is not None:
        args += ["--loader", loader]
    env = dict(os.environ, M6A_IO_TRACE="1", M6A_LOADER_TIMES="1")
    t0 = time.perf_counter()
    r = subprocess.run(args, cwd=repo, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
    wall = time.perf_counter() - t0
    if r.returncode != 0:
        raise SystemExit("leg %s failed: %s" % (loader, r.stderr[-2000:]))
    res = {"wall_s": wall}
    if loader == "device":
        m = re.search(r"^M6A_TIMES (.*)$", r.stdout, re.M)
        t = json.loads(m.group(1))
        res.update(load_s=t["ms"]["total"] / 1e3, phases_ms=t["ms"], d2h_bytes=t["d2h_bytes"], n_declined_sites=t["n_declined_sites"],
                   peak_bytes=t["peak_bytes"], n_sites=t["n_sites"], n_reads=t["n_reads"])
    else:
        res["load_s"] = sum(float(x) for x in re.findall(r"^m6a_io: .*? ([0-9.]+) ms$", r.stderr, re.M)) / 1e3
    return res


def summary(runs):
    w, ld = [r["wall_s"] for r in runs], [r["load_s"] for r in runs]
    return {"wall_s_median": statistics.median(w), "wall_s_min": min(w), "wall_s_max": max(w), "load_s_median": statistics.median(ld),
            "load_s_min": min(ld), "load_s_max": max(ld), "legs": len(runs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("copies", nargs="?", type=int, default=1400)
    ap.add_argument("--legs", type=int, default=5)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit: its default command is a leg too")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as d:
        size = measure_io.replicate(a.copies, d)
        names = ["host", "device"] + (["parent"] if a.parent else [])
        runs = {n: [] for n in names}
        leg(REPO, d, os.path.join(d, "warm"), "host")           # page cache, the interpreter's files
        for k in range(a.legs):
            for n in names:
                runs[n].append(leg(a.parent if n == "parent" else REPO, d, os.path.join(d, "out_" + n), None if n == "parent" else n))
        same = all(open(os.path.join(d, "out_host", f), "rb").read() == open(os.path.join(d, "out_device", f), "rb").read() for f in CSVS)
        res = {"copies": a.copies, "json_MB": size / 1e6, "csv_bytes_equal": same, "usable_cpus": len(os.sched_getaffinity(0)),
               **{n: summary(runs[n]) for n in names}, "device_last_leg": runs["device"][-1]}
        if a.parent:
            same_p = all(open(os.path.join(d, "out_host", f), "rb").read() == open(os.path.join(d, "out_parent", f), "rb").read() for f in CSVS)
            res["default_command_bytes_equal_parent"] = same_p
            res["default_command_bar_s"] = res["parent"]["wall_s_median"] + (res["parent"]["wall_s_max"] - res["parent"]["wall_s_min"])
            res["default_command_within_bar"] = res["host"]["wall_s_median"] <= res["default_command_bar_s"]
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
