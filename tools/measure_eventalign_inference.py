#!/usr/bin/env python3
"""`eventalign_inference` against the two-step path (`dataprep --device cpu`, then `inference`), from process start to exit, on the
reference's bundled eventalign.txt replicated with distinct transcript ids per copy (as tools/measure_dataprep_gpu.py and
tools/measure_pipeline.py build it), page-cache warm.

    python tools/measure_eventalign_inference.py [--shapes 1400,23.1GB] [--out profiles/r07_eventalign_inference.json] [--timeout 900]

A shape is a number of copies (1400: tools/measure_pipeline.py's shape) or a size in GB.  Every command runs in a child process of
its own under `timeout -k` (one that hangs ends there and nothing more is started), with --n_processes 16 for all three.  Records
both wall times, the fused path's phases (M6A_EVENTALIGN_TIMES: upload, newline offsets, parse + combine + windows, back half,
host, device-to-host copies and bytes, infer, CSV write) and whether the two CSVs are byte-identical."""
import filecmp
import gzip
import json
import os
import subprocess
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "golden", "ref_tests_data", "eventalign.txt.gz")
CSVS = ("data.site_proba.csv", "data.indiv_proba.csv")
THREADS = ["--n_processes", "16"]


def timed(cmd, limit, env=None):
    t0 = time.perf_counter()
    p = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, "-m", "m6anet_amd"] + cmd, capture_output=True, text=True,
                       cwd=REPO, env=env)
    return time.perf_counter() - t0, p


def shape(tag, ev_dir, limit):
    text = gzip.open(SRC, "rt").read()
    header, body = text.split("\n", 1)
    n = int(float(tag[:-2]) * 1e9 / len(body)) if tag.endswith("GB") else int(tag)
    path = os.path.join(ev_dir, "eventalign_%s.txt" % tag)
    with open(path, "w", buffering=16 << 20) as f:
        f.write(header + "\n")
        for k in range(n):
            f.write(body.replace("ENST", "C%dENST" % k) if k else body)
    subprocess.run(["cat", path], stdout=subprocess.DEVNULL, check=True)          # page-cache warm
    res = {"copies": n, "eventalign_GB": os.path.getsize(path) / 1e9}
    prep, two, fused = (os.path.join(ev_dir, tag + s) for s in ("_prep", "_two", "_fused"))
    s1, p1 = timed(["dataprep", "--eventalign", path, "--out_dir", prep] + THREADS, limit)
    if p1.returncode != 0:
        res["two_step"] = {"rc": p1.returncode, "stderr_tail": p1.stderr[-2000:]}
        return res
    s2, p2 = timed(["inference", "--input_dir", prep, "--out_dir", two] + THREADS, limit)
    if p2.returncode != 0:
        res["two_step"] = {"rc": p2.returncode, "stderr_tail": p2.stderr[-2000:]}
        return res
    res["two_step"] = {"s": s1 + s2, "dataprep_s": s1, "inference_s": s2}
    s3, p3 = timed(["eventalign_inference", "--eventalign", path, "--out_dir", fused] + THREADS, limit,
                   env=dict(os.environ, M6A_EVENTALIGN_TIMES="1"))
    if p3.returncode != 0:
        res["fused"] = {"rc": p3.returncode, "stderr_tail": p3.stderr[-2000:]}
        return res
    t = json.loads(p3.stdout.split("M6A_TIMES ", 1)[1].splitlines()[0])
    t["s"] = s3
    t["d2h_bytes_per_read"] = t["d2h_bytes"] / max(1, t["n_reads"])
    res["fused"] = t
    res["csvs_identical"] = all(filecmp.cmp(os.path.join(two, f), os.path.join(fused, f), shallow=False) for f in CSVS)
    res["fused_over_two_step_speed"] = res["two_step"]["s"] / s3
    for d in (prep, two, fused):
        subprocess.run(["rm", "-rf", d], check=False)
    os.remove(path)
    return res


def main():
    shapes = sys.argv[sys.argv.index("--shapes") + 1].split(",") if "--shapes" in sys.argv else ["1400", "23.1GB"]
    dest = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(REPO, "profiles", "r07_eventalign_inference.json")
    limit = int(sys.argv[sys.argv.index("--timeout") + 1]) if "--timeout" in sys.argv else 900
    res = {}
    with tempfile.TemporaryDirectory(dir=os.environ.get("M6A_MEASURE_TMP")) as d:
        for tag in shapes:
            res[tag] = shape(tag, d, limit)
            print(json.dumps({tag: res[tag]}), flush=True)
            if "csvs_identical" not in res[tag]:
                break                                       # a failed step: nothing more is started
    os.makedirs(os.path.dirname(dest), exist_ok=True)
    with open(dest, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
