#!/usr/bin/env python3
"""`eventalign_inference` against the two-step path (`dataprep --device cpu`, then `inference`), from process start to exit, on the
reference's bundled eventalign.txt replicated with distinct transcript ids per copy (as tools/measure_dataprep_gpu.py and
tools/measure_pipeline.py build it), page-cache warm.

    python tools/measure_eventalign_inference.py [--shapes 1400,23.1GB] [--out profiles/r07_eventalign_inference.json] [--timeout 900]

A shape is a number of copies (1400: tools/measure_pipeline.py's shape) or a size in GB.  Every command runs in a child process of
its own under `timeout -k` (one that hangs ends there and nothing more is started), with --n_processes 16 for all three.  Records
both wall times, the fused path's phases (M6A_EVENTALIGN_TIMES: upload, newline offsets, parse + combine + windows, back half,
host, device-to-host copies and bytes, infer, CSV write) and whether the two CSVs are byte-identical.

    python tools/measure_eventalign_inference.py --replicates 3 [--shapes 3.1GB] [--legs 3] [--parent_tree DIR] [--copy_rate]
                                                 [--out profiles/r08_eventalign_replicates.json]

The shape's file K times as K replicates.  Legs are interleaved and the medians reported: (a) the fused command on the K files
against K `dataprep`s and one `inference` over their K directories; (b) with --parent_tree (a built checkout of the parent commit)
the ONE-file fused command of this tree against that tree's, the bar being the parent's median plus its own spread (max - min of its
legs); (c) with --copy_rate one more fused run under `rocprofv3 --kernel-trace --stats`, a run of its own: pool_copy_kernel's bytes
read + written over its time, next to a device-to-device copy of the same bytes (torch) on the same device.

    python tools/measure_eventalign_inference.py --csv host,device [--shapes 1400,23.1GB] [--replicates 3] [--legs 5] [--parent_tree DIR]
                                                 [--copy_rate] [--out profiles/r09_csv_device.json]

The two CSV writers of this tree as interleaved legs of the same command (one file, or the shape's file K times with --replicates K):
medians, the phase table of every leg, and the bar -- the --csv device median below the --csv host median by more than the host legs'
spread (max - min).  With --parent_tree the default command (one file) against the parent's, the bar of mode (b).  With --copy_rate
one more --csv device run under `rocprofv3 --kernel-trace --stats`, a run of its own: csv_indiv_kernel's bytes read + written over
its time next to a device-to-device copy of as many bytes.

    python tools/measure_eventalign_inference.py --window_mb 0,256,1024,4096 [--shapes 3.1GB,24.3GB] [--legs 5] [--parent_tree DIR]
                                                 [--budget_mb 16384[,22528]] [--out profiles/r10_eventalign_windows.json]

The one-file command with each --window_mb (0: the whole file, the flag left out) as interleaved legs: medians, the phase table of
every leg with n_windows and peak_bytes, every windowed leg's CSVs compared with the whole-file leg's, the ratio of each windowed
median to the whole-file median and the best window.  No bar is set for that ratio.  With --parent_tree the default command against
the parent's, the bar of mode (b).  With --budget_mb B[,B...], on shapes larger than B: one more leg per B with M6A_PREP_BUDGET_MB=B and
the window with the lowest peak_bytes -- CSVs compared again, peak_bytes recorded, or the refusal's text: the rows of the whole file must
still fit -- and the whole-file command under the same budget, which must refuse the file.

    python tools/measure_eventalign_inference.py --bgzf [--shapes 3.1GB,24.3GB] [--legs 5] [--parent_tree DIR]
                                                 [--out profiles/r11_eventalign_bgzf.json]

The shape's file and its BGZF twin (m6anet_amd/bgzf.py, level 6, 16 processes) as interleaved legs of the one-file command: medians,
the phase table of every leg (upload wait, inflate + CRC ms, peak_bytes), the compression ratio of this GENERATED text, the inflate
rate in GB/s of text produced beside the link's upload rate from the same legs, and the CSVs of the two inputs compared.  The
compressed leg carries no bar.  With --parent_tree the default command on the plain file against the parent's, the bar of mode (b).
Both files are read from a warm page cache; a cold read from disk, which is what compressed input is for, is not measured here.

    python tools/measure_eventalign_inference.py --compress [--shapes 3.1GB,24.3GB] [--legs 5] [--parent_tree DIR]
                                                 [--out profiles/r13_csv_bgzf_dynamic.json]

`--csv device` plain, with `--compress` (level 1, fixed Huffman codes) and with `--compress --compress_level 2` (dynamic codes) as
interleaved legs of the one-file command: medians, the phase table of every leg (csv_format, csv_deflate, csv_copy, csv_pwrite ms),
device-to-host bytes per read, the compressed files' size over the text, the stored blocks and at level 2 the fixed and dynamic ones,
and level 2 over level 1 in csv_deflate ms, bytes and command time; every leg's .gz files are inflated (`gzip -dc`) and compared with
the plain leg's files.  The compressed legs carry no bar against the plain leg: which is faster is reported.  With --parent_tree the
default command against the parent's, the bar of mode (b), and this tree's `--compress` leg against the parent's `--compress`
command under the same rule (parent median + parent spread): level 2 is meant to leave both alone.

    python tools/measure_eventalign_inference.py --read_names [--shapes 3.1GB] [--legs 5] [--parent_tree DIR]
                                                 [--out profiles/r15_read_names.json]

The shape's file and its named twin -- every read index replaced by a UUID from a seeded bijection, as nanopolish --print-read-names
writes the column -- as interleaved legs of the one-file command, the named leg with --read_names: medians, the phase table of every
leg with the `intern` phase and n_read_names, the named file's size over the indexed one's, data.site_proba.csv of the two compared
and the rows of data.indiv_proba.csv counted.  The named leg carries no bar (its lines are 30-odd bytes longer, so it uploads more).
With --parent_tree the default command on the indexed file against the parent's, the bar of mode (b).

    python tools/measure_eventalign_inference.py --stream [--shapes 3.1GB] [--legs 5] [--window_mb 256] [--parent_tree DIR]
                                                 [--out profiles/r16_stream_input.json]

The shape's file read as a file and as a stream, interleaved legs of the one-file command at the same window size: `--eventalign FILE
--window_mb W` and `cat FILE | ... --eventalign - --window_mb W` (the time is the pipeline's: cat is started with the command and has
ended when it has).  Medians, the phase table of every leg with stream_bytes and n_streams, the stream's bytes per second of its
upload wait, peak and device-to-host bytes, and the CSV files of the two compared.  The stream leg carries no bar: a pipe moves its
bytes through read() and may be slower than pread from the page cache; which is faster is reported.  With --parent_tree the default
command (no window, a file) against the parent's, the bar of mode (b).

    python tools/measure_eventalign_inference.py --grouped [--shapes 3.1GB] [--legs 5] [--window_mb 256]
                                                 [--group_kb 65536,262144,1048576] [--parent_tree DIR] [--out profiles/r30_grouped_input.json]

The shape's file, checked to be grouped by transcript, as interleaved legs of the whole command, each in its own process: the default;
--window_mb W; --grouped --window_mb W at every group size (M6A_PREP_GROUP_KB); the same from `cat FILE |`.  Per leg the wall time, the
time at which data.site_proba.csv first held a row (polled from outside), peak_bytes, max_kept_rows and n_batches, and the CSV files
compared with the default's.  Then one leg with M6A_PREP_BUDGET_MB just under what the windowed leg needed: windowed refused and
grouped completed as yes / no, CSVs identical as yes / no.  The grouped legs carry no bar (they add a back half per batch); with
--parent_tree the default command against the parent's, the bar of mode (b)."""
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


def timed(cmd, limit, env=None, tree=REPO, wrap=()):
    t0 = time.perf_counter()
    p = subprocess.run(["timeout", "-k", "10", str(limit)] + list(wrap) + [sys.executable, "-m", "m6anet_amd"] + cmd, capture_output=True,
                       text=True, cwd=tree, env=env)
    return time.perf_counter() - t0, p


def write_shape(tag, ev_dir):
    text = gzip.open(SRC, "rt").read()
    header, body = text.split("\n", 1)
    n = int(float(tag[:-2]) * 1e9 / len(body)) if tag.endswith("GB") else int(tag)
    path = os.path.join(ev_dir, "eventalign_%s.txt" % tag)
    with open(path, "w", buffering=16 << 20) as f:
        f.write(header + "\n")
        for k in range(n):
            f.write(body.replace("ENST", "C%dENST" % k) if k else body)
    subprocess.run(["cat", path], stdout=subprocess.DEVNULL, check=True)          # page-cache warm
    return path, n


def median(v):
    v = sorted(v)
    return v[len(v) // 2] if len(v) % 2 else 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2])


class StepFailed(Exception):
    pass


def must(s, p, what):
    if p.returncode != 0:
        raise StepFailed({"step": what, "rc": p.returncode, "stderr_tail": p.stderr[-2000:]})
    return s


def copy_rate(path, K, ev_dir, limit):
    """(c): pool_copy_kernel under the kernel trace, and a device-to-device copy of as many bytes"""
    import glob
    out = os.path.join(ev_dir, "trace")
    s, p = timed(["eventalign_inference", "--eventalign"] + [path] * K + ["--out_dir", os.path.join(ev_dir, "trace_out")] + THREADS, limit,
                 env=dict(os.environ, M6A_EVENTALIGN_TIMES="1"), wrap=["rocprofv3", "--kernel-trace", "--stats", "-d", out, "--"])
    must(s, p, "fused under rocprofv3")
    t = json.loads(p.stdout.split("M6A_TIMES ", 1)[1].splitlines()[0])
    import sqlite3
    ns = None
    for fn in glob.glob(os.path.join(out, "**", "*_results.db"), recursive=True):      # the rocpd database, as tools/rocpd_summary.py reads it
        con = sqlite3.connect(fn)
        cols = [r[1] for r in con.execute("pragma table_info(kernels)")]
        name = "name" if "name" in cols else "kernel_name"
        row = con.execute("select sum(end - start), count(*) from kernels where %s like '%%pool_copy_kernel%%'" % name).fetchone()
        con.close()
        if row and row[1] == 1:
            ns = float(row[0])
    if ns is None:
        raise StepFailed({"step": "kernel trace", "error": "no single pool_copy_kernel launch in the trace under %s" % out})
    moved = 2 * 44 * t["n_reads"]                          # X (36 B) and the read id (8 B) of every pooled read, read and written
    import torch
    a = torch.empty(moved // 2, dtype=torch.uint8, device="cuda")
    b = torch.empty_like(a)
    times = []
    for _ in range(12):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        b.copy_(a)
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) * 1e6)
    d2d = median(times[2:])
    return {"n_reads": t["n_reads"], "n_sites": t["n_sites"], "bytes_read_and_written": moved, "pool_copy_kernel_ns": ns,
            "pool_copy_GBps": moved / ns, "d2d_copy_ns": d2d, "d2d_copy_GBps": moved / d2d, "ratio": d2d / ns}


def kernel_ns(trace_dir, like):
    """(summed duration in ns, launches) of the kernels whose name contains `like`, from the rocpd database under trace_dir"""
    import glob
    import sqlite3
    for fn in glob.glob(os.path.join(trace_dir, "**", "*_results.db"), recursive=True):
        con = sqlite3.connect(fn)
        cols = [r[1] for r in con.execute("pragma table_info(kernels)")]
        name = "name" if "name" in cols else "kernel_name"
        row = con.execute("select sum(end - start), count(*) from kernels where %s like '%%%s%%'" % (name, like)).fetchone()
        con.close()
        if row and row[1]:
            return float(row[0]), int(row[1])
    return None, 0


def csv_copy_rate(paths, ev_dir, limit):
    """csv_indiv_kernel under the kernel trace: per read it reads the id (8 B) and the probability (4 B) and writes the row's text"""
    out = os.path.join(ev_dir, "trace")
    s, p = timed(["eventalign_inference", "--eventalign"] + paths + ["--out_dir", os.path.join(ev_dir, "trace_out"), "--csv", "device"] + THREADS,
                 limit, env=dict(os.environ, M6A_EVENTALIGN_TIMES="1"), wrap=["rocprofv3", "--kernel-trace", "--stats", "-d", out, "--"])
    must(s, p, "--csv device under rocprofv3")
    t = json.loads(p.stdout.split("M6A_TIMES ", 1)[1].splitlines()[0])
    ns, n = kernel_ns(out, "csv_indiv_kernel")
    if ns is None:
        raise StepFailed({"step": "kernel trace", "error": "no csv_indiv_kernel launch in the trace under %s" % out})
    len_ns, _ = kernel_ns(out, "csv_len_kernel")
    indiv = os.path.getsize(os.path.join(ev_dir, "trace_out", CSVS[1]))
    moved = indiv + 12 * t["n_reads"]
    import torch
    a = torch.empty(moved // 2, dtype=torch.uint8, device="cuda")
    b = torch.empty_like(a)
    times = []
    for _ in range(12):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        b.copy_(a)
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) * 1e6)
    d2d = median(times[2:])
    subprocess.run(["rm", "-rf", out, os.path.join(ev_dir, "trace_out")], check=False)
    return {"n_reads": t["n_reads"], "n_sites": t["n_sites"], "indiv_text_bytes": indiv, "bytes_read_and_written": moved, "csv_indiv_kernel_ns": ns,
            "csv_indiv_kernel_launches": n, "csv_len_kernel_ns": len_ns, "csv_indiv_GBps": moved / ns, "d2d_copy_ns": d2d,
            "d2d_copy_GBps": moved / d2d, "ratio": d2d / ns}


def csv_writers(tag, K, legs, parent, with_copy_rate, ev_dir, limit):
    path, n = write_shape(tag, ev_dir)
    paths = [path] * K
    res = {"copies": n, "eventalign_GB": os.path.getsize(path) / 1e9, "replicates": K, "legs": legs}
    runs = {"host": [], "device": []}
    one, par = [], []
    env = dict(os.environ, M6A_EVENTALIGN_TIMES="1")
    try:
        for leg in range(legs):
            for mode in ("host", "device"):
                out = os.path.join(ev_dir, "csv_" + mode)
                s, p = timed(["eventalign_inference", "--eventalign"] + paths + ["--out_dir", out, "--csv", mode] + THREADS, limit, env=env)
                must(s, p, "--csv " + mode)
                t = json.loads(p.stdout.split("M6A_TIMES ", 1)[1].splitlines()[0])
                t["s"] = s
                runs[mode].append(t)
            res["csvs_identical"] = all(filecmp.cmp(os.path.join(ev_dir, "csv_host", f), os.path.join(ev_dir, "csv_device", f), shallow=False)
                                        for f in CSVS)
            res["csv_bytes"] = [os.path.getsize(os.path.join(ev_dir, "csv_device", f)) for f in CSVS]
            if parent:
                cmd = ["eventalign_inference", "--eventalign", path, "--out_dir", os.path.join(ev_dir, "one")] + THREADS
                one.append(must(*timed(cmd, limit), "default command, this tree"))
                cmd[4] = os.path.join(ev_dir, "one_parent")
                par.append(must(*timed(cmd, limit, tree=parent), "default command, parent tree"))
                res["one_file_csvs_identical"] = all(filecmp.cmp(os.path.join(ev_dir, "one", f), os.path.join(ev_dir, "one_parent", f),
                                                                 shallow=False) for f in CSVS)
            for d in ("csv_host", "csv_device", "one", "one_parent"):
                subprocess.run(["rm", "-rf", os.path.join(ev_dir, d)], check=False)
            print("%s: leg %d of %d: --csv host %.2f s, --csv device %.2f s" % (tag, leg + 1, legs, runs["host"][-1]["s"], runs["device"][-1]["s"]),
                  file=sys.stderr, flush=True)
        for mode in runs:
            res[mode] = {"median_s": median([x["s"] for x in runs[mode]]), "legs": runs[mode]}
        hs = [x["s"] for x in runs["host"]]
        res["host_spread_s"] = max(hs) - min(hs)
        res["device_below_host_by_s"] = res["host"]["median_s"] - res["device"]["median_s"]
        res["device_beats_host_by_more_than_the_spread"] = res["device_below_host_by_s"] > res["host_spread_s"]
        if parent:
            res["default_command"] = {"this_s": one, "parent_s": par, "this_median_s": median(one), "parent_median_s": median(par),
                                      "parent_spread_s": max(par) - min(par), "bar_s": median(par) + max(par) - min(par),
                                      "within_bar": median(one) <= median(par) + max(par) - min(par)}
        if with_copy_rate:
            res["csv_kernel"] = csv_copy_rate(paths, ev_dir, limit)
    except StepFailed as e:
        res["failed"] = e.args[0]
        res["legs_done"] = runs
    os.remove(path)
    return res


def windows(tag, sizes, legs, parent, budget_mb, ev_dir, limit):
    path, n = write_shape(tag, ev_dir)
    res = {"copies": n, "eventalign_GB": os.path.getsize(path) / 1e9, "legs": legs, "window_mb": sizes}
    runs = {mb: [] for mb in sizes}
    one, par = [], []
    env = dict(os.environ, M6A_EVENTALIGN_TIMES="1")
    env.pop("M6A_PREP_WINDOW_KB", None)
    env.pop("M6A_PREP_BUDGET_MB", None)

    def command(mb, out, env, check=True):
        cmd = ["eventalign_inference", "--eventalign", path, "--out_dir", os.path.join(ev_dir, out)] + THREADS
        s, p = timed(cmd + (["--window_mb", str(mb)] if mb else []), limit, env=env)
        if not check:
            return s, p
        must(s, p, "--window_mb %d" % mb)
        t = json.loads(p.stdout.split("M6A_TIMES ", 1)[1].splitlines()[0])
        t["s"] = s
        return t

    def same(a, b):
        return all(filecmp.cmp(os.path.join(ev_dir, a, f), os.path.join(ev_dir, b, f), shallow=False) for f in CSVS)
    try:
        identical = True
        for leg in range(legs):
            for mb in sizes:
                runs[mb].append(command(mb, "w%d" % mb, env))
            identical = identical and all(same("w0", "w%d" % mb) for mb in sizes if mb)
            if parent:
                cmd = ["eventalign_inference", "--eventalign", path, "--out_dir", os.path.join(ev_dir, "one")] + THREADS
                one.append(must(*timed(cmd, limit, env=env), "default command, this tree"))
                cmd[4] = os.path.join(ev_dir, "one_parent")
                par.append(must(*timed(cmd, limit, env=env, tree=parent), "default command, parent tree"))
                res["one_file_csvs_identical"] = same("one", "one_parent")
            print("%s: leg %d of %d: %s" % (tag, leg + 1, legs, ", ".join("%d MB %.2f s" % (mb, runs[mb][-1]["s"]) for mb in sizes)),
                  file=sys.stderr, flush=True)
        res["csvs_identical"] = identical
        res["csv_bytes"] = [os.path.getsize(os.path.join(ev_dir, "w0", f)) for f in CSVS]
        for mb in sizes:
            res["%d" % mb] = {"median_s": median([x["s"] for x in runs[mb]]), "n_windows": runs[mb][-1]["n_windows"],
                              "peak_bytes": runs[mb][-1]["peak_bytes"], "legs": runs[mb]}
        whole = res["0"]["median_s"]
        ws = [x["s"] for x in runs[0]]
        res["whole_file_spread_s"] = max(ws) - min(ws)
        res["windowed_over_whole_file_time"] = {"%d" % mb: res["%d" % mb]["median_s"] / whole for mb in sizes if mb}
        best = min((mb for mb in sizes if mb), key=lambda mb: res["%d" % mb]["median_s"])
        res["best_window_mb"] = best
        if parent:
            res["default_command"] = {"this_s": one, "parent_s": par, "this_median_s": median(one), "parent_median_s": median(par),
                                      "parent_spread_s": max(par) - min(par), "bar_s": median(par) + max(par) - min(par),
                                      "within_bar": median(one) <= median(par) + max(par) - min(par)}
        lean = min((mb for mb in sizes if mb), key=lambda mb: res["%d" % mb]["peak_bytes"])
        res["under_budget"] = []
        for mb in budget_mb:
            if os.path.getsize(path) <= mb << 20:          # only a file larger than the memory allowed
                continue
            tight = dict(env, M6A_PREP_BUDGET_MB=str(mb))
            s, p = command(lean, "tight", tight, check=False)
            leg = {"budget_mb": mb, "window_mb": lean, "s": s}
            if p.returncode != 0:                          # the rows of the whole file must still fit: a finding, not a failed step
                leg["refused"] = p.stderr.strip().splitlines()[-1][-400:]
            else:
                t = json.loads(p.stdout.split("M6A_TIMES ", 1)[1].splitlines()[0])
                leg.update(peak_bytes=t["peak_bytes"], n_windows=t["n_windows"], ms=t["ms"], csvs_identical=same("w0", "tight"),
                           peak_under_budget=t["peak_bytes"] <= mb << 20)
            s, p = command(0, "tight_whole", tight, check=False)
            leg["whole_file_refused"] = p.returncode != 0 and "two-step path" in p.stderr
            res["under_budget"].append(leg)
    except StepFailed as e:
        res["failed"] = e.args[0]
        res["legs_done"] = {"%d" % mb: v for mb, v in runs.items()}
    for d in ["w%d" % mb for mb in sizes] + ["one", "one_parent", "tight", "tight_whole"]:
        subprocess.run(["rm", "-rf", os.path.join(ev_dir, d)], check=False)
    os.remove(path)
    return res


def bgzf_legs(tag, legs, parent, ev_dir, limit):
    sys.path.insert(0, REPO)
    from m6anet_amd import bgzf
    path, n = write_shape(tag, ev_dir)
    t0 = time.perf_counter()
    n_in, n_out = bgzf.compress_file(path, level=6, n_processes=16)
    gz = path + ".gz"
    subprocess.run(["cat", gz], stdout=subprocess.DEVNULL, check=True)             # page-cache warm, like the text
    res = {"copies": n, "eventalign_GB": n_in / 1e9, "compressed_GB": n_out / 1e9, "compression_ratio_of_generated_text": n_in / n_out,
           "compress_s": time.perf_counter() - t0, "legs": legs, "cold_cache_read": "not measured"}
    runs = {"plain": [], "bgzf": []}
    one, par = [], []
    env = dict(os.environ, M6A_EVENTALIGN_TIMES="1")
    env.pop("M6A_PREP_WINDOW_KB", None)
    try:
        for leg in range(legs):
            for mode, src in (("plain", path), ("bgzf", gz)):
                s, p = timed(["eventalign_inference", "--eventalign", src, "--out_dir", os.path.join(ev_dir, mode)] + THREADS, limit, env=env)
                must(s, p, mode)
                t = json.loads(p.stdout.split("M6A_TIMES ", 1)[1].splitlines()[0])
                t["s"] = s
                runs[mode].append(t)
            res["csvs_identical"] = all(filecmp.cmp(os.path.join(ev_dir, "plain", f), os.path.join(ev_dir, "bgzf", f), shallow=False) for f in CSVS)
            if parent:
                cmd = ["eventalign_inference", "--eventalign", path, "--out_dir", os.path.join(ev_dir, "one")] + THREADS
                one.append(must(*timed(cmd, limit), "default command, this tree"))
                cmd[4] = os.path.join(ev_dir, "one_parent")
                par.append(must(*timed(cmd, limit, tree=parent), "default command, parent tree"))
                res["one_file_csvs_identical"] = all(filecmp.cmp(os.path.join(ev_dir, "one", f), os.path.join(ev_dir, "one_parent", f),
                                                                 shallow=False) for f in CSVS)
            for d in ("plain", "bgzf", "one", "one_parent"):
                subprocess.run(["rm", "-rf", os.path.join(ev_dir, d)], check=False)
            print("%s: leg %d of %d: plain %.2f s, bgzf %.2f s" % (tag, leg + 1, legs, runs["plain"][-1]["s"], runs["bgzf"][-1]["s"]),
                  file=sys.stderr, flush=True)
        for mode in runs:
            v = runs[mode]
            res[mode] = {"median_s": median([x["s"] for x in v]), "upload_wait_ms": median([x["ms"]["upload"] for x in v]),
                         "upload_GBps": median([x["ms"]["upload_GBps"] for x in v]), "inflate_and_crc_ms": median([x["inflate"] for x in v]),
                         "peak_bytes": v[-1]["peak_bytes"], "legs": v}
        res["bgzf"]["inflate_GBps_of_text"] = n_in / (res["bgzf"]["inflate_and_crc_ms"] * 1e6) if res["bgzf"]["inflate_and_crc_ms"] else None
        res["bgzf"]["n_bgzf_blocks"] = runs["bgzf"][-1]["n_bgzf_blocks"]
        res["bgzf_over_plain_time"] = res["bgzf"]["median_s"] / res["plain"]["median_s"]
        if parent:
            res["default_command"] = {"this_s": one, "parent_s": par, "this_median_s": median(one), "parent_median_s": median(par),
                                      "parent_spread_s": max(par) - min(par), "bar_s": median(par) + max(par) - min(par),
                                      "within_bar": median(one) <= median(par) + max(par) - min(par)}
    except StepFailed as e:
        res["failed"] = e.args[0]
        res["legs_done"] = runs
    os.remove(path)
    os.remove(gz)
    return res


def write_named_shape(tag, ev_dir, seed=15):
    """write_shape's file with field 4 of every body line replaced by the UUID of its read index (one seeded UUID per index)"""
    import random
    import re
    import uuid
    text = gzip.open(SRC, "rt").read()
    header, body = text.split("\n", 1)
    n = int(float(tag[:-2]) * 1e9 / len(body)) if tag.endswith("GB") else int(tag)       # as many copies as the indexed file has
    rng, book = random.Random(seed), {}

    def name(m):
        if m.group(2) not in book:
            book[m.group(2)] = str(uuid.UUID(int=rng.getrandbits(128)))
        return m.group(1) + book[m.group(2)]
    body = re.sub(r"^([^\t\n]*\t[^\t\n]*\t[^\t\n]*\t)([^\t\n]*)", name, body, flags=re.M)
    path = os.path.join(ev_dir, "eventalign_%s_named.txt" % tag)
    with open(path, "w", buffering=16 << 20) as f:
        f.write(header + "\n")
        for k in range(n):
            f.write(body.replace("ENST", "C%dENST" % k) if k else body)
    subprocess.run(["cat", path], stdout=subprocess.DEVNULL, check=True)          # page-cache warm
    return path, len(book)


def read_names_legs(tag, legs, parent, ev_dir, limit):
    path, n = write_shape(tag, ev_dir)
    named, n_names = write_named_shape(tag, ev_dir)
    res = {"copies": n, "eventalign_GB": os.path.getsize(path) / 1e9, "named_GB": os.path.getsize(named) / 1e9,
           "named_over_indexed_bytes": os.path.getsize(named) / os.path.getsize(path), "names_per_copy": n_names, "legs": legs}
    runs = {"indexed": [], "named": []}
    one, par = [], []
    env = dict(os.environ, M6A_EVENTALIGN_TIMES="1")
    env.pop("M6A_PREP_WINDOW_KB", None)
    try:
        for leg in range(legs):
            for mode, src, flag in (("indexed", path, []), ("named", named, ["--read_names"])):
                s, p = timed(["eventalign_inference", "--eventalign", src, "--out_dir", os.path.join(ev_dir, mode)] + flag + THREADS, limit, env=env)
                must(s, p, mode)
                t = json.loads(p.stdout.split("M6A_TIMES ", 1)[1].splitlines()[0])
                t["s"] = s
                runs[mode].append(t)
            a, b = (os.path.join(ev_dir, m) for m in ("indexed", "named"))
            res["site_proba_identical"] = filecmp.cmp(os.path.join(a, CSVS[0]), os.path.join(b, CSVS[0]), shallow=False)
            rows = [int(subprocess.run(["wc", "-l", os.path.join(d, CSVS[1])], capture_output=True, text=True, check=True).stdout.split()[0]) for d in (a, b)]
            res["indiv_proba_rows"] = {"indexed": rows[0], "named": rows[1], "equal": rows[0] == rows[1]}
            if parent:
                cmd = ["eventalign_inference", "--eventalign", path, "--out_dir", os.path.join(ev_dir, "one")] + THREADS
                one.append(must(*timed(cmd, limit), "default command, this tree"))
                cmd[4] = os.path.join(ev_dir, "one_parent")
                par.append(must(*timed(cmd, limit, tree=parent), "default command, parent tree"))
                res["one_file_csvs_identical"] = all(filecmp.cmp(os.path.join(ev_dir, "one", f), os.path.join(ev_dir, "one_parent", f),
                                                                 shallow=False) for f in CSVS)
            for d in ("indexed", "named", "one", "one_parent"):
                subprocess.run(["rm", "-rf", os.path.join(ev_dir, d)], check=False)
            print("%s: leg %d of %d: indexed %.2f s, named %.2f s" % (tag, leg + 1, legs, runs["indexed"][-1]["s"], runs["named"][-1]["s"]),
                  file=sys.stderr, flush=True)
        for mode in runs:
            v = runs[mode]
            res[mode] = {"median_s": median([x["s"] for x in v]), "upload_wait_ms": median([x["ms"]["upload"] for x in v]),
                         "intern_ms": median([x["ms"]["intern"] for x in v]), "back_half_ms": median([x["ms"]["back_half"] for x in v]),
                         "n_read_names": v[-1]["n_read_names"], "peak_bytes": v[-1]["peak_bytes"], "d2h_bytes": v[-1]["d2h_bytes"], "legs": v}
        res["named_over_indexed_time"] = res["named"]["median_s"] / res["indexed"]["median_s"]
        if parent:
            res["default_command"] = {"this_s": one, "parent_s": par, "this_median_s": median(one), "parent_median_s": median(par),
                                      "parent_spread_s": max(par) - min(par), "bar_s": median(par) + max(par) - min(par),
                                      "within_bar": median(one) <= median(par) + max(par) - min(par)}
    except StepFailed as e:
        res["failed"] = e.args[0]
        res["legs_done"] = runs
    os.remove(path)
    os.remove(named)
    return res


def timed_from_pipe(path, cmd, limit, env=None):
    """`cat path | python -m m6anet_amd cmd`: the wall time of the two and the command's result"""
    t0 = time.perf_counter()
    cat = subprocess.Popen(["cat", path], stdout=subprocess.PIPE)
    try:
        p = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, "-m", "m6anet_amd"] + cmd, stdin=cat.stdout, capture_output=True,
                           text=True, cwd=REPO, env=env)
    finally:
        cat.stdout.close()                                  # a command that ended early: cat meets a closed pipe and ends
        cat.wait()
    return time.perf_counter() - t0, p


def stream_legs(tag, legs, window_mb, parent, ev_dir, limit):
    path, n = write_shape(tag, ev_dir)
    res = {"copies": n, "eventalign_GB": os.path.getsize(path) / 1e9, "legs": legs, "window_mb": window_mb}
    runs = {"file": [], "stream": []}
    one, par = [], []
    env = dict(os.environ, M6A_EVENTALIGN_TIMES="1")
    env.pop("M6A_PREP_WINDOW_KB", None)
    flags = ["--window_mb", str(window_mb)] + THREADS
    try:
        for leg in range(legs):
            s, p = timed(["eventalign_inference", "--eventalign", path, "--out_dir", os.path.join(ev_dir, "file")] + flags, limit, env=env)
            must(s, p, "file")
            runs["file"].append(dict(json.loads(p.stdout.split("M6A_TIMES ", 1)[1].splitlines()[0]), s=s))
            s, p = timed_from_pipe(path, ["eventalign_inference", "--eventalign", "-", "--out_dir", os.path.join(ev_dir, "stream")] + flags, limit, env=env)
            must(s, p, "stream")
            runs["stream"].append(dict(json.loads(p.stdout.split("M6A_TIMES ", 1)[1].splitlines()[0]), s=s))
            res["csvs_identical"] = all(filecmp.cmp(os.path.join(ev_dir, "file", f), os.path.join(ev_dir, "stream", f), shallow=False) for f in CSVS)
            if parent:
                cmd = ["eventalign_inference", "--eventalign", path, "--out_dir", os.path.join(ev_dir, "one")] + THREADS
                one.append(must(*timed(cmd, limit), "default command, this tree"))
                cmd[4] = os.path.join(ev_dir, "one_parent")
                par.append(must(*timed(cmd, limit, tree=parent), "default command, parent tree"))
                res["one_file_csvs_identical"] = all(filecmp.cmp(os.path.join(ev_dir, "one", f), os.path.join(ev_dir, "one_parent", f),
                                                                 shallow=False) for f in CSVS)
            for d in ("file", "stream", "one", "one_parent"):
                subprocess.run(["rm", "-rf", os.path.join(ev_dir, d)], check=False)
            print("%s: leg %d of %d: file %.2f s, stream %.2f s" % (tag, leg + 1, legs, runs["file"][-1]["s"], runs["stream"][-1]["s"]),
                  file=sys.stderr, flush=True)
        for mode in runs:
            v = runs[mode]
            res[mode] = {"median_s": median([x["s"] for x in v]), "upload_wait_ms": median([x["ms"]["upload"] for x in v]),
                         "upload_GBps": median([x["ms"]["upload_GBps"] for x in v]), "back_half_ms": median([x["ms"]["back_half"] for x in v]),
                         "n_windows": v[-1]["n_windows"], "window_bytes": v[-1]["window_bytes"], "stream_bytes": v[-1]["stream_bytes"],
                         "n_streams": v[-1]["n_streams"], "peak_bytes": v[-1]["peak_bytes"], "d2h_bytes": v[-1]["d2h_bytes"], "legs": v}
        res["stream_over_file_time"] = res["stream"]["median_s"] / res["file"]["median_s"]
        if parent:
            res["default_command"] = {"this_s": one, "parent_s": par, "this_median_s": median(one), "parent_median_s": median(par),
                                      "parent_spread_s": max(par) - min(par), "bar_s": median(par) + max(par) - min(par),
                                      "within_bar": median(one) <= median(par) + max(par) - min(par)}
    except StepFailed as e:
        res["failed"] = e.args[0]
        res["legs_done"] = runs
    os.remove(path)
    return res


def check_grouped(path):
    """every contig of the file forms one stretch (lines without a tab belong to no run): what --grouped needs of a shape"""
    closed, current = set(), None
    with open(path, "rb") as f:
        f.readline()
        for line in f:
            tab = line.find(b"\t")
            if tab < 0:
                continue
            name = line[:tab]
            if name != current:
                if current is not None:
                    closed.add(current)
                if name in closed:
                    raise SystemExit("%s is not grouped by transcript: %s appears again" % (path, name.decode()))
                current = name


def timed_watching(cmd, out_dir, limit, env=None, pipe_from=None):
    """timed() or timed_from_pipe() with the time at which data.site_proba.csv first holds a row: polled every 10 ms from outside"""
    import threading
    site = os.path.join(out_dir, CSVS[0])
    seen, stop = [None], threading.Event()
    t0 = time.perf_counter()

    def watch():
        while not stop.is_set():
            try:
                if os.path.getsize(site) > 100:              # the header line is 78 bytes
                    seen[0] = time.perf_counter() - t0
                    return
            except OSError:
                pass
            stop.wait(0.01)
    w = threading.Thread(target=watch, daemon=True)
    w.start()
    try:
        s, p = timed_from_pipe(pipe_from, cmd, limit, env=env) if pipe_from else timed(cmd, limit, env=env)
    finally:
        stop.set()
        w.join()
    return s, p, seen[0]


def grouped_legs(tag, legs, window_mb, group_kbs, parent, ev_dir, limit):
    """--grouped: interleaved legs, each the whole command in its own process -- the default; --window_mb W; --grouped --window_mb W at
    every group size; the same from `cat FILE |`.  Per leg the wall time, when the first CSV row was there, peak_bytes, and for the
    grouped legs max_kept_rows and n_batches.  Then one leg with M6A_PREP_BUDGET_MB just under what the windowed leg needed: windowed
    refused, grouped completed, CSVs identical.  The grouped legs carry no bar; with --parent_tree the default command against the parent's."""
    path, n = write_shape(tag, ev_dir)
    check_grouped(path)
    res = {"copies": n, "eventalign_GB": os.path.getsize(path) / 1e9, "legs": legs, "window_mb": window_mb, "group_kb": group_kbs, "grouped_input": True}
    modes = {"default": ([], None, False), "windows": (["--window_mb", str(window_mb)], None, False)}
    for kb in group_kbs:
        modes["grouped_%d" % kb] = (["--grouped", "--window_mb", str(window_mb)], kb, False)
        modes["grouped_%d_pipe" % kb] = (["--grouped", "--window_mb", str(window_mb)], kb, True)
    runs = {m: [] for m in modes}
    one, par = [], []
    base = dict(os.environ, M6A_EVENTALIGN_TIMES="1")
    for k in ("M6A_PREP_WINDOW_KB", "M6A_PREP_GROUP_KB", "M6A_PREP_BUDGET_MB"):
        base.pop(k, None)
    ref = os.path.join(ev_dir, "default")

    def leg(mode, out, env_more=None):
        flags, kb, piped = modes[mode]
        env = dict(base, **(env_more or {}), **({"M6A_PREP_GROUP_KB": str(kb)} if kb else {}))
        cmd = ["eventalign_inference", "--eventalign", "-" if piped else path, "--out_dir", out] + flags + THREADS
        subprocess.run(["rm", "-rf", out], check=False)       # the watcher must not see an earlier leg's file
        return timed_watching(cmd, out, limit, env=env, pipe_from=path if piped else None)
    try:
        for k in range(legs):
            same = {}
            for mode in modes:
                out = os.path.join(ev_dir, mode)
                s, p, first = leg(mode, out)
                must(s, p, mode)
                t = json.loads(p.stdout.split("M6A_TIMES ", 1)[1].splitlines()[0])
                runs[mode].append(dict(t, s=s, first_csv_row_s=first))
                if mode != "default":
                    same[mode] = all(filecmp.cmp(os.path.join(ref, f), os.path.join(out, f), shallow=False) for f in CSVS)
                    subprocess.run(["rm", "-rf", out], check=False)
            res["csvs_identical"] = same
            if parent:
                cmd = ["eventalign_inference", "--eventalign", path, "--out_dir", os.path.join(ev_dir, "one")] + THREADS
                one.append(must(*timed(cmd, limit), "default command, this tree"))
                cmd[4] = os.path.join(ev_dir, "one_parent")
                par.append(must(*timed(cmd, limit, tree=parent), "default command, parent tree"))
                res["one_file_csvs_identical"] = all(filecmp.cmp(os.path.join(ev_dir, "one", f), os.path.join(ev_dir, "one_parent", f),
                                                                 shallow=False) for f in CSVS)
                for d in ("one", "one_parent"):
                    subprocess.run(["rm", "-rf", os.path.join(ev_dir, d)], check=False)
            print("%s: leg %d of %d: %s" % (tag, k + 1, legs, ", ".join("%s %.2f s" % (m, runs[m][-1]["s"]) for m in modes)), file=sys.stderr, flush=True)
        for mode, v in runs.items():
            res[mode] = {"median_s": median([x["s"] for x in v]),
                         "first_csv_row_s": median([x["first_csv_row_s"] for x in v]) if all(x["first_csv_row_s"] is not None for x in v) else None,
                         "peak_bytes": v[-1]["peak_bytes"], "n_windows": v[-1]["n_windows"], "max_kept_rows": v[-1].get("max_kept_rows"),
                         "max_kept_runs": v[-1].get("max_kept_runs"), "n_batches": v[-1].get("n_batches"), "group_bytes": v[-1].get("group_bytes"),
                         "legs": v}
        # ---- the wall: a budget just under what the windowed leg needed
        budget_mb = max(1, (res["windows"]["peak_bytes"] >> 20) - 1)
        first_grouped = "grouped_%d" % group_kbs[0]
        _, pw, _ = leg("windows", os.path.join(ev_dir, "w_budget"), {"M6A_PREP_BUDGET_MB": str(budget_mb)})
        _, pg, _ = leg(first_grouped, os.path.join(ev_dir, "g_budget"), {"M6A_PREP_BUDGET_MB": str(budget_mb)})
        res["budget"] = {"budget_mb": budget_mb, "windowed_refused": "yes" if pw.returncode != 0 else "no",
                         "grouped_completed": "yes" if pg.returncode == 0 else "no", "grouped_mode": first_grouped,
                         "csvs_identical": "yes" if pg.returncode == 0 and all(
                             filecmp.cmp(os.path.join(ref, f), os.path.join(ev_dir, "g_budget", f), shallow=False) for f in CSVS) else "no"}
        if parent:
            res["default_command"] = {"this_s": one, "parent_s": par, "this_median_s": median(one), "parent_median_s": median(par),
                                      "parent_spread_s": max(par) - min(par), "bar_s": median(par) + max(par) - min(par),
                                      "within_bar": median(one) <= median(par) + max(par) - min(par)}
    except StepFailed as e:
        res["failed"] = e.args[0]
        res["legs_done"] = runs
    for d in list(modes) + ["w_budget", "g_budget"]:
        subprocess.run(["rm", "-rf", os.path.join(ev_dir, d)], check=False)
    os.remove(path)
    return res


def compress_legs(tag, legs, parent, ev_dir, limit):
    path, n = write_shape(tag, ev_dir)
    res = {"copies": n, "eventalign_GB": os.path.getsize(path) / 1e9, "legs": legs}
    runs = {"plain": [], "compress": [], "compress2": []}
    one, par, par_gz = [], [], []
    env = dict(os.environ, M6A_EVENTALIGN_TIMES="1")
    try:
        for leg in range(legs):
            for mode, flag in (("plain", []), ("compress", ["--compress"]), ("compress2", ["--compress", "--compress_level", "2"])):
                cmd = ["eventalign_inference", "--eventalign", path, "--out_dir", os.path.join(ev_dir, mode), "--csv", "device"] + flag + THREADS
                s, p = timed(cmd, limit, env=env)
                must(s, p, "--csv device " + mode)
                t = json.loads(p.stdout.split("M6A_TIMES ", 1)[1].splitlines()[0])
                t["s"] = s
                runs[mode].append(t)
            same = []
            for mode in ("compress", "compress2"):
                for f in CSVS:                              # the text inside the .gz files is the plain leg's file
                    z = subprocess.Popen(["gzip", "-dc", os.path.join(ev_dir, mode, f + ".gz")], stdout=subprocess.PIPE)
                    c = subprocess.run(["cmp", "-s", "-", os.path.join(ev_dir, "plain", f)], stdin=z.stdout)
                    z.stdout.close()
                    same.append(z.wait() == 0 and c.returncode == 0 and not os.path.exists(os.path.join(ev_dir, mode, f)))
            res["gunzipped_identical"] = all(same)
            if parent:
                cmd = ["eventalign_inference", "--eventalign", path, "--out_dir", os.path.join(ev_dir, "one")] + THREADS
                one.append(must(*timed(cmd, limit), "default command, this tree"))
                cmd[4] = os.path.join(ev_dir, "one_parent")
                par.append(must(*timed(cmd, limit, tree=parent), "default command, parent tree"))
                cmd = ["eventalign_inference", "--eventalign", path, "--out_dir", os.path.join(ev_dir, "gz_parent"), "--csv", "device",
                       "--compress"] + THREADS                # level 1 is held to the parent's --compress leg of the same session
                par_gz.append(must(*timed(cmd, limit, tree=parent), "--csv device --compress, parent tree"))
                res["one_file_csvs_identical"] = all(filecmp.cmp(os.path.join(ev_dir, "one", f), os.path.join(ev_dir, "one_parent", f),
                                                                 shallow=False) for f in CSVS)
            for d in ("plain", "compress", "compress2", "one", "one_parent", "gz_parent"):
                subprocess.run(["rm", "-rf", os.path.join(ev_dir, d)], check=False)
            print("%s: leg %d of %d: --csv device %.2f s, with --compress %.2f s, with --compress_level 2 %.2f s" % (
                tag, leg + 1, legs, runs["plain"][-1]["s"], runs["compress"][-1]["s"], runs["compress2"][-1]["s"]), file=sys.stderr, flush=True)
        for mode in runs:
            v = runs[mode]
            res[mode] = {"median_s": median([x["s"] for x in v]), "d2h_bytes_per_read": v[-1]["d2h_bytes"] / v[-1]["n_reads"],
                         "csv_write_ms": median([x["ms"]["csv_write"] for x in v]), "csv_format_ms": median([x["ms"]["csv_format"] for x in v]),
                         "csv_copy_ms": median([x["ms"]["csv_copy"] for x in v]), "csv_pwrite_ms": median([x["ms"]["csv_pwrite"] for x in v]),
                         "csv_text_bytes": v[-1]["csv_text_bytes"], "peak_bytes": v[-1]["peak_bytes"], "legs": v}
        for mode in ("compress", "compress2"):
            c = res[mode]
            c["csv_deflate_ms"] = median([x["ms"]["csv_deflate"] for x in runs[mode]])
            c["csv_compressed_bytes"] = runs[mode][-1]["csv_compressed_bytes"]
            c["csv_stored_blocks"] = runs[mode][-1]["csv_stored_blocks"]
            c["compressed_over_text"] = c["csv_compressed_bytes"] / c["csv_text_bytes"]
            c["deflate_GBps_of_text"] = c["csv_text_bytes"] / (c["csv_deflate_ms"] * 1e6) if c["csv_deflate_ms"] else None
        res["compress2"]["csv_dynamic_blocks"] = runs["compress2"][-1]["csv_dynamic_blocks"]
        res["compress2"]["csv_fixed_blocks"] = runs["compress2"][-1]["csv_fixed_blocks"]
        res["level_2_over_level_1"] = {"csv_deflate_ms": res["compress2"]["csv_deflate_ms"] / res["compress"]["csv_deflate_ms"],
                                       "bytes": res["compress2"]["csv_compressed_bytes"] / res["compress"]["csv_compressed_bytes"],
                                       "median_s": res["compress2"]["median_s"] / res["compress"]["median_s"]}
        c = res["compress"]
        res["compress_over_plain_time"] = c["median_s"] / res["plain"]["median_s"]
        res["compress_is"] = "faster" if c["median_s"] < res["plain"]["median_s"] else "slower"
        if parent:
            res["default_command"] = {"this_s": one, "parent_s": par, "this_median_s": median(one), "parent_median_s": median(par),
                                      "parent_spread_s": max(par) - min(par), "bar_s": median(par) + max(par) - min(par),
                                      "within_bar": median(one) <= median(par) + max(par) - min(par)}
            res["compress_command"] = {"this_median_s": c["median_s"], "parent_s": par_gz, "parent_median_s": median(par_gz),
                                       "parent_spread_s": max(par_gz) - min(par_gz), "bar_s": median(par_gz) + max(par_gz) - min(par_gz),
                                       "within_bar": c["median_s"] <= median(par_gz) + max(par_gz) - min(par_gz)}
    except StepFailed as e:
        res["failed"] = e.args[0]
        res["legs_done"] = runs
    os.remove(path)
    return res


def replicates(tag, K, legs, parent, with_copy_rate, ev_dir, limit):
    path, n = write_shape(tag, ev_dir)
    res = {"copies": n, "eventalign_GB": os.path.getsize(path) / 1e9, "replicates": K, "legs": legs}
    two, fused, one, par = [], [], [], []
    times_env = dict(os.environ, M6A_EVENTALIGN_TIMES="1")
    try:
        for leg in range(legs):
            dirs = [os.path.join(ev_dir, "prep_%d" % k) for k in range(K)]
            s = sum(must(*timed(["dataprep", "--eventalign", path, "--out_dir", d] + THREADS, limit), "dataprep") for d in dirs)
            s2 = must(*timed(["inference", "--input_dir"] + dirs + ["--out_dir", os.path.join(ev_dir, "two")] + THREADS, limit), "inference")
            two.append({"s": s + s2, "dataprep_s": s, "inference_s": s2})
            s3, p3 = timed(["eventalign_inference", "--eventalign"] + [path] * K + ["--out_dir", os.path.join(ev_dir, "fused")] + THREADS, limit,
                           env=times_env)
            must(s3, p3, "fused")
            t = json.loads(p3.stdout.split("M6A_TIMES ", 1)[1].splitlines()[0])
            t["s"] = s3
            fused.append(t)
            res["csvs_identical"] = all(filecmp.cmp(os.path.join(ev_dir, "two", f), os.path.join(ev_dir, "fused", f), shallow=False) for f in CSVS)
            if parent:
                cmd = ["eventalign_inference", "--eventalign", path, "--out_dir", os.path.join(ev_dir, "one")] + THREADS
                one.append(must(*timed(cmd, limit), "one file, this tree"))
                cmd[4] = os.path.join(ev_dir, "one_parent")
                par.append(must(*timed(cmd, limit, tree=parent), "one file, parent tree"))
                res["one_file_csvs_identical"] = all(filecmp.cmp(os.path.join(ev_dir, "one", f), os.path.join(ev_dir, "one_parent", f),
                                                                 shallow=False) for f in CSVS)
            for d in dirs + [os.path.join(ev_dir, x) for x in ("two", "fused", "one", "one_parent")]:
                subprocess.run(["rm", "-rf", d], check=False)
        res["two_step"] = {"median_s": median([x["s"] for x in two]), "legs": two}
        res["fused"] = {"median_s": median([x["s"] for x in fused]), "legs": fused}
        res["fused_over_two_step_speed"] = res["two_step"]["median_s"] / res["fused"]["median_s"]
        if parent:
            res["one_file"] = {"this_s": one, "parent_s": par, "this_median_s": median(one), "parent_median_s": median(par),
                               "parent_spread_s": max(par) - min(par), "bar_s": median(par) + max(par) - min(par),
                               "within_bar": median(one) <= median(par) + max(par) - min(par)}
        if with_copy_rate:
            res["pooled_copy"] = copy_rate(path, K, ev_dir, limit)
    except StepFailed as e:
        res["failed"] = e.args[0]
    os.remove(path)
    return res


def shape(tag, ev_dir, limit):
    path, n = write_shape(tag, ev_dir)
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
    if "--bgzf" in sys.argv:
        shapes = sys.argv[sys.argv.index("--shapes") + 1].split(",") if "--shapes" in sys.argv else ["3.1GB", "24.3GB"]
        dest = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(REPO, "profiles", "r11_eventalign_bgzf.json")
        legs = int(sys.argv[sys.argv.index("--legs") + 1]) if "--legs" in sys.argv else 5
        parent = os.path.abspath(sys.argv[sys.argv.index("--parent_tree") + 1]) if "--parent_tree" in sys.argv else None
        if os.path.exists(dest):                            # one shape per call is allowed: the shapes share the file
            res = json.load(open(dest))
        with tempfile.TemporaryDirectory(dir=os.environ.get("M6A_MEASURE_TMP")) as d:
            for tag in shapes:
                res[tag] = bgzf_legs(tag, legs, parent, d, limit)
                print(json.dumps({tag: res[tag]}), flush=True)
                os.makedirs(os.path.dirname(dest), exist_ok=True)
                with open(dest, "w") as f:                  # after every shape: a later failure keeps what was measured
                    json.dump(res, f, indent=1)
                if "failed" in res[tag]:
                    break                                   # a failed step: nothing more is started
        return
    if "--grouped" in sys.argv:
        shapes = sys.argv[sys.argv.index("--shapes") + 1].split(",") if "--shapes" in sys.argv else ["3.1GB"]
        dest = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(REPO, "profiles", "r30_grouped_input.json")
        legs = int(sys.argv[sys.argv.index("--legs") + 1]) if "--legs" in sys.argv else 5
        window_mb = int(sys.argv[sys.argv.index("--window_mb") + 1]) if "--window_mb" in sys.argv else 256
        group_kbs = [int(x) for x in (sys.argv[sys.argv.index("--group_kb") + 1] if "--group_kb" in sys.argv else "65536,262144,1048576").split(",")]
        parent = os.path.abspath(sys.argv[sys.argv.index("--parent_tree") + 1]) if "--parent_tree" in sys.argv else None
        if os.path.exists(dest):                            # one shape per call is allowed: the shapes share the file
            res = json.load(open(dest))
        with tempfile.TemporaryDirectory(dir=os.environ.get("M6A_MEASURE_TMP")) as d:
            for tag in shapes:
                res[tag] = grouped_legs(tag, legs, window_mb, group_kbs, parent, d, limit)
                print(json.dumps({tag: res[tag]}), flush=True)
                os.makedirs(os.path.dirname(dest), exist_ok=True)
                with open(dest, "w") as f:                  # after every shape: a later failure keeps what was measured
                    json.dump(res, f, indent=1)
                if "failed" in res[tag]:
                    break                                   # a failed step: nothing more is started
        return
    if "--stream" in sys.argv:
        shapes = sys.argv[sys.argv.index("--shapes") + 1].split(",") if "--shapes" in sys.argv else ["3.1GB"]
        dest = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(REPO, "profiles", "r16_stream_input.json")
        legs = int(sys.argv[sys.argv.index("--legs") + 1]) if "--legs" in sys.argv else 5
        window_mb = int(sys.argv[sys.argv.index("--window_mb") + 1]) if "--window_mb" in sys.argv else 256
        parent = os.path.abspath(sys.argv[sys.argv.index("--parent_tree") + 1]) if "--parent_tree" in sys.argv else None
        if os.path.exists(dest):                            # one shape per call is allowed: the shapes share the file
            res = json.load(open(dest))
        with tempfile.TemporaryDirectory(dir=os.environ.get("M6A_MEASURE_TMP")) as d:
            for tag in shapes:
                res[tag] = stream_legs(tag, legs, window_mb, parent, d, limit)
                print(json.dumps({tag: res[tag]}), flush=True)
                os.makedirs(os.path.dirname(dest), exist_ok=True)
                with open(dest, "w") as f:                  # after every shape: a later failure keeps what was measured
                    json.dump(res, f, indent=1)
                if "failed" in res[tag]:
                    break                                   # a failed step: nothing more is started
        return
    if "--read_names" in sys.argv:
        shapes = sys.argv[sys.argv.index("--shapes") + 1].split(",") if "--shapes" in sys.argv else ["3.1GB"]
        dest = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(REPO, "profiles", "r15_read_names.json")
        legs = int(sys.argv[sys.argv.index("--legs") + 1]) if "--legs" in sys.argv else 5
        parent = os.path.abspath(sys.argv[sys.argv.index("--parent_tree") + 1]) if "--parent_tree" in sys.argv else None
        if os.path.exists(dest):                            # one shape per call is allowed: the shapes share the file
            res = json.load(open(dest))
        with tempfile.TemporaryDirectory(dir=os.environ.get("M6A_MEASURE_TMP")) as d:
            for tag in shapes:
                res[tag] = read_names_legs(tag, legs, parent, d, limit)
                print(json.dumps({tag: res[tag]}), flush=True)
                os.makedirs(os.path.dirname(dest), exist_ok=True)
                with open(dest, "w") as f:                  # after every shape: a later failure keeps what was measured
                    json.dump(res, f, indent=1)
                if "failed" in res[tag]:
                    break                                   # a failed step: nothing more is started
        return
    if "--compress" in sys.argv:
        shapes = sys.argv[sys.argv.index("--shapes") + 1].split(",") if "--shapes" in sys.argv else ["3.1GB", "24.3GB"]
        dest = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(REPO, "profiles", "r13_csv_bgzf_dynamic.json")
        legs = int(sys.argv[sys.argv.index("--legs") + 1]) if "--legs" in sys.argv else 5
        parent = os.path.abspath(sys.argv[sys.argv.index("--parent_tree") + 1]) if "--parent_tree" in sys.argv else None
        if os.path.exists(dest):                            # one shape per call is allowed: the shapes share the file
            res = json.load(open(dest))
        with tempfile.TemporaryDirectory(dir=os.environ.get("M6A_MEASURE_TMP")) as d:
            for tag in shapes:
                res[tag] = compress_legs(tag, legs, parent, d, limit)
                print(json.dumps({tag: res[tag]}), flush=True)
                os.makedirs(os.path.dirname(dest), exist_ok=True)
                with open(dest, "w") as f:                  # after every shape: a later failure keeps what was measured
                    json.dump(res, f, indent=1)
                if "failed" in res[tag]:
                    break                                   # a failed step: nothing more is started
        return
    if "--window_mb" in sys.argv:
        sizes = [int(x) for x in sys.argv[sys.argv.index("--window_mb") + 1].split(",")]
        if 0 not in sizes or len(sizes) < 2 or min(sizes) < 0:
            raise SystemExit("--window_mb 0,N[,N...]: windows are measured against the whole file")
        shapes = sys.argv[sys.argv.index("--shapes") + 1].split(",") if "--shapes" in sys.argv else ["3.1GB", "24.3GB"]
        dest = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(REPO, "profiles", "r10_eventalign_windows.json")
        legs = int(sys.argv[sys.argv.index("--legs") + 1]) if "--legs" in sys.argv else 5
        parent = os.path.abspath(sys.argv[sys.argv.index("--parent_tree") + 1]) if "--parent_tree" in sys.argv else None
        budget = [int(x) for x in sys.argv[sys.argv.index("--budget_mb") + 1].split(",")] if "--budget_mb" in sys.argv else []
        if os.path.exists(dest):                            # one shape per call is allowed: the shapes share the file
            res = json.load(open(dest))
        with tempfile.TemporaryDirectory(dir=os.environ.get("M6A_MEASURE_TMP")) as d:
            for tag in shapes:
                res[tag] = windows(tag, sorted(sizes), legs, parent, budget, d, limit)
                print(json.dumps({tag: res[tag]}), flush=True)
                os.makedirs(os.path.dirname(dest), exist_ok=True)
                with open(dest, "w") as f:                  # after every shape: a later failure keeps what was measured
                    json.dump(res, f, indent=1)
                if "failed" in res[tag]:
                    break                                   # a failed step: nothing more is started
        return
    if "--csv" in sys.argv:
        if sorted(sys.argv[sys.argv.index("--csv") + 1].split(",")) != ["device", "host"]:
            raise SystemExit("--csv host,device: both writers are measured against each other")
        K = int(sys.argv[sys.argv.index("--replicates") + 1]) if "--replicates" in sys.argv else 1
        dest = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(REPO, "profiles", "r09_csv_device.json")
        legs = int(sys.argv[sys.argv.index("--legs") + 1]) if "--legs" in sys.argv else 5
        parent = os.path.abspath(sys.argv[sys.argv.index("--parent_tree") + 1]) if "--parent_tree" in sys.argv else None
        if os.path.exists(dest):                            # the one-file and the replicate run share the file
            res = json.load(open(dest))
        with tempfile.TemporaryDirectory(dir=os.environ.get("M6A_MEASURE_TMP")) as d:
            for tag in shapes:
                key = tag if K == 1 else "%s x %d replicates" % (tag, K)
                res[key] = csv_writers(tag, K, legs, parent, "--copy_rate" in sys.argv, d, limit)
                print(json.dumps({key: res[key]}), flush=True)
                with open(dest, "w") as f:                  # after every shape: a later failure keeps what was measured
                    json.dump(res, f, indent=1)
                if "failed" in res[key]:
                    break                                   # a failed step: nothing more is started
        return
    if "--replicates" in sys.argv:
        K = int(sys.argv[sys.argv.index("--replicates") + 1])
        shapes = sys.argv[sys.argv.index("--shapes") + 1].split(",") if "--shapes" in sys.argv else ["3.1GB"]
        dest = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(REPO, "profiles", "r08_eventalign_replicates.json")
        legs = int(sys.argv[sys.argv.index("--legs") + 1]) if "--legs" in sys.argv else 3
        parent = os.path.abspath(sys.argv[sys.argv.index("--parent_tree") + 1]) if "--parent_tree" in sys.argv else None
        with tempfile.TemporaryDirectory(dir=os.environ.get("M6A_MEASURE_TMP")) as d:
            for tag in shapes:
                res[tag] = replicates(tag, K, legs, parent, "--copy_rate" in sys.argv, d, limit)
                print(json.dumps({tag: res[tag]}), flush=True)
                if "failed" in res[tag]:
                    break                                   # a failed step: nothing more is started
        os.makedirs(os.path.dirname(dest), exist_ok=True)
        with open(dest, "w") as f:
            json.dump(res, f, indent=1)
        return
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
