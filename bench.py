#!/usr/bin/env python3
"""bench.py -- DRACH sites/s of the m6A inference hot path on MI355X.

Workloads
  uniform (default; BASELINE.json configs[2], the config the metric is quoted on): per GPU
      1,000,000 synthetic DRACH sites x 20 reads, HCT116_RNA002 weights, num_iterations=1000.
      With N GPUs: configs[3]'s shape (N x 1M sites, site-sharded).
  ragged (BASELINE.json configs[4], per-GPU shape): per GPU 125,000 sites x 50..500 reads,
      HEK293T_RNA004 weights, num_iterations=1000.
Both: exact NumPy-stream replay (batch_size 16, save_per_batch 2, seed 0).  One step = one pass of the
hot path (read encoder -> site pooling; read_prob, site_prob, mod_ratio all produced) over the rank's
sites, inputs resident in HBM.  With N GPUs every rank holds its own shard of an N-times-larger job
(weak scaling; shards are flush-group aligned and carry the job offset, so the job's results do not
depend on N) and each step ends with ONE gather of site_prob + mod_ratio to rank 0 over RCCL.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--workload uniform|ragged] [--sites S] [--iters T] [--dump-outputs DIR] [--full]

A plain run does what the headline needs and nothing more: it sets up, makes the cold call, warms up, times the K steps (HIP
events around the encoder launches inside them give `roofline`), writes --dump-outputs, and prints the line.  --full adds
everything else the line can carry, each in runs of its own after the timed steps: the pooling kernel's roofline with its
measured ceiling, live rocprofv3 PMC traffic, the sustained leg (--min-seconds, 3 s by default), on the default shape the opt-in
12-slot encoder, host inputs and the `ragged` shape, and the CPU baseline; --no-* options leave parts of it out.  An N-rank run
keeps, either way, what certifies its line: each rank's compute-only steps before the process group, `rccl`, `per_rank`, `efficiency`.

`--gpus N` without a launcher starts its own N ranks (re-executes under torch.distributed.run on
127.0.0.1); under torch.distributed.run (RANK/WORLD_SIZE set) it runs as one rank.  The 8-GPU run is
    python bench.py --gpus 8        (or: python -m torch.distributed.run --nnodes=1 --nproc-per-node 8
                                      --master-addr 127.0.0.1 --master-port 29500 bench.py --gpus 8)
M6A_BENCH_BACKEND=gloo is a debugging aid: ranks may then share one GPU and the gather is staged
through host memory.
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REPO)
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")     # dmabuf IPC for RCCL's P2P set-up (the boxes export it; kept for scrubbed environments)

ENC_FLOP_PER_READ = 14164      # 2*(15*150 + 150*32 + 32)           SURVEY.md section 8(d)
ENC_BYTES_PER_READ = 40        # 9 f32 in + 1 f32 out               SURVEY.md section 8(d)
# what the kernels EXECUTE per read: v_mfma_f32_32x32x2_f32 = 4096 FLOP for a tile of 32 reads; the two 16-slot kernels (auto) issue
# 116 of them per tile (40 layer 1 + 76 layer 2), the opt-in 12-slot kernel 106 (30 + 76) -- padding of 150 hidden units to 160 rows included,
# the 32 -> 1 layer and the embedding fold (VALU) not
ENC_MFMA_PER_TILE = {"enc_csite_kernel": 106, "enc_site16_kernel": 116, "enc_kernel": 116}
PEAK_F32_TFLOPS = 157.3        # MI355X_MICROARCH.md: f32 MFMA = f32 vector peak
PEAK_HBM_GBPS = 8000.0
# ds_read_b32 gathers, conflict-free: 64 lanes per 2 LDS cycles per CU (MI355X_MICROARCH.md, LDS table)
PEAK_LDS_GATHERS = 256 * 2.4e9 * 32

# one multiply per draw; packed f32: 2 per lane per 4-cycle issue slot = the 157.3 TFLOP/s vector peak / 2 flops per FMA
PEAK_VALU_MULS = PEAK_F32_TFLOPS * 1e12 / 2

# --dump-outputs: at most 4 M read probabilities (16 MB) and 3 M sites (12 MB site_prob + 24 MB mod_ratio) are written
DUMP_READS_MAX = 4_000_000
DUMP_SITES_MAX = 3_000_000
DUMP_SEEDS = {"read_prob": 1, "site_prob": 2, "mod_ratio": 2}


def pool_roofline(variant, draws, avg_ms, launches):
    """The pooling kernel against the resource that bounds it: the register kernel of uniform bags issues one
    v_pk_mul_f32 per two draws and no LDS gather at all (VALU issue); every other variant gathers one 4-byte value
    per draw from LDS.  DESIGN.md sections 4.2 / 4.3 (HISTORY.md 4.2r / 4.3 for the derivations) give both and the practical ceilings under them."""
    rate = draws / (avg_ms * 1e-3) if avg_ms else None
    if variant == "table-reg":
        bound, peak = "valu", PEAK_VALU_MULS
        note = ("peak = nominal float32 multiply rate, 32 lanes per SIMD cycle at 2.4 GHz = 78.6 T/s (a wave64 v_mul_f32 in 2 cycles, a "
                "v_pk_mul_f32 in 4: packing buys nothing).  Chain-free streams reach 0.85-0.94 of it (tools/valu_rate_bench, "
                "profiles/r04_valu_rate.json: 2.2-2.4 / 4.2-4.7 cycles; dependent chains and register banks make no difference, random "
                "mantissas cost 3-12 % through the clock).  measured_ceiling, taken live, is the kernel's own draw with nothing around it")
    else:
        bound, peak = "l1-lds", PEAK_LDS_GATHERS
        note = ("a draw moves 2 index bytes through the vector L1 (64 B/clk/CU) and one 4-byte LDS gather (32 banks/clk/CU): both pipes "
                "peak at 19.7 T draws/s; knock-out builds show the index rows are the binding one for the table kernel "
                "(DESIGN.md section 4.3; the preparation kernel runs on a side stream under the encoder and is not in avg_launch_ms)"
                if variant == "ragged-table" else
                "peak = conflict-free ds_read_b32 gather rate (one 4-byte gather per draw)")
    return {"kernel": "site pooling (%s)" % variant, "bound": bound, "achieved": rate / 1e12 if rate else None, "peak": peak / 1e12,
            "unit": "T draws/s", "frac": rate / peak if rate else None, "note": note, "avg_launch_ms": avg_ms, "launches": launches,
            "draws_per_launch": draws}


NOMINAL_GHZ = 2.4


def at_measured_clock(roof, clk):
    """`peak` assumes the 2.4 GHz maximum clock; a kernel that draws enough power makes the part clock lower,
    and `frac` then mixes that with issue loss.  clk = the shader clock the kernel's own waves lived at (s_memtime over
    s_memrealtime, stamped by lane 0 of up to 64 workgroups of the last profiled launch: m6a_profile_clock).  Adds the clock,
    the peak at that clock and the fraction of THAT peak; `peak` / `frac` stay nominal (comparable across rounds)."""
    if not clk or not roof.get("achieved"):
        roof["clock_ghz_measured"] = None
        return roof
    g = clk["ghz"]
    roof["clock_ghz_measured"] = g
    roof["clock_detail"] = dict(clk, nominal_ghz=NOMINAL_GHZ,
                                source="in-kernel: s_memtime / s_memrealtime of %d stamped waves of the last profiled launch "
                                       "(median; span_ms = first start to last end of those waves)" % clk["waves"])
    roof["peak_at_measured_clock"] = roof["peak"] * g / NOMINAL_GHZ
    roof["frac_at_measured_clock"] = roof["achieved"] / roof["peak_at_measured_clock"]
    if "achieved_executed" in roof:
        roof["frac_executed_at_measured_clock"] = roof["achieved_executed"] / roof["peak_at_measured_clock"]
    return roof


WORKLOADS = {
    "uniform": dict(model="HCT116_RNA002", sites=1_000_000, bag=20, config="BASELINE.json configs[2]"),
    "ragged": dict(model="HEK293T_RNA004", sites=125_000, bag=(50, 500), config="BASELINE.json configs[4] per-GPU shape"),
}


def measured_traffic(S, bag):
    """HBM bytes per encoder launch from the committed PMC passes (rocprofv3 --pmc FETCH_SIZE /
    WRITE_SIZE, separate runs; profiles/*_enc_traffic.json), when they were taken on this workload.
    The newest profile wins; the bench line names the file so a stale figure is visible."""
    import glob
    best = None
    for f in sorted(glob.glob(os.path.join(REPO, "profiles", "*_enc_traffic.json"))):
        try:
            d = json.load(open(f))
        except (OSError, ValueError):
            continue
        w = d.get("workload", {})
        if w.get("sites") == S and w.get("reads_per_site") == (list(bag) if isinstance(bag, tuple) else bag):
            best = dict(d, file=os.path.relpath(f, REPO))
    return best


def live_traffic(workload, kernel_name, pool_kernel_name=None, timeout_s=240, enc_variant=0):
    """HBM bytes per encoder launch measured NOW: two short re-runs of this script under
    `rocprofv3 --pmc FETCH_SIZE` / `--pmc WRITE_SIZE` (separate passes, --kernel-trace only, as
    MI355X_MICROARCH.md prescribes), read back from the rocpd database.  FETCH_SIZE x2: gfx950 tallies the 128-byte
    requests of wide streaming reads at 64 bytes.  Returns None when rocprofv3 is unavailable or a pass fails."""
    import glob
    import shutil
    import sqlite3
    import tempfile
    if shutil.which("rocprofv3") is None:
        return None
    vals, pool_vals = {}, {}
    for ctr in ("FETCH_SIZE", "WRITE_SIZE"):
        d = tempfile.mkdtemp(prefix="m6a_pmc_")
        try:
            cmd = ["rocprofv3", "--pmc", ctr, "--kernel-trace", "-d", d, "-o", "pmc", "--", sys.executable, os.path.abspath(__file__),
                   "--workload", workload, "--steps", "3", "--warmup", "1", "--enc-variant", str(enc_variant)]     # a plain run
            subprocess.run(cmd, capture_output=True, timeout=timeout_s, env=dict(os.environ, TMPDIR=os.environ.get("TMPDIR", "/tmp")))
            dbs = glob.glob(os.path.join(d, "**", "*_results.db"), recursive=True)
            if not dbs:
                return None
            con = sqlite3.connect(dbs[0])
            cols = [r[1] for r in con.execute("pragma table_info(counters_collection)")]
            kn = "kernel_name" if "kernel_name" in cols else "name"
            q = "select avg(value), count(*) from counters_collection where counter_name = ? and %s like ?" % kn
            row = con.execute(q, (ctr, kernel_name + "%")).fetchone()
            prow = con.execute(q, (ctr, pool_kernel_name + "%")).fetchone() if pool_kernel_name else None
            con.close()
            if not row or not row[1]:
                return None
            vals[ctr] = float(row[0])
            if prow and prow[1]:
                pool_vals[ctr] = float(prow[0])
        except (subprocess.SubprocessError, OSError, sqlite3.Error):
            return None
        finally:
            shutil.rmtree(d, ignore_errors=True)
    pool = None
    if len(pool_vals) == 2:
        # the pooling kernel's reads are 80-byte bags at a 2.5 KB stride per lane, not wide streams: whether gfx950's x2 applies to
        # them is not established, so both readings are given
        pool = {"kernel": pool_kernel_name, "FETCH_SIZE_KiB": pool_vals["FETCH_SIZE"], "WRITE_SIZE_KiB": pool_vals["WRITE_SIZE"],
                "fetch_bytes_as_counted": pool_vals["FETCH_SIZE"] * 1024.0, "fetch_bytes_with_gfx950_x2": 2048.0 * pool_vals["FETCH_SIZE"]}
    return {"traffic_bytes_per_launch": (2.0 * vals["FETCH_SIZE"] + vals["WRITE_SIZE"]) * 1024.0, "pool": pool,
            "source": "measured by this run: rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes over 4 launches of %s "
                      "(FETCH_SIZE %.0f KiB x2 gfx950 correction + WRITE_SIZE %.0f KiB)" % (kernel_name, vals["FETCH_SIZE"], vals["WRITE_SIZE"])}


# ---------------------------------------------------------------------------------------------
# CPU baseline (runs in its own process: it forks worker pools, which must not happen after HIP is up)
# ---------------------------------------------------------------------------------------------
def _pool_site_worker(job):
    """One site of a flush group, as a Pool task (the reference's imap over sites, inference_utils.py:103-104)."""
    from oracle import m6a_oracle as orc
    p, T, thr = job
    off = np.array([0, len(p)], np.int64)
    site, _ = orc.site_pool(p, off, T, thr, batch_size=1, save_per_batch=1)
    return float(site[0])


def host_cpu_facts():
    """What this process may actually use of the host: logical CPUs, the scheduler affinity mask, the cgroup CPU quota
    (v2 cpu.max, v1 cfs_quota_us / cfs_period_us), physical cores, and how busy the host already is."""
    logical = os.cpu_count() or 1
    try:
        affinity = len(os.sched_getaffinity(0))
    except (AttributeError, OSError):
        affinity = logical
    quota = None
    try:
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if q != "max":
            quota = float(q) / float(per)
    except (OSError, ValueError):
        try:
            q = float(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read())
            per = float(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
            if q > 0:
                quota = q / per
        except (OSError, ValueError):
            pass
    model, phys, cur = "unknown", set(), [None, None]
    try:
        for line in open("/proc/cpuinfo"):
            k, _, v = line.partition(":")
            k, v = k.strip(), v.strip()
            if k == "model name" and model == "unknown":
                model = v
            elif k == "physical id":
                cur[0] = v
            elif k == "core id":
                cur[1] = v
                phys.add(tuple(cur))
    except OSError:
        pass
    try:
        load = [float(x) for x in open("/proc/loadavg").read().split()[:3]]
    except (OSError, ValueError):
        load = None
    eff = affinity if quota is None else max(1, min(affinity, int(quota + 0.5)))
    return {"cpu_model": model, "logical_cpus": logical, "physical_cores": len(phys) or None, "affinity_cpus": affinity,
            "cgroup_cpu_quota": quota, "effective_cores": eff, "loadavg_1_5_15_before": load}


def cpu_calibration():
    """tests/golden/calibrate_cpu_baseline.py (build container, imports the reference): oracle vs the reference's own NumPy / torch
    code on the same inputs, one thread.  BASELINE.md section 3: the port stands for the reference within +-10 % or this factor."""
    path = os.path.join(REPO, "profiles", "r06_cpu_calibration.json")
    try:
        with open(path) as f:
            c = json.load(f)
        return {"file": "profiles/r06_cpu_calibration.json", "oracle_over_reference": c["oracle_over_reference"],
                "measured_on": c.get("host"), "note": c.get("note")}
    except (OSError, ValueError, KeyError):
        return None


def cpu_baseline_main(workload, T, budget_s):
    """The oracle (a port of the reference's algorithm, oracle/m6a_oracle.c) on this host's cores, on a
    bounded sample of the bench workload.  Three figures, as BASELINE.md section 3 asks:
      reference_shaped  the loop `m6anet inference` runs: encoder per 16-site batch, then per flush group
                        of <= 32 sites a NEW multiprocessing.Pool(n) and one task per site
                        (inference_utils.py:33-54,102-104), at n = 1, 25 (the reference's default) and all cores;
      best_case         the same arithmetic with one persistent set of threads over all sites (what the
                        reference could do at best) -- `value`, the figure most favourable to the CPU;
      single_thread     one thread in-process.
    `cores` = the threads the best case ran on = the CPUs this process may really use (affinity mask and cgroup
    quota, not os.cpu_count()); `scaling` = the same job at 1, 2, 4, ... threads with the efficiency of each point, so a
    host that is shared or throttled shows up in the line instead of in the ratio."""
    import multiprocessing as mp
    from m6anet_amd import synthetic
    from m6anet_amd.constants import DEFAULT_READ_THRESHOLD
    from m6anet_amd.engine import load_weights
    from oracle import m6a_oracle as orc
    orc.build()
    spec = WORKLOADS[workload]
    facts = host_cpu_facts()
    cores = facts["effective_cores"]
    thr = np.float32(DEFAULT_READ_THRESHOLD)
    weights = load_weights(spec["model"])
    n_sample = 600_000 if workload == "uniform" else 60_000
    d = synthetic.make_sites(n_sample, spec["bag"], seed=20250328)
    S = n_sample

    def run(n, threads):
        off = d["off"][:n + 1]
        t0 = time.perf_counter()
        p = orc.encode_reads(weights, d["X"][:off[-1]], d["site_kmers"][:n], off, n_threads=threads)
        orc.site_pool(p, off, T, thr, n_threads=threads)
        return time.perf_counter() - t0

    # (iii) one thread in-process
    n1 = 512 if workload == "uniform" else 64
    run(32, 1)
    t1 = run(n1, 1)
    single = n1 / t1
    # the scaling curve: every thread count gets the same sites PER THREAD (whole flush groups), ~0.5 s each
    per_thread = max(32, int(single * 0.5) // 32 * 32)
    curve, th = [], 1
    counts = []
    while th < cores:
        counts.append(th)
        th *= 2
    counts.append(cores)
    for th in counts:
        n = min(S - S % 32, per_thread * th)
        t = run(n, th)
        curve.append({"threads": th, "sites": n, "sites_per_s": n / t, "efficiency": n / t / (th * single)})
    # (ii) persistent threads over all sites, the bounded sample sized from the curve's last point
    rate = curve[-1]["sites_per_s"]
    n = int(min(S, max(32 * cores, rate * budget_s * 0.5)))
    n -= n % 32
    n = max(n, min(S, 32))
    t = run(n, cores)
    best = n / t

    # (i) reference-shaped: per batch of 16 sites the encoder, per flush group a fresh Pool
    def ref_shaped(n_proc, n_groups):
        ctx = mp.get_context("fork")
        bs, gsz = 16, 32
        done = 0
        t0 = time.perf_counter()
        for g in range(n_groups):
            a, b = g * gsz, min(S, (g + 1) * gsz)
            probs = []
            for s0 in range(a, b, bs):
                s1 = min(b, s0 + bs)
                off = d["off"][s0:s1 + 1] - d["off"][s0]
                p = orc.encode_reads(weights, d["X"][d["off"][s0]:d["off"][s1]], d["site_kmers"][s0:s1], off)
                probs.extend(p[off[i]:off[i + 1]] for i in range(s1 - s0))
            with ctx.Pool(n_proc) as pool:
                list(pool.imap(_pool_site_worker, [(p, T, thr) for p in probs]))
            done += b - a
        return done / (time.perf_counter() - t0)

    shaped = {}
    for n_proc, groups in ((1, 12), (25, 8), (facts["logical_cpus"], 3)):
        if n_proc > facts["logical_cpus"]:
            continue
        shaped["n_processes=%d" % n_proc] = ref_shaped(n_proc, groups)
    try:
        facts["loadavg_1_5_15_after"] = [float(x) for x in open("/proc/loadavg").read().split()[:3]]
    except (OSError, ValueError):
        pass
    out = {"value": best, "unit": "sites/s", "cores": cores, "kind": "port", "cpu_model": facts["cpu_model"],
           "effective_cores": cores, "host": facts,
           "per_core_value": best / cores, "single_thread_value": single,
           "scaling_efficiency": best / (cores * single), "scaling": curve,
           "reference_shaped_value": shaped,
           "sample": "first %d sites of the same workload (encoder + T=%d sampling) on %d host threads, %.1f s; "
                     "single thread: %d sites; scaling curve: %d sites per thread at %s threads; reference-shaped "
                     "(fresh Pool per 32-site flush): 3-12 flush groups per setting"
                     % (n, T, cores, t, n1, per_thread, "/".join(str(c) for c in counts))}
    cal = cpu_calibration()
    if cal:
        out["calibration"] = cal
        # what the REFERENCE's own code would do on this host, by the calibration factor (oracle speed / reference speed)
        out["reference_equivalent_value"] = best / cal["oracle_over_reference"]["whole_path"]
    return out


def run_cpu_baseline_subprocess(workload, T):
    cmd = [sys.executable, os.path.abspath(__file__), "--cpu-baseline-only", "--workload", workload, "--iters", str(T)]
    try:
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=dict(os.environ, HIP_VISIBLE_DEVICES=""))
        for line in reversed(out.stdout.strip().splitlines()):
            if line.startswith("{"):
                return json.loads(line)
        return {"error": (out.stderr or out.stdout)[-400:]}
    except (subprocess.SubprocessError, OSError, ValueError) as e:
        return {"error": repr(e)}


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def measured_gather_ceiling(bag):
    """The random-gather ceiling of a one-gather-per-draw pooling kernel on THIS box, measured now: tools/rg_probe
    (tools/ragged_gather_probe.hip, built by __graft_entry__.build()) times nothing but ds_read_b32 gathers at random
    indices of an n-entry LDS bag plus the multiplies, 8 waves per SIMD, for a ladder of n.  Every site draws T*K
    times whatever its bag size, so the ceiling over a mix of sizes is the harmonic mean of the per-size rates."""
    exe = os.path.join(REPO, "tools", "rg_probe")
    if not os.path.exists(exe):
        return None
    try:
        out = subprocess.run([exe], capture_output=True, text=True, timeout=120).stdout
    except (subprocess.SubprocessError, OSError):
        return None
    pts = []
    for line in out.splitlines():
        f = line.split()
        if line.startswith("ds_read_b32") and "gathers/s" in line:
            try:
                n = int(line.split("n=")[1].split()[0])
                pts.append((n, float(f[f.index("T") - 1]) * 1e12))
            except (ValueError, IndexError):
                pass
    if len(pts) < 2:
        return None
    pts.sort()
    lo, hi = (bag, bag) if not isinstance(bag, tuple) else bag
    ns = np.arange(lo, hi + 1)
    inv = np.interp(ns, [p[0] for p in pts], [1.0 / p[1] for p in pts])
    return {"rate": float(1.0 / inv.mean()), "points": {str(n): r / 1e12 for n, r in pts},
            "source": "tools/rg_probe run by this bench (random ds_read_b32 gathers from an n-entry LDS bag, 8 waves/SIMD; "
                      "harmonic mean over bag sizes %d..%d)" % (lo, hi)}


def measured_multiply_ceiling():
    """What float32 multiplies cost on THIS box, measured now by tools/valu_rate_bench --ceiling (chain-free streams with
    random mantissas, events over ~1 ms kernels): the plain and the packed multiply at 2 and 8 waves per SIMD, and
    pool_reg_kernel's own draw -- two indexed v_pk_mul_f32 behind ONE scalar instruction that writes the draw's M0 (rounds 1-4: a
    shift and an index switch), 256-register single-wave workgroups, 2 waves per SIMD -- with nothing else around it.  `rate` = the last one: what the kernel's instruction
    stream can reach; the chain-free rows say what the datapath delivers (profiles/r04_valu_rate.json has every variant)."""
    exe = os.path.join(REPO, "tools", "valu_rate_bench")
    if not os.path.exists(exe):
        return None
    try:
        out = subprocess.run([exe, "--ceiling"], capture_output=True, text=True, timeout=120).stdout
        rows = json.loads(out)["rows"]
    except (subprocess.SubprocessError, OSError, ValueError, KeyError):
        return None
    table = {"%s @ %d waves/SIMD" % (" ".join(r["variant"].split()), r["waves_per_simd"]): r["T_lane_ops_per_s"] for r in rows}
    like = [r for r in rows if "M0 write" in r["variant"]] or [r for r in rows if "2 SALU" in r["variant"]]
    if not like:
        return None
    return {"rate": like[0]["T_lane_ops_per_s"] * 1e12, "variant": like[0]["variant"], "rows": table,
            "source": "tools/valu_rate_bench --ceiling run by this bench: pool_reg_kernel's draw (%s; two indexed v_pk_mul_f32, random "
                      "mantissas, 2 waves per SIMD) with nothing else around it" % like[0]["variant"]}


def smi_snapshot():
    """Clock and power as rocm-smi reports them right now (None if the tool is missing)."""
    try:
        o = subprocess.run(["rocm-smi", "--showclocks", "--showpower", "--json"], capture_output=True, text=True, timeout=20).stdout
        d = json.loads(o)
        card = d.get("card0") or next(iter(d.values()))
        keep = {k: v for k, v in card.items() if any(t in k.lower() for t in ("sclk", "mclk", "power"))}
        return keep or card
    except Exception as e:                                   # noqa: BLE001 -- a diagnostic, never fatal
        return {"error": repr(e)[:200]}


def with_h2d(b, T, steps=5):
    """The same workload with its inputs in HOST memory and its results wanted there (the reference's seam:
    m6anet/utils/inference_utils.py:35-36 moves every batch `.to(device)`; SURVEY.md section 8(e) last sentence): one
    m6a_infer per step on host pointers -- the library's chunked pinned ring, H2D of chunk k+1 under the encoder of chunk k,
    read probabilities flowing back the same way -- from pageable NumPy arrays and from pinned (hipHostMalloc) tensors.
    Outside the headline's timed region; never `value`."""
    import torch
    eng = b.eng
    X, km, off = b.X.cpu().numpy(), b.km.cpu().numpy(), b.off_host
    out = (np.empty(b.R, np.float32), np.empty(b.Sr, np.float32), np.empty(b.Sr, np.float64))
    res = {"steps": steps, "bytes_in_per_step": int(X.nbytes + km.nbytes + off.nbytes), "bytes_out_per_step": int(sum(o.nbytes for o in out)),
           "note": "m6a_infer on host pointers, read_prob + site_prob + mod_ratio returned to host arrays that are reused across steps; "
                   "each step synchronous (the call returns with the results in place); sites/s = sites / median step; pageable arrays go "
                   "through the library's pinned ring (copy threads + DMA), page-locked ones are DMA'd in place"}
    eng.set_stream(None)
    try:
        eng.prepare_host_io()

        def rate(args, outs):
            for _ in range(2):
                eng.infer(*args, T, 20, b.thr, 0, 16, 2, out=outs)              # ring set up, pages touched, fresh pinned pages mapped
            ts = []
            for _ in range(steps):
                t0 = time.perf_counter()
                eng.infer(*args, T, 20, b.thr, 0, 16, 2, out=outs)
                ts.append(time.perf_counter() - t0)
            med = sorted(ts)[len(ts) // 2]
            return {"sites_per_s": b.Sr / med, "ms_per_step": med * 1e3, "best_ms": min(ts) * 1e3, "ms_of_each_step": [t * 1e3 for t in ts],
                    "GBps_in_plus_out": (res["bytes_in_per_step"] + res["bytes_out_per_step"]) / med / 1e9}
        res["pageable"] = rate((X, km, off), out)
        pin = [torch.from_numpy(a).pin_memory() for a in (X, km, off)]
        pout = tuple(torch.empty(o.shape, dtype=getattr(torch, str(o.dtype))).pin_memory() for o in out)
        res["pinned"] = rate(tuple(pin), pout)
        res["encoder_kernel"] = eng.last_encoder_kernel
    except Exception as e:                                  # noqa: BLE001 -- an optional leg: the line goes out without it
        res["error"] = "%s: %s" % (type(e).__name__, str(e)[:200])
    finally:
        eng.use_torch_stream()
    return res


class Bench:
    """One workload on this rank: data resident in HBM, engine, the step, and the timed regions."""

    def __init__(self, args, workload, S, bag, T, rank, world, local_rank, dev, backend):
        import torch
        from m6anet_amd import synthetic
        from m6anet_amd.constants import DEFAULT_READ_THRESHOLD
        from m6anet_amd.engine import M6ANetEngine, load_weights, shard_plan
        self.torch, self.args, self.workload = torch, args, workload
        self.S, self.bag, self.T, self.rank, self.world, self.dev, self.backend = S, bag, T, rank, world, dev, backend
        self.spec = WORKLOADS[workload]
        self.thr = np.float32(DEFAULT_READ_THRESHOLD)
        self.weights = load_weights(self.spec["model"])
        # this rank's shard of the world*S-site job: flush-group-aligned cut of the global site range, balanced by reads
        self.n_reads_job = synthetic.bag_sizes(world * S, bag)
        self.off_job = np.zeros(world * S + 1, np.int64)
        np.cumsum(self.n_reads_job, out=self.off_job[1:])
        self.cuts = shard_plan(self.off_job, world)
        a, b = int(self.cuts[rank]), int(self.cuts[rank + 1])
        d = synthetic.make_sites(b - a, seed=20250328 + rank, n_reads=self.n_reads_job[a:b])
        self.X = torch.from_numpy(d["X"]).to(dev)
        self.km = torch.from_numpy(d["site_kmers"]).to(dev)
        self.off = torch.from_numpy(d["off"]).to(dev)
        self.Sr, self.R = b - a, int(d["off"][-1])
        self.off_host = np.ascontiguousarray(d["off"], dtype=np.int64)
        self.host_offsets = os.environ.get("M6A_BENCH_HOST_OFFSETS", "1") != "0"
        t0 = time.perf_counter()
        eng = M6ANetEngine(weights=self.weights, device=local_rank)
        t1 = time.perf_counter()
        if args.enc_variant:
            eng.set_encoder_variant(args.enc_variant)
        if args.scan_driver:
            eng.set_scan_driver(args.scan_driver)
        eng.use_torch_stream()                               # the first entry point that waits for m6a_create's background set-up
        # what the context costs before the first call (first_call_ms does NOT include it: the set-up runs beside whatever the
        # caller does after m6a_create -- here nothing, so the wait is its whole length)
        self.context_ms = {"m6a_create": (t1 - t0) * 1e3, "wait_for_background_setup": (time.perf_counter() - t1) * 1e3}
        eng.set_job_offset(a)
        self.eng = eng
        self.rp = torch.empty(self.R, dtype=torch.float32, device=dev)
        self.site = torch.empty(self.Sr, dtype=torch.float32, device=dev)
        self.mod = torch.empty(self.Sr, dtype=torch.float64, device=dev)
        self.gather = None
        self.dist = None
        self.gather_kind = "none"

    def compute(self):
        # the loader's host copy of the CSR offsets rides along (every step: its statistics are recomputed from it on
        # the host, the device array is checked against them on the GPU), so the call has nothing to read back and the
        # steps queue back to back; M6A_BENCH_HOST_OFFSETS=0: the library reads the statistics back itself (one stream
        # sync per step)
        if self.host_offsets:
            self.eng.set_host_offsets(self.off_host)
        self.eng.infer(self.X, self.km, self.off, self.T, 20, self.thr, 0, 16, 2, out=(self.rp, self.site, self.mod))

    def step(self):
        self.compute()
        if self.gather is not None:
            if self.backend == "nccl":
                self.gather.start(self.site, self.mod)
            else:
                self.eng.sync()
                self.gather.start(self.site.cpu(), self.mod.cpu())

    def fence(self):
        if self.gather is not None:
            self.gather.drain()          # every gather issued so far has completed
        self.torch.cuda.synchronize(self.dev)
        if self.dist is not None:
            self.dist.barrier()
            self.torch.cuda.synchronize(self.dev)

    def timed(self, n):
        self.fence()
        t0 = time.perf_counter()
        for _ in range(n):
            self.step()
        if self.dist is not None:
            # this rank's OWN time: its compute and its exchanges done, before it waits for anybody at the barrier
            # (rank 0's includes the arrival of every shard: it is the receiving end of the gather)
            if self.gather is not None:
                self.gather.drain()
            self.torch.cuda.synchronize(self.dev)
            self.own_dt = time.perf_counter() - t0
        self.fence()
        return time.perf_counter() - t0

    def max_over_ranks(self, *vals):
        if self.dist is None:
            return vals
        t = self.torch.tensor(list(vals), dtype=self.torch.float64, device=self.dev if self.backend == "nccl" else "cpu")
        self.dist.all_reduce(t, op=self.dist.ReduceOp.MAX)
        return tuple(float(x) for x in t.tolist())

    # the job's one exchange: site_prob + mod_ratio to rank 0, once per step, issued async and double-buffered so the
    # exchange of step i overlaps the compute of step i+1.  Default: the C ABI's own RCCL communicator (m6a_gather, one
    # grouped send/recv over xGMI); if the library cannot bind RCCL, or its self-test fails, torch.distributed's gather.
    def setup_exchange(self, dist, mdist):
        self.dist = dist
        want = os.environ.get("M6A_BENCH_GATHER", "native")
        why = None
        if self.backend != "nccl":
            self.gather = mdist.SiteGather(self.cuts, "cpu", dst=0)
            self.gather_kind = self.backend
            return
        if want == "native":
            # NativeGather's constructor and self-test are collective and end with the same verdict on every rank
            try:
                g = mdist.NativeGather(self.eng, self.cuts, self.dev, dst=0)
                why = g.self_test()
                if why is None:
                    self.gather, self.gather_kind = g, "RCCL (m6a_gather: the C ABI's own communicator, one grouped send/recv)"
                    return
            except Exception as e:                           # noqa: BLE001 -- any failure here means: fall back
                why = "%s: %s" % (type(e).__name__, str(e)[:200])
            if self.rank == 0:
                print("bench: native m6a_gather not usable (%s); falling back to torch.distributed's gather" % why, file=sys.stderr)
        self.gather = mdist.SiteGather(self.cuts, self.dev, dst=0)
        self.gather_kind = "RCCL (torch.distributed)" + ("; native m6a_gather unavailable -- %s" % why if why else "")

    def run(self, steps, warmup, min_seconds=0.0, want_outputs=False):
        """Cold call, warm-up, the timed region (HIP events around the encoder launches inside it); with --full extra steps
        with events around the pooling launches; optionally a sustained leg of at least `min_seconds`.  want_outputs: the
        results of the timed region's last step are copied out right after it (Bench.outputs)."""
        eng = self.eng
        # the cold call: whatever the context did not set up at creation (flush-group offsets, output staging, tables of
        # bag sizes it could not know) is built inside
        self.fence()
        t0 = time.perf_counter()
        self.step()
        self.fence()
        first_call_ms = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        self.step()                                          # the same call again, alone and synchronised: what a cold call could cost at best
        self.fence()
        second_call_ms = (time.perf_counter() - t0) * 1e3
        for _ in range(warmup):
            self.step()
        # HIP events around every launch of the dominant kernel (the encoder) inside the timed region -- roofline.achieved
        # comes from them; the pooling kernel is timed the same way over a few extra steps after it (every pair of events
        # costs the stream ~10 us per step, and the headline pays only for the pair it needs)
        self.fence()
        eng.profile("encoder")
        timing_gather = hasattr(self.gather, "timed_pairs")
        if timing_gather:
            self.gather.timing = True
        dt = self.timed(steps)
        own_dt = getattr(self, "own_dt", dt)
        outputs = self.outputs() if want_outputs else None
        gather_ms = None
        if timing_gather:
            gather_ms, _ = self.gather.exchange_ms()
            self.gather.timing = False
        enc_ms, enc_n = eng.profile_read(0)
        enc_clk = eng.profile_clock(0)                       # in-kernel stamps of the region's last encoder launch
        pool_ms, pool_n, pool_clk = 0.0, 0, None
        if self.args.full:
            eng.profile("pooling")
            self.timed(min(steps, 10))
            pool_ms, pool_n = eng.profile_read(1)
            pool_clk = eng.profile_clock(1)
        eng.profile(False)
        eng.sync()
        sustained = None
        if min_seconds > 0:
            smi, n_done, t_all = None, 0, 0.0
            while t_all < min_seconds:
                if smi is None and t_all >= 0.7 * min_seconds:
                    # sample while the GPU is loaded: queue a leg, ask rocm-smi, then wait for the leg
                    self.fence()
                    t0 = time.perf_counter()
                    for _ in range(steps):
                        self.step()
                    smi = smi_snapshot() if self.rank == 0 else {}
                    self.fence()
                    t_leg = time.perf_counter() - t0
                else:
                    t_leg = self.timed(steps)
                t_leg, = self.max_over_ranks(t_leg)           # every rank adds the same number: they leave the loop together
                t_all += t_leg
                n_done += steps
            sustained = {"seconds": t_all, "steps": n_done, "ms_per_step": t_all / n_done * 1e3, "rocm_smi_under_load": smi}
        dt, first_call_ms = self.max_over_ranks(dt, first_call_ms)
        return {"dt": dt, "first_call_ms": first_call_ms, "second_call_ms": second_call_ms, "enc_ms": enc_ms, "enc_n": enc_n, "pool_ms": pool_ms, "pool_n": pool_n,
                "enc_clk": enc_clk, "pool_clk": pool_clk,
                "sustained": sustained, "own_ms_per_step": own_dt / steps * 1e3, "gather_ms_per_step": gather_ms, "outputs": outputs}

    def outputs(self):
        """What the timed region's last step handed its caller, copied to the host (rank 0; None elsewhere): read_prob (this
        rank's reads), site_prob and mod_ratio (the whole job's, gathered, when there is an exchange).  An array longer than
        its cap is cut to a fixed seeded sample of positions, so the dump stays under 64 MB.
        Returns {name: (host array, length of the full array, sorted sample positions or None)}."""
        torch = self.torch
        site, mod = self.gather.finish() if self.gather is not None else (self.site, self.mod)
        if self.rank != 0:
            return None

        def take(t, cap, seed, idx=None):
            n = int(t.numel())
            if n <= cap:
                return t.cpu().numpy(), n, None
            if idx is None:
                idx = np.sort(np.random.default_rng(seed).choice(n, cap, replace=False))
            return t[torch.from_numpy(idx).to(t.device)].cpu().numpy(), n, idx
        out = {"read_prob": take(self.rp, DUMP_READS_MAX, DUMP_SEEDS["read_prob"])}
        out["site_prob"] = take(site, DUMP_SITES_MAX, DUMP_SEEDS["site_prob"])
        out["mod_ratio"] = take(mod, DUMP_SITES_MAX, DUMP_SEEDS["mod_ratio"], out["site_prob"][2])     # the same sites as site_prob
        return out

    def certify(self, r, local_ms):
        """What makes an N-rank line checkable from the line alone (collective; returns the keys on rank 0): the communicator's
        own rank count / device / RCCL version on every rank, how rank 0's device reaches the others, every rank's own step
        time (in the timed region, before the barrier), its compute-only step time (before the process group existed), and the
        exchange's own duration from HIP events on the stream that carries it."""
        info = None
        if hasattr(self.gather, "timed_pairs"):
            try:
                info = self.eng.comm_info()
            except Exception as e:                          # noqa: BLE001
                info = {"error": str(e)[:200]}
        mine = {"rank": self.rank, "device": self.dev.index, "sites": self.Sr, "reads": self.R, "own_ms_per_step": r["own_ms_per_step"],
                "local_ms_per_step": local_ms, "gather_ms_per_step": r["gather_ms_per_step"], "comm": info}
        rows = [None] * self.world
        self.dist.all_gather_object(rows, mine)
        if self.rank != 0:
            return None
        links = None
        try:
            from m6anet_amd.engine import device_link
            links = [dict(device_link(rows[0]["device"], x["device"]), to_rank=x["rank"]) for x in rows[1:]]
        except Exception as e:                              # noqa: BLE001 -- e.g. each rank sees only its own device
            links = "unavailable: %s" % str(e)[:120]
        comms = [x["comm"] for x in rows]
        native = all(isinstance(c, dict) and "ranks_seen" in c for c in comms)
        return {
            "rccl": {"ranks_seen": [c["ranks_seen"] for c in comms] if native else None,
                     "ranks_seen_all_equal_world": bool(native and all(c["ranks_seen"] == self.world for c in comms)),
                     "version": comms[0].get("rccl_version") if native else None,
                     "comm_devices": [c["device"] for c in comms] if native else None,
                     "communicator": "m6a_comm_init (the library's own)" if native else "torch.distributed's (%s)" % self.backend,
                     "links_from_rank0": links},
            "per_rank": {"sites": [x["sites"] for x in rows], "reads": [x["reads"] for x in rows],
                         "ms_per_step": [x["own_ms_per_step"] for x in rows],
                         "local_ms_per_step": [x["local_ms_per_step"] for x in rows],
                         "gather_ms_per_step": [x["gather_ms_per_step"] for x in rows],
                         "note": "ms_per_step: the rank's own wall time per step inside the timed region, exchange included, before the "
                                 "closing barrier; local_ms_per_step: its compute-only step before the process group was formed; "
                                 "gather_ms_per_step: HIP events around m6a_gather on the side stream that carries it (it overlaps the next step)"},
        }

    def verify(self):
        """rank 0 recomputes the WHOLE job unsharded on its GPU and compares the gathered arrays bit for bit"""
        from m6anet_amd import synthetic
        from m6anet_amd.engine import M6ANetEngine
        torch = self.torch
        got = self.gather.finish() if self.gather is not None else (self.site, self.mod)
        if self.rank != 0:
            return None
        parts = [synthetic.make_sites(int(self.cuts[r + 1] - self.cuts[r]), seed=20250328 + r,
                                      n_reads=self.n_reads_job[int(self.cuts[r]):int(self.cuts[r + 1])]) for r in range(self.world)]
        wX = torch.from_numpy(np.concatenate([p["X"] for p in parts])).to(self.dev)
        wk = torch.from_numpy(np.concatenate([p["site_kmers"] for p in parts])).to(self.dev)
        whole = M6ANetEngine(weights=self.weights, device=self.dev.index or 0)
        _, w_site, w_mod = whole.infer(wX, wk, torch.from_numpy(self.off_job).to(self.dev), self.T, 20, self.thr, 0, 16, 2, want_read_probs=False)
        whole.sync()
        ok = bool(np.array_equal(got[0].cpu().numpy(), w_site.cpu().numpy()) and np.array_equal(got[1].cpu().numpy(), w_mod.cpu().numpy()))
        whole.close()
        return ok

    def report(self, r, steps, traffic=True, gather_ceiling=True):
        """The measured quantities of one workload as the keys of the bench line."""
        eng, args, spec = self.eng, self.args, self.spec
        world, S, T, bag, R, Sr = self.world, self.S, self.T, self.bag, self.R, self.Sr
        total_sites = int(self.cuts[-1])
        enc_avg_ms = r["enc_ms"] / max(r["enc_n"], 1)
        pool_avg_ms = r["pool_ms"] / max(r["pool_n"], 1)
        enc_tflops = ENC_FLOP_PER_READ * R / (enc_avg_ms * 1e-3) / 1e12
        enc_gbps = ENC_BYTES_PER_READ * R / (enc_avg_ms * 1e-3) / 1e9
        draws = Sr * T * 20
        enc_kernel = eng.last_encoder_kernel
        executed = ENC_MFMA_PER_TILE[enc_kernel] * 4096 // 32
        enc_tflops_executed = executed * R / (enc_avg_ms * 1e-3) / 1e12
        pool_kernel = {"table-reg": "pool_reg_kernel", "table": "pool_table_kernel", "ragged-table": "pool_rtab_kernel"}.get(
            eng.last_pool_variant, "pool_scan_kernels")
        tr = None
        if world == 1 and traffic:
            default_shape = S == spec["sites"] and T == 1000 and (self.workload == "ragged" or bag == spec["bag"])
            if args.full and default_shape and not args.no_live_traffic:
                tr = live_traffic(self.workload, enc_kernel, pool_kernel, enc_variant=args.enc_variant)
            if tr is None:
                tr = measured_traffic(S, bag)
                if tr is not None:
                    tr = dict(tr, source="%s (%s) -- committed, not measured by this run" % (tr["file"], tr["source"]))
        proof = pool_roofline(eng.last_pool_variant, draws, pool_avg_ms, r["pool_n"])
        # the pooling kernels are priced against what the part DELIVERS for their instruction mix, measured by this run with the
        # microbenchmark of their inner loop: `peak` / `frac` are that; the nominal figure stays beside it
        m, detail = None, {}
        if gather_ceiling and self.rank == 0 and proof["achieved"]:
            if eng.last_pool_variant == "table-reg":
                m = measured_multiply_ceiling()
                detail = {"T_lane_multiplies_per_s": m["rows"]} if m else {}
            elif eng.last_pool_variant == "ragged-table":
                m = measured_gather_ceiling(bag)
                detail = {"T_gathers_per_s_by_bag_size": m["points"]} if m else {}
        # `peak` / `frac` are ALWAYS the nominal figure (comparable across rounds); what the part delivers for the kernel's
        # instruction mix, measured by this run, sits beside them
        proof["peak_source"] = "nominal"
        if tr and tr.get("pool"):
            # HBM reads of the pooling kernel from the same PMC passes, next to the read probabilities it needs (4 B per read)
            proof["traffic"] = dict(tr["pool"], algorithmic_read_bytes=4 * R)
        if m is not None:
            proof["measured_ceiling"] = dict({"peak": m["rate"] / 1e12, "unit": "T draws/s", "frac": proof["achieved"] * 1e12 / m["rate"],
                                              "source": m["source"]}, **detail)
        else:
            proof["measured_ceiling"] = None
        value = total_sites * steps / r["dt"]
        out = {
            "value": value,
            "ms_per_step": r["dt"] / steps * 1e3,
            "first_call_ms": r["first_call_ms"],
            "context_ms": self.context_ms,
            "second_call_ms": r["second_call_ms"],           # one call, alone and synchronised, everything cached (steps in the timed region queue back to back)
            # a real job is ONE call on a fresh context: sites / the cold call (what m6a_create did not prepare is inside)
            "value_one_shot": total_sites / (r["first_call_ms"] * 1e-3),
            # ... and if the caller does NOTHING between m6a_create and that call (no loading, no H2D), the whole background
            # set-up is waited for as well: the worst case of a one-shot process, HIP runtime start-up aside
            "value_one_shot_incl_context": total_sites / ((r["first_call_ms"] + sum(self.context_ms.values())) * 1e-3),
            "roofline": {"kernel": "read encoder (%s: %s)" % (eng.last_encoder_variant, enc_kernel), "bound": "mfma", "achieved": enc_tflops,
                         "peak": PEAK_F32_TFLOPS, "unit": "TFLOP/s", "frac": enc_tflops / PEAK_F32_TFLOPS,
                         # the same launch priced by the MFMA work it EXECUTES rather than SURVEY 8(d)'s algorithmic count
                         "executed_flop_per_read": executed, "mfma_per_32_read_tile": ENC_MFMA_PER_TILE[enc_kernel],
                         "achieved_executed": enc_tflops_executed, "frac_executed": enc_tflops_executed / PEAK_F32_TFLOPS,
                         "traffic": tr["traffic_bytes_per_launch"] if tr else None,
                         "traffic_source": tr["source"] if tr else None,
                         "algorithmic_bytes_per_launch": ENC_BYTES_PER_READ * R,
                         "avg_launch_ms": enc_avg_ms, "launches": r["enc_n"],
                         "algorithmic_flop_per_read": ENC_FLOP_PER_READ, "reads_per_launch": R,
                         "hbm_view": {"achieved": enc_gbps, "peak": PEAK_HBM_GBPS, "unit": "GB/s",
                                      "frac": enc_gbps / PEAK_HBM_GBPS, "algorithmic_bytes_per_read": ENC_BYTES_PER_READ}},
            "pool_roofline": at_measured_clock(proof, r.get("pool_clk")),
            "kernels": {enc_kernel: {"avg_ms": enc_avg_ms, "launches": r["enc_n"]},
                        pool_kernel: {"avg_ms": pool_avg_ms, "launches": r["pool_n"], "timed_in": "extra steps after the timed region",
                                      "Gdraws_per_s": draws / (pool_avg_ms * 1e-3) / 1e9 if pool_avg_ms else None}},
        }
        at_measured_clock(out["roofline"], r.get("enc_clk"))
        if not r["pool_n"]:
            # only --full times the pooling launches (extra steps in Bench.run): without them there is no pooling figure
            del out["pool_roofline"], out["kernels"][pool_kernel]
        if r["sustained"]:
            su = r["sustained"]
            out["value_sustained"] = total_sites * su["steps"] / su["seconds"]
            out["sustained"] = su
        return out

    def config(self):
        spec, bag, world = self.spec, self.bag, self.world
        bag_txt = "%d reads" % bag if not isinstance(bag, tuple) else "%d..%d reads" % bag
        return {"workload": "synthetic %d DRACH sites x %s per GPU, %s weights, num_iterations=%d, numpy-stream replay "
                            "(batch_size 16, save_per_batch 2, seed 0); %s%s"
                            % (self.S, bag_txt, spec["model"], self.T, spec["config"],
                               " x%d GPUs%s" % (world, " (configs[3])" if self.workload == "uniform" else " (configs[4])") if world > 1 else ""),
                "sites_per_gpu": self.S, "reads_per_site": list(bag) if isinstance(bag, tuple) else bag, "reads_rank0": self.R,
                "num_iterations": self.T,
                "bag_statistics": "host copy of off[] per step, device-checked (m6a_set_host_offsets)" if self.host_offsets else "read back per step",
                "pool_kernel": self.eng.last_pool_variant, "encoder_kernel": self.eng.last_encoder_variant,
                "encoder_kernel_function": self.eng.last_encoder_kernel,
                # ONE encoder for the product and the headline: the library's automatic choice, the CLI's default
                # and this line's timed region are the same kernel -- tests/test_gpu_stream.py asserts it
                "library_auto_encoder": "general16 (m6a_set_encoder_variant 0: enc_site16_kernel on bags >= 16 reads, enc_kernel otherwise)",
                "cli_default_encoder": "general16 (`m6anet_amd inference`, = --encoder reference: the library's automatic choice; the reference's "
                                       "float32 operations in its order, read probabilities bit-identical to the oracle; --encoder fast = "
                                       "the opt-in 12-slot kernel, key fast_encoder_optin)",
                "encoder_selected_by": {0: "auto (library default)", 1: "--enc-variant 1", 2: "--enc-variant 2 (12-slot, opt-in)",
                                        3: "--enc-variant 3", 4: "--enc-variant 4 (fast, opt-in)"}[self.args.enc_variant],
                "sharding": "contiguous flush-group-aligned site shards balanced by reads, 1 gather of site_prob + mod_ratio to rank 0 per step "
                            "over %s" % self.gather_kind if self.gather is not None else "none"}


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--workload", choices=sorted(WORKLOADS), default="uniform")
    ap.add_argument("--sites", type=int, default=None, help="sites per GPU (default: the workload's)")
    ap.add_argument("--reads", type=int, default=None, help="uniform workload: reads per site (default 20)")
    ap.add_argument("--iters", type=int, default=1000, help="num_iterations")
    ap.add_argument("--full", action="store_true",
                    help="after the headline, measure everything else the line can carry (runs of their own): the pooling roofline and "
                         "its measured ceiling, live PMC traffic, the sustained leg, the extra legs of the default shape, the CPU baseline")
    ap.add_argument("--min-seconds", type=float, default=None,
                    help="after the timed region (which alone defines `value`) keep stepping for at least this long and report "
                         "value_sustained plus rocm-smi's clock / power under load -- the K-step region is tens of milliseconds, inside "
                         "one DVFS window; default 3 with --full, otherwise 0 (no leg)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--no-ragged-extra", action="store_true",
                    help="with --full, default run only: skip the extra legs (the opt-in 12-slot encoder, host inputs, and the `ragged` "
                         "key: configs[4]'s per-GPU shape, ~10 steps after the headline)")
    ap.add_argument("--no-live-traffic", action="store_true",
                    help="with --full: do not re-run under rocprofv3 for roofline.traffic; quote the committed "
                         "profiles/*_enc_traffic.json instead (what a plain run does)")
    ap.add_argument("--cpu-baseline-only", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--enc-variant", type=int, default=0,
                    help="m6a_set_encoder_variant: 0 auto = the 16-slot kernels (the reference's bits; what the CLI runs), 1 the same, "
                         "2 the 12-slot kernel, 3 16-slot per-lane walk, 4 fast (12-slot where it applies)")
    ap.add_argument("--scan-driver", type=int, default=0, help="ragged bags: 0 auto, 1 per group, 2 per site, 3 index tables")
    ap.add_argument("--verify", action="store_true",
                    help="after the timed steps rank 0 recomputes the WHOLE job unsharded on its GPU and checks that the gathered "
                         "site_prob / mod_ratio equal it bit for bit (small --sites only: rank 0 holds the whole job)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps write what their last step computed to DIR/<name>.npy: read_prob (float32), site_prob "
                         "(float32), mod_ratio (float64); arrays above 4 M reads / 3 M sites are a fixed seeded sample of positions")
    args = ap.parse_args(argv)
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if args.min_seconds is None:
        args.min_seconds = 3.0 if args.full else 0.0
    return args


def main():
    args = parse_args()
    if args.cpu_baseline_only:
        print(json.dumps(cpu_baseline_main(args.workload, args.iters, budget_s=20.0)))
        return

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # no launcher: start our own ranks, one per GPU, rendezvous on 127.0.0.1
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus),
               "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.abspath(__file__)] + sys.argv[1:]
        sys.exit(subprocess.call(cmd))

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit("--gpus %d but WORLD_SIZE=%d" % (args.gpus, world))

    spec = WORKLOADS[args.workload]
    S = args.sites or spec["sites"]
    bag = spec["bag"] if args.workload == "ragged" else (args.reads or spec["bag"])
    T = args.iters
    line = {"metric": "DRACH sites/sec at num_iterations=%d" % T, "value": None, "unit": "sites/s", "n_gpus": world,
            "steps": args.steps, "warmup": args.warmup, "ms_per_step": None, "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": "f32", "data": "synthetic", "config": {"workload": "%s (%s)" % (args.workload, spec["config"])}}
    printed = []

    def emit(error=None):
        """rank 0's ONE JSON line -- also when the run does not get to its end (a rank died, an exchange hung): the
        driver then still reads what was measured and why the rest is missing."""
        if rank != 0 or printed:
            return
        printed.append(1)
        if error:
            line["error"] = error
        print(json.dumps(line), flush=True)

    # Fail-safe for the multi-rank run: torch.distributed.run terminates every rank when one of them dies, and a stuck
    # exchange never returns.  A watchdog thread prints rank 0's line with what is known and leaves with a non-zero code,
    # on SIGTERM or at the deadline.  The signal reaches it through the wake-up descriptor: the main thread may be blocked
    # inside a collective (no Python handler runs there), the C-level handler still writes the signal number to the socket.
    import signal
    import threading
    deadline = float(os.environ.get("M6A_BENCH_TIMEOUT", "1500"))
    done = threading.Event()
    rsock, wsock = socket.socketpair()
    wsock.setblocking(False)

    def watchdog():
        rsock.settimeout(deadline)
        try:
            data = rsock.recv(1)
        except socket.timeout:
            emit("watchdog: no result after %.0f s (M6A_BENCH_TIMEOUT); a rank or an exchange is stuck" % deadline)
            os._exit(3)
        if done.is_set():
            return
        emit("terminated by the launcher (signal %d): another rank failed" % (data[0] if data else 0))
        os._exit(4)

    if world > 1:
        signal.signal(signal.SIGTERM, lambda signum, frame: None)
        signal.set_wakeup_fd(wsock.fileno(), warn_on_full_buffer=False)
        threading.Thread(target=watchdog, daemon=True).start()

    def finish():
        done.set()
        try:
            wsock.send(b"\0")
        except OSError:
            pass

    try:
        run(args, line, rank, world, local_rank, S, bag, T)
    except BaseException as e:                                # noqa: BLE001 -- the line must come out whatever happened
        if isinstance(e, SystemExit) and not e.code:
            raise
        import traceback
        traceback.print_exc()
        emit("%s: %s" % (type(e).__name__, str(e)[:400]))
        finish()
        sys.stdout.flush()
        sys.stderr.flush()
        if world > 1:
            os._exit(1)
        sys.exit(1)
    finish()
    emit()


def dump_outputs(out_dir, outputs):
    """Writes Bench.outputs() as <out_dir>/<name>.npy; returns what the bench line says about them."""
    os.makedirs(out_dir, exist_ok=True)
    arrays = {}
    for name, (a, n, idx) in outputs.items():
        np.save(os.path.join(out_dir, name + ".npy"), a)
        arrays[name] = {"dtype": str(a.dtype), "shape": list(a.shape), "length": n,
                        "sample": None if idx is None else "%d sorted positions drawn without replacement by numpy default_rng(%d)"
                                                          % (len(idx), DUMP_SEEDS[name])}
    return {"dir": os.path.abspath(out_dir), "step": "last timed step", "arrays": arrays}


def run(args, line, rank, world, local_rank, S, bag, T):
    import torch
    from m6anet_amd import dist as mdist

    backend = os.environ.get("M6A_BENCH_BACKEND", "nccl")
    if backend != "nccl":
        local_rank %= max(torch.cuda.device_count(), 1)
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)

    b = Bench(args, args.workload, S, bag, T, rank, world, local_rank, dev, backend)
    line["config"] = b.config()
    # M6A_BENCH_FORCE_EXCHANGE=1 (under a launcher's environment): form the process group and run the exchange at world
    # size 1 too -- the one-GPU test box drives the RCCL leg of the N-GPU run that way
    multi = world > 1 or (os.environ.get("M6A_BENCH_FORCE_EXCHANGE") == "1" and "RANK" in os.environ)
    if multi:
        # before any rank depends on another: this rank's own cold call and a few compute-only steps
        t0 = time.perf_counter()
        b.compute()
        torch.cuda.synchronize(dev)
        cold = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        for _ in range(5):
            b.compute()
        torch.cuda.synchronize(dev)
        local_ms = (time.perf_counter() - t0) / 5 * 1e3
        line["rank0_local"] = {"cold_call_ms": cold, "ms_per_step": local_ms, "sites_per_s": b.Sr / (local_ms * 1e-3),
                               "note": "rank 0's own shard, no exchange, measured before the process group is formed"}
        import torch.distributed as dist
        mdist.init_from_env(backend, device_id=dev if backend == "nccl" else None)
        b.setup_exchange(dist, mdist)
        line["config"] = b.config()

    if os.environ.get("M6A_BENCH_TEST_KILL_RANK") == str(rank):   # test hook: this rank dies before the timed region
        os._exit(9)
    r = b.run(args.steps, args.warmup, args.min_seconds, want_outputs=args.dump_outputs is not None)
    if r["outputs"] is not None:
        line["dump_outputs"] = dump_outputs(args.dump_outputs, r.pop("outputs"))
    cert = None
    if multi:
        # every rank made its cold call alone above; what run() timed first was only the first call WITH the exchange
        r["first_call_ms"], = b.max_over_ranks(cold)
        cert = b.certify(r, local_ms)
    verified = b.verify() if args.verify else None
    if rank == 0:
        rep = b.report(r, args.steps)
        line.update({"value": rep.pop("value"), "ms_per_step": rep.pop("ms_per_step"), "config": b.config(),
                     "first_call_ms": rep.pop("first_call_ms"), "second_call_ms": rep.pop("second_call_ms"), "value_one_shot": rep.pop("value_one_shot"), "verify": verified})
        line.update(rep)
        if cert:
            line.update(cert)
            # the driver computes scaling efficiency itself from the per-N values; this is the same quantity from ONE line:
            # whole-job rate over N x what rank 0 does alone on its shard (weak scaling: 1.0 = the exchange and the barrier are free)
            line["efficiency"] = line["value"] / (world * line["rank0_local"]["sites_per_s"])
        default_run = (world == 1 and args.workload == "uniform" and S == WORKLOADS["uniform"]["sites"] and T == 1000 and
                       bag == WORKLOADS["uniform"]["bag"])
        if args.full and default_run and not args.no_ragged_extra:
            # three EXTRA legs after the headline; each is optional: a failure is recorded under "<leg>_error" and the line goes out
            def optional(name, leg):
                try:
                    leg()
                except Exception as e:                      # noqa: BLE001
                    line[name + "_error"] = "%s: %s" % (type(e).__name__, str(e)[:300])

            def leg_fast_encoder():
                # the same workload on the OPT-IN 12-slot encoder (m6a_set_encoder_variant(4), `--encoder fast`): 106 MFMAs per
                # tile instead of 116, read probabilities within rtol 1e-5 of the reference instead of its bits.  The headline
                # above is the library's automatic choice -- the kernel the CLI, INTEGRATION.md's stub and every caller that
                # sets nothing run; this key says what the opt-in buys, with its own roofline from HIP events around its launches
                b.eng.set_encoder_variant(4)
                for _ in range(3):
                    b.compute()
                legs = []
                for _ in range(3):                            # three legs of 10 steps, the median reported: a 27 ms region is one hiccup away from +4 %
                    torch.cuda.synchronize(dev)
                    t0 = time.perf_counter()
                    for _ in range(10):
                        b.compute()
                    torch.cuda.synchronize(dev)
                    legs.append((time.perf_counter() - t0) / 10 * 1e3)
                ms = sorted(legs)[1]
                b.eng.profile("encoder")
                for _ in range(10):
                    b.compute()
                k_ms, k_n = b.eng.profile_read(0)
                k_clk = b.eng.profile_clock(0)
                b.eng.profile(False)
                kern = b.eng.last_encoder_kernel
                k_avg = k_ms / max(k_n, 1)
                ex = ENC_MFMA_PER_TILE[kern] * 4096 // 32
                tf, tfx = (f * b.R / (k_avg * 1e-3) / 1e12 for f in (ENC_FLOP_PER_READ, ex))
                line["fast_encoder_optin"] = {
                    "encoder_kernel": b.eng.last_encoder_variant, "kernel": kern, "ms_per_step": ms, "value": b.Sr / (ms * 1e-3), "steps": 10, "warmup": 3,
                    "ms_per_step_of_each_leg": legs,
                    "note": "same workload, m6a_set_encoder_variant(4) / `m6anet_amd inference --encoder fast` / M6A_ENCODER=fast: the 12-slot "
                            "kernel (per-site constants pre-summed, plain 32 -> 1 sum; within rtol 1e-5 of the reference, not its bits). "
                            "NOT the headline: `value` above runs the automatic choice, the 16-slot kernel",
                    "roofline": at_measured_clock({
                        "kernel": "read encoder (%s: %s), opt-in" % (b.eng.last_encoder_variant, kern),
                        "bound": "mfma", "achieved": tf, "peak": PEAK_F32_TFLOPS, "unit": "TFLOP/s", "frac": tf / PEAK_F32_TFLOPS,
                        "traffic": None, "avg_launch_ms": k_avg, "launches": k_n, "algorithmic_flop_per_read": ENC_FLOP_PER_READ,
                        "executed_flop_per_read": ex, "mfma_per_32_read_tile": ENC_MFMA_PER_TILE[kern], "achieved_executed": tfx,
                        "frac_executed": tfx / PEAK_F32_TFLOPS, "reads_per_launch": b.R,
                        "timed_in": "10 extra steps after the three legs, HIP events around every launch"}, k_clk)}
                b.eng.set_encoder_variant(args.enc_variant)

            def leg_ragged():
                # the path real data takes (bags are never uniform), in the same record: configs[4]'s per-GPU shape
                del b.X, b.rp
                b.eng.close()
                torch.cuda.empty_cache()
                rs = WORKLOADS["ragged"]
                rb = Bench(args, "ragged", rs["sites"], rs["bag"], 1000, 0, 1, local_rank, dev, backend)
                rr = rb.run(10, 3, args.min_seconds)
                rg = rb.report(rr, 10)                        # incl. its own live PMC passes for roofline.traffic
                rg["config"] = rb.config()
                rg["steps"], rg["warmup"] = 10, 3
                line["ragged"] = rg
                rb.eng.close()

            optional("fast_encoder_optin", leg_fast_encoder)
            b.eng.set_encoder_variant(args.enc_variant)
            line["with_h2d"] = with_h2d(b, T)
            optional("ragged", leg_ragged)
        if args.full and world == 1 and not args.no_cpu_baseline:
            line["cpu_baseline"] = run_cpu_baseline_subprocess(args.workload, T)
    if multi:
        import torch.distributed as dist
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
