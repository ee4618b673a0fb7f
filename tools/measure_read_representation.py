#!/usr/bin/env python
"""What storing the read representation costs (m6a_read_representation, enc_repr_kernel) -> profiles/r23_read_representation.json.

The job: 1 M sites x 20 reads, X / site_kmers / off resident in device memory, outputs in device memory.  Three times, each the
median over interleaved legs (a leg = the median of --calls device-event timings of one call, after a warm-up call):

  T_repr   m6a_read_representation (repr [20 M][32] = 2.56 GB and read_prob), this build;
  T_walk   m6a_encode_reads with M6A_ENCODER=walk16 (enc_kernel: the same arithmetic behind the same per-lane walk, no repr) --
           of the built checkout given with --parent-tree (the parent commit: its package and its library) when there is one,
           else of this build (the shipped kernels are not edited by the change that added enc_repr_kernel, and the JSON says
           which library was timed);
  T_write  a device-to-device hipMemcpyAsync of repr's 2.56 GB.

The bar: T_repr <= T_walk + T_write + spread(T_walk), spread = max - min over T_walk's own legs: a kernel that computed and THEN
stored with no overlap at all would meet it, so missing it means the stores are badly formed.

The default path is untouched: with --parent-tree, bench.py of the parent checkout and of this tree run in alternating processes
(--bench-rounds each); `value` of this build must be within the parent's median and its own spread, and the arrays of
--dump-outputs must be equal.

Legs run in child processes, one tree per process, alternating parent / this build for --rounds rounds; inside a process the
calls of its legs are interleaved as well.  Every device call is made by the children; a child that finds no GPU fails.

    python tools/measure_read_representation.py [--parent-tree DIR] [--out profiles/r23_read_representation.json]

--eventalign SHAPE (a size such as 3.1GB, or a number of copies of the bundled file: tools/measure_eventalign_inference.py's shapes)
measures `eventalign_inference --read_representation` instead -> profiles/r24_repr_eventalign.json:

  the command without the flag, with it, and with it in float16 (and, with --parent-tree, the parent's command without the flag),
  --legs interleaved runs each in processes of their own: wall seconds and the M6A_EVENTALIGN_TIMES phases;
  the writer against its parts with no overlap: its own repr_kernel + one plain hipMemcpy of the same bytes into pinned memory + one
  pwrite of the same bytes into the same directory, timed in the same session (child `parts`); the writer's wall time (repr_total) must
  not exceed that sum plus the spread of the sum's legs;
  the float32 kernel of this build against the parent's at 1 M sites x 20 reads (bar: the parent's median plus its own spread), the
  float16 kernel beside it, and bench.py against the parent as above.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_SITES, BAG = 1_000_000, 20


def child(args):
    """One process, one library: `--calls` timed calls of each of its legs, interleaved call by call."""
    sys.path.insert(0, os.path.abspath(args.tree) if args.tree else REPO)
    import numpy as np
    import torch
    from m6anet_amd import _lib
    from m6anet_amd.engine import M6ANetEngine, load_weights
    if not torch.cuda.is_available():
        raise SystemExit("no HIP device: nothing is measured without one")
    dev = "cuda:0"
    S, R = args.sites, args.sites * BAG
    g = torch.Generator(device=dev).manual_seed(1)
    X = torch.randn((R, 9), generator=g, device=dev, dtype=torch.float32).clamp_(-6, 6)
    km = torch.randint(0, 66, (S, 3), generator=g, device=dev, dtype=torch.uint8)
    off_h = np.arange(S + 1, dtype=np.int64) * BAG
    off = torch.from_numpy(off_h).to(dev)
    rp = torch.empty(R, dtype=torch.float32, device=dev)
    eng = M6ANetEngine(weights=load_weights(), device=0)        # M6A_ENCODER (walk16 for the walk leg) was set by the parent process
    torch.cuda.synchronize()

    def kernel_ms(call):
        """The library's own device events around the encoder launch (m6a_profile_enable): the kernel, not the host side of the call."""
        eng.profile("encoder")
        eng.set_host_offsets(off_h)                              # no read-back, no host synchronise inside the call
        call()
        ms, n = eng.profile_read(0)
        eng.sync()                                               # the deferred check of the host offsets
        assert n == 1, n
        return ms

    legs = {}
    if args.child == "walk":
        legs["walk"] = lambda: kernel_ms(lambda: eng.get_read_probability(X, km, off, out=rp))
    else:
        rep = torch.empty((R, 32), dtype=torch.float32, device=dev)
        dst = torch.empty_like(rep)
        hip = C.CDLL(os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so"))
        hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
        side = torch.cuda.Stream()

        def write():
            with torch.cuda.stream(side):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                rc = hip.hipMemcpyAsync(dst.data_ptr(), rep.data_ptr(), rep.numel() * 4, 3, side.cuda_stream)   # hipMemcpyDeviceToDevice
                b.record()
            if rc != 0:
                raise RuntimeError("hipMemcpyAsync: %d" % rc)
            b.synchronize()
            return a.elapsed_time(b)
        legs["repr"] = lambda: kernel_ms(lambda: eng.get_read_representation(X, km, off, out=(rep, rp)))
        legs["write"] = write
        if hasattr(_lib, "REPR_DTYPES"):                         # a build with m6a_read_representation_dtype
            rep16 = torch.empty((R, 32), dtype=torch.float16, device=dev)
            legs["repr_f16"] = lambda: kernel_ms(lambda: eng.get_read_representation(X, km, off, out=(rep16, rp), dtype="float16"))
    times = {k: [] for k in legs}
    for f in legs.values():                                      # warm-up: code objects, first touch of the outputs
        f()
    for _ in range(args.calls):
        for k, f in legs.items():
            times[k].append(f())
    out = {"lib": os.path.relpath(_lib.LIB_PATH, os.path.abspath(args.tree) if args.tree else REPO), "kernel": eng.last_encoder_kernel, "device": torch.cuda.get_device_name(0),
           "ms": {k: statistics.median(v) for k, v in times.items()}, "calls_ms": times}
    print("LEG " + json.dumps(out), flush=True)


def parts_child(args):
    """The writer's parts with no overlap: one hipMemcpy of --bytes from device into pinned memory, one pwrite of them into --dir."""
    import time
    import numpy as np
    import torch
    n = args.bytes
    dev = torch.empty(n, dtype=torch.uint8, device="cuda:0").fill_(7)
    pin = torch.empty(n, dtype=torch.uint8).pin_memory()
    host = pin.numpy()
    path = os.path.join(args.dir, "parts.bin")
    copy_ms, write_ms = [], []
    for k in range(args.calls + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pin.copy_(dev)                                           # blocking hipMemcpy into pinned memory
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        fd = os.open(path, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
        os.ftruncate(fd, n)
        at = 0
        view = memoryview(host)
        while at < n:
            at += os.pwrite(fd, view[at:at + (1 << 30)], at)
        os.close(fd)
        t2 = time.perf_counter()
        if k:                                                    # the first pass touches the pages
            copy_ms.append((t1 - t0) * 1e3)
            write_ms.append((t2 - t1) * 1e3)
    os.remove(path)
    assert int(np.asarray(host[:1])[0]) == 7
    print("LEG " + json.dumps({"copy_ms": copy_ms, "write_ms": write_ms, "bytes": n}), flush=True)


def eventalign_legs(args):
    """`eventalign_inference` without the flag, with it and with it in float16 (and the parent's command without it), interleaved"""
    import shutil
    import tempfile
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import measure_eventalign_inference as ME
    ev_dir = tempfile.mkdtemp(prefix="repr_eventalign_", dir=args.ev_dir)
    try:
        path, n = ME.write_shape(args.eventalign, ev_dir)
        kinds = {"plain": (REPO, []), "repr": (REPO, ["--read_representation"]),
                 "repr_f16": (REPO, ["--read_representation", "--representation_dtype", "float16"])}
        if args.parent_tree:
            kinds["parent_plain"] = (os.path.abspath(args.parent_tree), [])
        runs = {k: [] for k in kinds}
        env = dict(os.environ, M6A_EVENTALIGN_TIMES="1")
        for _ in range(args.legs):
            for kind, (tree, flags) in kinds.items():
                out = os.path.join(ev_dir, "out_" + kind)
                s, p = ME.timed(["eventalign_inference", "--eventalign", path, "--out_dir", out] + ME.THREADS + flags, args.leg_timeout, env=env, tree=tree)
                if p.returncode != 0:
                    raise SystemExit("%s failed (%d):\n%s" % (kind, p.returncode, p.stderr[-3000:]))
                t = json.loads(p.stdout.split("M6A_TIMES ", 1)[1].splitlines()[0])
                runs[kind].append({"wall_s": s, "ms": t["ms"], "d2h_bytes": t["d2h_bytes"], "peak_bytes": t["peak_bytes"], "n_reads": t["n_reads"],
                                   **{k: t[k] for k in ("repr_rounds", "repr_bytes") if k in t}})
                shutil.rmtree(out, ignore_errors=True)
                print("%s: %.2f s" % (kind, s), file=sys.stderr, flush=True)
        res = {"copies": n, "eventalign_GB": os.path.getsize(path) / 1e9, "legs": args.legs, "n_reads": runs["plain"][0]["n_reads"], "runs": runs}
        for kind, v in runs.items():
            w = [r["wall_s"] for r in v]
            res[kind + "_wall_s"] = {"median": statistics.median(w), "spread": max(w) - min(w)}
        if args.parent_tree:
            bar = res["parent_plain_wall_s"]["median"] + res["parent_plain_wall_s"]["spread"]
            res["plain_against_parent"] = {"bar_s": bar, "this_s": res["plain_wall_s"]["median"], "meets_bar": res["plain_wall_s"]["median"] <= bar}
        for kind in ("repr", "repr_f16"):
            nbytes = runs[kind][0]["repr_bytes"] - 128
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "parts", "--bytes", str(nbytes), "--dir", ev_dir, "--calls", str(args.legs)],
                               capture_output=True, text=True, timeout=args.leg_timeout)
            lines = [ln for ln in r.stdout.splitlines() if ln.startswith("LEG ")]
            if r.returncode != 0 or not lines:
                raise SystemExit("parts failed (%d):\n%s" % (r.returncode, r.stderr[-3000:]))
            parts = json.loads(lines[-1][4:])
            sums = [a["ms"]["repr_kernel"] + c + w for a, c, w in zip(runs[kind], parts["copy_ms"], parts["write_ms"])]
            total = statistics.median([a["ms"]["repr_total"] for a in runs[kind]])
            bar = statistics.median(sums) + max(sums) - min(sums)
            res[kind + "_writer"] = {"bytes": nbytes, "rounds": runs[kind][0]["repr_rounds"],
                                     "repr_kernel_ms": statistics.median([a["ms"]["repr_kernel"] for a in runs[kind]]),
                                     "repr_copy_ms": statistics.median([a["ms"]["repr_copy"] for a in runs[kind]]),
                                     "repr_write_ms": statistics.median([a["ms"]["repr_write"] for a in runs[kind]]),
                                     "plain_hipMemcpy_ms": statistics.median(parts["copy_ms"]), "plain_pwrite_ms": statistics.median(parts["write_ms"]),
                                     "sum_of_parts_ms": statistics.median(sums), "sum_spread_ms": max(sums) - min(sums), "bar_ms": bar,
                                     "writer_wall_ms": total, "meets_bar": total <= bar, "below_the_sum_ms": statistics.median(sums) - total,
                                     "flag_costs_s": res[kind + "_wall_s"]["median"] - res["plain_wall_s"]["median"]}
        return res
    finally:
        shutil.rmtree(ev_dir, ignore_errors=True)


def kernels_against_parent(args):
    """enc_repr_kernel of this build and of the parent at the r23 shape, and the float16 kernel beside them"""
    legs = {"parent_repr": [], "repr": [], "repr_f16": []}
    for _ in range(args.rounds):
        if args.parent_tree:
            legs["parent_repr"].append(run_child("repr", args.parent_tree, args)["ms"]["repr"])
        n = run_child("repr", None, args)
        legs["repr"].append(n["ms"]["repr"])
        legs["repr_f16"].append(n["ms"]["repr_f16"])
        print("kernels: %s" % {k: v[-1] for k, v in legs.items() if v}, file=sys.stderr, flush=True)
    res = {"shape": {"sites": args.sites, "reads_per_site": BAG}, "legs_ms": legs,
           "T_repr_ms": statistics.median(legs["repr"]), "T_repr_f16_ms": statistics.median(legs["repr_f16"]),
           "r23_T_repr_ms": 2.752}
    if args.parent_tree:
        med, spread = statistics.median(legs["parent_repr"]), max(legs["parent_repr"]) - min(legs["parent_repr"])
        res.update(T_parent_repr_ms=med, parent_spread_ms=spread, bar_ms=med + spread, meets_bar=res["T_repr_ms"] <= med + spread)
    return res


def run_child(kind, tree, args):
    env = dict(os.environ)
    env.pop("M6A_ENCODER", None)
    env.pop("M6A_HIP_LIB", None)
    if kind == "walk":
        env["M6A_ENCODER"] = "walk16"
    cmd = [sys.executable, os.path.abspath(__file__), "--child", kind, "--sites", str(args.sites), "--calls", str(args.calls)]
    if tree:
        cmd += ["--tree", tree]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=args.leg_timeout)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("LEG ")]
    if r.returncode != 0 or not lines:
        raise SystemExit("leg %s failed (%d):\n%s\n%s" % (kind, r.returncode, r.stdout[-2000:], r.stderr[-4000:]))
    return json.loads(lines[-1][4:])


def bench_alternating(args):
    """bench.py (--gpus 1 --steps 50 --warmup 10) of the parent checkout and of this tree, alternating, each run a process of its own"""
    import tempfile
    import numpy as np
    trees = {"parent": os.path.abspath(args.parent_tree), "this": REPO}
    values = {k: [] for k in trees}
    with tempfile.TemporaryDirectory() as tmp:
        for _ in range(args.bench_rounds):
            for name, tree in trees.items():
                r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "50", "--warmup", "10", "--dump-outputs",
                                    os.path.join(tmp, name)], cwd=tree, capture_output=True, text=True, timeout=args.leg_timeout)
                lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
                if r.returncode != 0 or not lines:
                    raise SystemExit("bench.py of the %s tree failed (%d):\n%s" % (name, r.returncode, r.stderr[-4000:]))
                values[name].append(json.loads(lines[-1])["value"])
        equal = {}
        for f in ("read_prob", "site_prob", "mod_ratio"):
            a, b = (np.load(os.path.join(tmp, n, f + ".npy")) for n in trees)
            equal[f] = bool(a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8)))
    med = statistics.median(values["parent"])
    spread = max(values["parent"]) - min(values["parent"])
    return {"unit": "sites/s (bench.py value, higher is better)", "parent_values": values["parent"], "this_values": values["this"],
            "parent_median": med, "parent_spread": spread, "this_median": statistics.median(values["this"]),
            "this_within_parent_median_and_spread": bool(statistics.median(values["this"]) >= med - spread), "dump_outputs_equal": equal}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--parent-tree", default=None, help="a built checkout of the parent commit: T_walk is taken from its package and library")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r23_read_representation.json"))
    ap.add_argument("--sites", type=int, default=N_SITES)
    ap.add_argument("--rounds", type=int, default=4, help="interleaved legs per time")
    ap.add_argument("--calls", type=int, default=7, help="timed calls per leg")
    ap.add_argument("--bench-rounds", type=int, default=4, help="with --parent-tree: bench.py runs per tree, alternating (0: none)")
    ap.add_argument("--leg-timeout", type=float, default=240.0, help="seconds a child process may take")
    ap.add_argument("--child", choices=("walk", "repr", "parts"), default=None, help=argparse.SUPPRESS)
    ap.add_argument("--tree", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--eventalign", default=None, help="a shape (3.1GB, or copies of the bundled file): measure the command, write r24_repr_eventalign.json")
    ap.add_argument("--legs", type=int, default=5, help="with --eventalign: interleaved runs per kind of command")
    ap.add_argument("--ev-dir", default=None, help="with --eventalign: where the generated file and the outputs go (default: the temporary directory)")
    ap.add_argument("--bytes", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--dir", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child == "parts":
        return parts_child(args)
    if args.child:
        return child(args)
    if args.eventalign:
        out = args.out if "r23_" not in os.path.basename(args.out) else os.path.join(REPO, "profiles", "r24_repr_eventalign.json")
        res = {"what": "eventalign_inference --read_representation [--representation_dtype float16] against the command without the flag, "
                       "the writer against its parts with no overlap, and the default paths against the parent commit",
               "parent_tree_given": bool(args.parent_tree)}

        def save():
            os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
            with open(out, "w") as f:
                json.dump(res, f, indent=1)
                f.write("\n")
        res["eventalign"] = eventalign_legs(args)
        save()
        res["kernels"] = kernels_against_parent(args)
        save()
        if args.parent_tree and args.bench_rounds > 0:
            res["bench"] = bench_alternating(args)
            save()
        print(json.dumps({k: (v if k != "eventalign" else {a: b for a, b in v.items() if a != "runs"}) for k, v in res.items()}))
        return
    legs = {"walk": [], "repr": [], "write": []}
    meta = {}
    for _ in range(args.rounds):
        w = run_child("walk", args.parent_tree, args)
        n = run_child("repr", None, args)
        legs["walk"].append(w["ms"]["walk"])
        legs["repr"].append(n["ms"]["repr"])
        legs["write"].append(n["ms"]["write"])
        meta = {"walk_lib": w["lib"], "walk_kernel": w["kernel"], "repr_lib": n["lib"], "repr_kernel": n["kernel"], "device": n["device"]}
    T = {k: statistics.median(v) for k, v in legs.items()}
    spread = max(legs["walk"]) - min(legs["walk"])
    reads = args.sites * BAG
    repr_bytes = reads * 32 * 4
    bar = T["walk"] + T["write"] + spread
    res = {"what": "m6a_read_representation against m6a_encode_reads (M6A_ENCODER=walk16) plus a device-to-device copy of repr",
           "shape": {"sites": args.sites, "reads_per_site": BAG, "reads": reads, "repr_bytes": repr_bytes},
           "rounds": args.rounds, "calls_per_leg": args.calls, **meta,
           "walk_is_parent_build": bool(args.parent_tree),
           "T_repr_ms": T["repr"], "T_walk_ms": T["walk"], "T_write_ms": T["write"], "T_walk_spread_ms": spread,
           "legs_ms": legs, "bar_ms": bar, "meets_bar": T["repr"] <= bar,
           "repr_write_rate_GBps": repr_bytes / (T["repr"] * 1e-3) / 1e9,
           "repr_write_rate_over_walk_GBps": repr_bytes / (max(T["repr"] - T["walk"], 1e-6) * 1e-3) / 1e9,
           "copy_rate_GBps_read_plus_write": 2 * repr_bytes / (T["write"] * 1e-3) / 1e9}
    if args.parent_tree and args.bench_rounds > 0:
        res["default_path"] = bench_alternating(args)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in res.items() if k != "legs_ms"}))


if __name__ == "__main__":
    main()
