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
    times = {k: [] for k in legs}
    for f in legs.values():                                      # warm-up: code objects, first touch of the outputs
        f()
    for _ in range(args.calls):
        for k, f in legs.items():
            times[k].append(f())
    out = {"lib": os.path.relpath(_lib.LIB_PATH, os.path.abspath(args.tree) if args.tree else REPO), "kernel": eng.last_encoder_kernel, "device": torch.cuda.get_device_name(0),
           "ms": {k: statistics.median(v) for k, v in times.items()}, "calls_ms": times}
    print("LEG " + json.dumps(out), flush=True)


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
    ap.add_argument("--child", choices=("walk", "repr"), default=None, help=argparse.SUPPRESS)
    ap.add_argument("--tree", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
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
