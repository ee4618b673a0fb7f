#!/usr/bin/env python3
"""What m6a_site_ks and m6a_site_signal_ks (include/m6a.h) cost beside the rank-sum calls on the same data, on resident inputs, and that
the calls which existed before them did not move:

  legs     two synthetic conditions of the same shape lie in device memory: read probabilities uniform in [0, 1) and X [R][9] (normal
           values, the three norm_mean columns rounded to 0.1 so that they tie as the real ones do).  Four kinds alternate on one
           context: `ks` = m6a_site_ks and `ranksum` = m6a_site_ranksum on the probabilities, `signal_ks` = m6a_site_signal_ks and
           `signal_ranksum` = m6a_site_signal_ranksum on the two X.  Every step is timed by a pair of device events on the context's
           stream; per kind the median over all steps and the spread of the legs' medians, and the ratio of either new call to its
           rank-sum twin.  Before anything is timed the new calls' outputs are held bit for bit to the host core (m6a_io_site_ks on
           every pair; m6a_io_site_signal_ks on the first --check_pairs pairs).  Shapes: 1 M pairs of 20 + 20 reads and 125 k pairs of
           50..500 reads a side.  The new kernels carry no speed bar.
  parent   --parent_root DIR (a built tree of the parent commit): the four calls themselves, in alternating processes of this tree and
           that one, on both shapes; bar: this tree's median within the parent's median plus the parent's own spread.
  bench    with --parent_root: plain `bench.py --gpus 1` in alternating processes of the two trees, with --dump-outputs; bar as above on
           ms_per_step, and the dumped arrays byte-identical.

Writes one JSON file (default profiles/r33_site_ks.json).  Needs an MI355X; there is no fallback.  What a run leaves out (--shapes, no
--parent_root, --no_bench) is written down as "not measured"."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = {"uniform": (1_000_000, 20), "ragged": (125_000, (50, 500))}
MODEL = "HCT116_RNA002"
CALLS = {"site_ranksum": ("prob", 1, 3), "site_signal_ranksum": ("X", 9, 3), "site_ks": ("prob", 1, 2),
         "site_signal_ks": ("X", 9, 2)}     # the engine's *_ptrs method: (input, values per pair, how many of the four outputs are int64)


def offsets(shape, seed):
    import numpy as np
    S, bag = SHAPES[shape]
    g = np.random.Generator(np.random.PCG64(seed))
    n = g.integers(bag[0], bag[1] + 1, size=S) if isinstance(bag, tuple) else np.full(S, bag)
    return np.concatenate([[0], np.cumsum(n)]).astype(np.int64)


def summary(per_leg):
    flat = [t for l in per_leg for t in l]
    meds = [statistics.median(l) for l in per_leg]
    return {"median_ms": round(statistics.median(flat), 4), "leg_medians_ms": [round(m, 4) for m in meds],
            "spread_ms": round(max(meds) - min(meds), 4), "steps": len(flat)}


def timed_ms(fn):
    """one call of fn between two device events on the current stream"""
    import torch
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1)


def run_legs(kinds, steps, warmup, legs):
    times = {k: [] for k in kinds}
    for fn in kinds.values():
        for _ in range(warmup):
            timed_ms(fn)
    for _ in range(legs):
        for k, fn in kinds.items():
            times[k].append([timed_ms(fn) for _ in range(steps)])
    return {k: summary(v) for k, v in times.items()}


def engine(root):
    sys.path.insert(0, root)
    from m6anet_amd.engine import M6ANetEngine, load_weights
    eng = M6ANetEngine(weights=load_weights(MODEL))
    eng.use_torch_stream()
    return eng


def conditions(shape, dev):
    """two conditions of the shape in device memory: prob [R], X [R][9], off [S + 1]"""
    import torch
    gen = torch.Generator(device=dev).manual_seed(20250501)
    out = []
    for seed in (1, 2):
        off = offsets(shape, seed)
        X = torch.randn((int(off[-1]), 9), generator=gen, device=dev, dtype=torch.float32)
        X[:, 2::3] = torch.round(X[:, 2::3] * 10) / 10
        prob = torch.rand(int(off[-1]), generator=gen, device=dev, dtype=torch.float32)
        out.append({"X": X, "prob": prob, "off": torch.from_numpy(off).to(dev), "host_off": off})
    return out


def same_bits(got, want):
    import numpy as np
    got, want = np.ascontiguousarray(got).ravel(), np.ascontiguousarray(want).ravel()
    if want.dtype.kind != "f":
        return bool(np.array_equal(got, want))
    nan = np.isnan(want)
    return bool(np.array_equal(nan, np.isnan(got)) and np.array_equal(got[~nan].view(np.uint64), want[~nan].view(np.uint64)))


def host_check(a, b, S, ks, sks, check_pairs):
    """the two new calls' outputs against libm6a_io.so's host core, bit for bit"""
    import numpy as np
    from m6anet_amd import _io
    L = _io.load()
    ptr = lambda x: x.ctypes.data    # noqa: E731
    oa, ob = a["host_off"], b["host_off"]
    pa, pb = a["prob"].cpu().numpy(), b["prob"].cpu().numpy()
    want = [np.empty(S, np.int64), np.empty(S, np.int64), np.empty(S, np.float64), np.empty(S, np.float64)]
    if L.m6a_io_site_ks(ptr(pa), ptr(oa), S, ptr(pb), ptr(ob), S, None, None, S, *[ptr(w) for w in want], 0):
        raise RuntimeError("m6a_io_site_ks failed")
    if not all(same_bits(g.cpu().numpy(), w) for g, w in zip(ks, want)):
        raise RuntimeError("m6a_site_ks differs from the host core")
    K = min(S, check_pairs)
    oa, ob = np.ascontiguousarray(oa[:K + 1]), np.ascontiguousarray(ob[:K + 1])
    Xa, Xb = a["X"][:int(oa[-1])].cpu().numpy(), b["X"][:int(ob[-1])].cpu().numpy()
    want = [np.empty(K * 9, np.int64), np.empty(K * 9, np.int64), np.empty(K * 9, np.float64), np.empty(K * 9, np.float64)]
    if L.m6a_io_site_signal_ks(ptr(Xa), ptr(oa), K, ptr(Xb), ptr(ob), K, None, None, K, *[ptr(w) for w in want], 0):
        raise RuntimeError("m6a_io_site_signal_ks failed")
    if not all(same_bits(g[:K * 9].cpu().numpy(), w) for g, w in zip(sks, want)):
        raise RuntimeError("m6a_site_signal_ks differs from the host core")
    return {"site_ks_pairs_checked": S, "site_signal_ks_pairs_checked": K}


def measure_legs(shape, steps, warmup, legs, check_pairs):
    import torch
    S = SHAPES[shape][0]
    eng = engine(REPO)
    dev = torch.device("cuda:0")
    a, b = conditions(shape, dev)
    pair = torch.arange(S, dtype=torch.int64, device=dev)
    i64, f64 = torch.int64, torch.float64
    ks = [torch.empty(S, dtype=dt, device=dev) for dt in (i64, i64, f64, f64)]
    rs = [torch.empty(S, dtype=dt, device=dev) for dt in (i64, i64, i64, f64)]
    sks = [torch.empty(S * 9, dtype=dt, device=dev) for dt in (i64, i64, f64, f64)]
    srs = [torch.empty(S * 9, dtype=dt, device=dev) for dt in (i64, i64, i64, f64)]

    def call(method, key, out):
        return lambda: method(a[key].data_ptr(), a["off"].data_ptr(), S, b[key].data_ptr(), b["off"].data_ptr(), S, pair.data_ptr(),
                              pair.data_ptr(), S, *[o.data_ptr() for o in out])

    kinds = {"ks": call(eng.site_ks_ptrs, "prob", ks), "ranksum": call(eng.site_ranksum_ptrs, "prob", rs),
             "signal_ks": call(eng.site_signal_ks_ptrs, "X", sks), "signal_ranksum": call(eng.site_signal_ranksum_ptrs, "X", srs)}
    for fn in kinds.values():
        fn()
    eng.sync()
    checked = host_check(a, b, S, ks, sks, check_pairs)
    res = run_legs(kinds, steps, warmup, legs)
    eng.sync()
    eng.close()
    res["pairs"], res["reads"], res["agree_with_host_core_bit_for_bit"] = S, int(a["host_off"][-1] + b["host_off"][-1]), checked
    res["ks_over_ranksum"] = round(res["ks"]["median_ms"] / res["ranksum"]["median_ms"], 4)
    res["signal_ks_over_signal_ranksum"] = round(res["signal_ks"]["median_ms"] / res["signal_ranksum"]["median_ms"], 4)
    return res


def child(root, steps, warmup):
    """the four calls alone, from the tree at `root`: one JSON line {call: {shape: [ms, ...]}}"""
    import torch
    eng = engine(root)
    dev = torch.device("cuda:0")
    out = {c: {} for c in CALLS}
    for shape, (S, _) in SHAPES.items():
        a, b = conditions(shape, dev)
        pair = torch.arange(S, dtype=torch.int64, device=dev)
        for name, (key, W, n_int) in CALLS.items():
            method = getattr(eng, name + "_ptrs")
            res = [torch.empty(S * W, dtype=torch.int64 if i < n_int else torch.float64, device=dev) for i in range(4)]

            def run():
                method(a[key].data_ptr(), a["off"].data_ptr(), S, b[key].data_ptr(), b["off"].data_ptr(), S, pair.data_ptr(), pair.data_ptr(), S,
                       *[o.data_ptr() for o in res])
            for _ in range(warmup):
                timed_ms(run)
            out[name][shape] = [timed_ms(run) for _ in range(steps)]
            eng.sync()
        del a, b
    eng.close()
    print("CHILD " + json.dumps(out), flush=True)


def against(per):
    """{"parent": [[ms, ...] per process], "this": ...} -> the two summaries and the bar"""
    r = {name: summary(per[name]) for name in per}
    r["bar_ms"] = round(r["parent"]["median_ms"] + r["parent"]["spread_ms"], 4)
    r["bar_met"] = r["this"]["median_ms"] <= r["bar_ms"]
    return r


def measure_parent(parent_root, steps, warmup, rounds, limit):
    per = {c: {s: {"parent": [], "this": []} for s in SHAPES} for c in CALLS}
    for _ in range(rounds):
        for name, root in (("parent", os.path.abspath(parent_root)), ("this", REPO)):
            p = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--child", root, "--steps", str(steps),
                                "--warmup", str(warmup)], capture_output=True, text=True, env=dict(os.environ, PYTHONPATH=root))
            if p.returncode != 0:
                raise RuntimeError("the %s process failed (%d): %s" % (name, p.returncode, p.stderr[-2000:]))
            got = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("CHILD ")][-1][6:])
            for c in CALLS:
                for s in SHAPES:
                    per[c][s][name].append(got[c][s])
    return {c: {s: against(per[c][s]) for s in SHAPES} for c in CALLS}


def measure_bench(parent_root, steps, warmup, rounds, limit):
    per = {"parent": [], "this": []}
    dumps = {}
    with tempfile.TemporaryDirectory(prefix="m6a_ks_bench_") as d:
        for r in range(rounds):
            for name, root in (("parent", os.path.abspath(parent_root)), ("this", REPO)):
                out = os.path.join(d, "%s_%d" % (name, r))
                p = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", str(steps),
                                    "--warmup", str(warmup), "--dump-outputs", out], capture_output=True, text=True, cwd=root,
                                   env=dict(os.environ, PYTHONPATH=root))
                if p.returncode != 0:
                    raise RuntimeError("bench.py of the %s tree failed (%d): %s" % (name, p.returncode, p.stderr[-2000:]))
                line = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
                per[name].append([line["ms_per_step"]])
                dumps[name, r] = {fn: open(os.path.join(out, fn), "rb").read() for fn in sorted(os.listdir(out))}
    res = against(per)
    first = dumps["parent", 0]
    res["dumped_arrays"] = sorted(first)
    res["dump_outputs_byte_identical"] = bool(first) and all(v == first for v in dumps.values())
    res["timer"] = "bench.py's ms_per_step, one value per process"
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--legs", type=int, default=4, help="legs per kind; with --parent_root, processes per tree")
    ap.add_argument("--shapes", default="uniform,ragged")
    ap.add_argument("--check_pairs", type=int, default=50_000, help="pairs of m6a_site_signal_ks held to the host core per shape")
    ap.add_argument("--parent_root", default=None, help="a built tree of the parent commit (its m6anet_amd package and bench.py)")
    ap.add_argument("--no_bench", action="store_true")
    ap.add_argument("--bench_steps", type=int, default=20)
    ap.add_argument("--bench_warmup", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=600)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r33_site_ks.json"))
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("measure_ks: no HIP device visible; nothing is measured without one")
    if a.child:
        return child(a.child, a.steps, a.warmup)
    res = {"steps_per_leg": a.steps, "warmup": a.warmup, "device": torch.cuda.get_device_name(0), "timer": "device events on the context's stream",
           "shapes": {k: {"pairs": v[0], "bag": v[1]} for k, v in SHAPES.items()}}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)

    def write():                             # after every part: a run that is cut short leaves what it measured
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")

    for part in list(SHAPES) + ["calls_against_parent", "bench_against_parent"]:
        res[part] = "not measured"
    for shape in SHAPES:
        if shape in a.shapes.split(","):
            res[shape] = measure_legs(shape, a.steps, a.warmup, a.legs, a.check_pairs)
        print(shape, json.dumps(res[shape]), flush=True)
        write()
    if a.parent_root:
        res["calls_against_parent"] = measure_parent(a.parent_root, a.steps, a.warmup, a.legs, a.timeout)
    print("calls_against_parent", json.dumps(res["calls_against_parent"]), flush=True)
    write()
    if a.parent_root and not a.no_bench:
        res["bench_against_parent"] = measure_bench(a.parent_root, a.bench_steps, a.bench_warmup, a.legs, a.timeout)
    print("bench_against_parent", json.dumps(res["bench_against_parent"]), flush=True)
    write()
    print("wrote", a.out)


if __name__ == "__main__":
    main()
