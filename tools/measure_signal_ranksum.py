#!/usr/bin/env python3
"""What m6a_site_signal_ranksum (include/m6a.h) costs beside nine calls of m6a_site_ranksum, on resident inputs:

  legs     two synthetic conditions of the same shape lie in device memory as X [R][9] (normal values, the three norm_mean columns
           rounded to 0.1 so that they tie as the real ones do) and, de-interleaved outside the clock, as nine contiguous columns.
           The legs alternate on one context: `signal` = one m6a_site_signal_ranksum on the two X, `nine` = nine m6a_site_ranksum
           calls, one per column copy (which flatters them: the copies are free).  Every step is timed by a pair of device events on
           the context's stream; per kind the median over all steps and the spread of the legs' medians.  The two must agree bit for
           bit before anything is timed.  Shapes: 1 M pairs of 20 + 20 reads and 125 k pairs of 50..500 reads a side.
  bar      per shape: the signal median is no longer than the nine calls' median plus their own spread -- the kernel makes the same
           compares and fetches each bag once.
  parent   --parent_root DIR (a built tree of the parent commit): m6a_site_ranksum itself, in alternating processes of this tree and
           that one, on both shapes (values uniform in [0, 1)); bar: this tree's median within the parent's median plus its spread.
  command  `eventalign_diff` without and with --signal, once each, on a generated eventalign file (--command_shape) as both
           conditions: wall time, no bar.

Writes one JSON file (default profiles/r32_signal_ranksum.json).  Needs an MI355X; there is no fallback.  What a run leaves out
(--shapes, no --parent_root, --no_command) is written down as "not measured"."""
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


def measure_legs(shape, steps, warmup, legs):
    import torch
    S = SHAPES[shape][0]
    eng = engine(REPO)
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(20250401)
    conds = []
    for seed in (1, 2):
        off = offsets(shape, seed)
        X = torch.randn((int(off[-1]), 9), generator=gen, device=dev, dtype=torch.float32)
        X[:, 2::3] = torch.round(X[:, 2::3] * 10) / 10
        conds.append({"X": X, "cols": X.t().contiguous(), "off": torch.from_numpy(off).to(dev), "rows": int(off[-1])})
    pair = torch.arange(S, dtype=torch.int64, device=dev)
    sig = [torch.empty(S * 9, dtype=torch.int64, device=dev) for _ in range(3)] + [torch.empty(S * 9, dtype=torch.float64, device=dev)]
    nine = [torch.empty((9, S), dtype=torch.int64, device=dev) for _ in range(3)] + [torch.empty((9, S), dtype=torch.float64, device=dev)]
    a, b = conds

    def signal():
        eng.site_signal_ranksum_ptrs(a["X"].data_ptr(), a["off"].data_ptr(), S, b["X"].data_ptr(), b["off"].data_ptr(), S, pair.data_ptr(),
                                     pair.data_ptr(), S, *[o.data_ptr() for o in sig])

    def nine_calls():
        for c in range(9):
            eng.site_ranksum_ptrs(a["cols"][c].data_ptr(), a["off"].data_ptr(), S, b["cols"][c].data_ptr(), b["off"].data_ptr(), S,
                                  pair.data_ptr(), pair.data_ptr(), S, *[o[c].data_ptr() for o in nine])

    signal()
    nine_calls()
    eng.sync()
    agree = all(torch.equal(s.view(S, 9).t().contiguous().view(torch.int64), n.view(torch.int64)) for s, n in zip(sig, nine))
    if not agree:
        raise RuntimeError("m6a_site_signal_ranksum and nine m6a_site_ranksum calls differ on the %s shape" % shape)
    res = run_legs({"signal": signal, "nine": nine_calls}, steps, warmup, legs)
    eng.sync()
    z = sig[3].cpu().numpy()
    eng.close()
    res["pairs"], res["rows"], res["agree_bit_for_bit"] = S, sum(c["rows"] for c in conds), agree
    res["signal_over_nine"] = round(res["signal"]["median_ms"] / res["nine"]["median_ms"], 4)
    res["columns_beyond_z_3"] = int((abs(z) > 3).sum())
    res["bar_ms"] = round(res["nine"]["median_ms"] + res["nine"]["spread_ms"], 4)
    res["bar_met"] = res["signal"]["median_ms"] <= res["bar_ms"]
    return res


def child(root, steps, warmup):
    """m6a_site_ranksum alone, from the tree at `root`: one JSON line {shape: [ms, ...]}"""
    import torch
    eng = engine(root)
    dev = torch.device("cuda:0")
    out = {}
    for shape, (S, _) in SHAPES.items():
        gen = torch.Generator(device=dev).manual_seed(20250402)
        offs = [offsets(shape, seed) for seed in (1, 2)]
        prob = [torch.rand(int(o[-1]), generator=gen, device=dev, dtype=torch.float32) for o in offs]
        offs = [torch.from_numpy(o).to(dev) for o in offs]
        pair = torch.arange(S, dtype=torch.int64, device=dev)
        res = [torch.empty(S, dtype=torch.int64, device=dev) for _ in range(3)] + [torch.empty(S, dtype=torch.float64, device=dev)]

        def ranksum():
            eng.site_ranksum_ptrs(prob[0].data_ptr(), offs[0].data_ptr(), S, prob[1].data_ptr(), offs[1].data_ptr(), S, pair.data_ptr(),
                                  pair.data_ptr(), S, *[o.data_ptr() for o in res])
        for _ in range(warmup):
            timed_ms(ranksum)
        out[shape] = [timed_ms(ranksum) for _ in range(steps)]
        eng.sync()
    eng.close()
    print("CHILD " + json.dumps(out), flush=True)


def measure_parent(parent_root, steps, warmup, rounds, limit):
    per = {"parent": {s: [] for s in SHAPES}, "this": {s: [] for s in SHAPES}}
    for _ in range(rounds):
        for name, root in (("parent", os.path.abspath(parent_root)), ("this", REPO)):
            p = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--child", root, "--steps", str(steps),
                                "--warmup", str(warmup)], capture_output=True, text=True, env=dict(os.environ, PYTHONPATH=root))
            if p.returncode != 0:
                raise RuntimeError("the %s process failed (%d): %s" % (name, p.returncode, p.stderr[-2000:]))
            got = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("CHILD ")][-1][6:])
            for s in SHAPES:
                per[name][s].append(got[s])
    res = {}
    for s in SHAPES:
        r = {name: summary(per[name][s]) for name in per}
        r["bar_ms"] = round(r["parent"]["median_ms"] + r["parent"]["spread_ms"], 4)
        r["bar_met"] = r["this"]["median_ms"] <= r["bar_ms"]
        res[s] = r
    return res


def measure_command(tag, limit):
    sys.path.insert(1, os.path.join(REPO, "tools"))
    import measure_eventalign_inference as M
    with tempfile.TemporaryDirectory(prefix="m6a_signal_ranksum_") as d:
        path, n = M.write_shape(tag, d)
        env = dict(os.environ, PYTHONPATH=REPO)
        res = {"copies": n, "eventalign_GB": os.path.getsize(path) / 1e9}
        for name, extra in (("without", []), ("with_signal", ["--signal"])):
            out = os.path.join(d, "out_" + name)
            t, p = M.timed(["eventalign_diff", "--eventalign_a", path, "--eventalign_b", path, "--out_dir", out] + extra + M.THREADS, limit, env=env)
            if p.returncode != 0:
                raise RuntimeError("eventalign_diff failed (%d): %s" % (p.returncode, p.stderr[-2000:]))
            res[name] = {"wall_s": round(t, 3), "files": sorted(os.listdir(out)), "stdout": p.stdout.strip().splitlines()[-1]}
        res["with_signal"]["signal_rows"] = sum(1 for _ in open(os.path.join(d, "out_with_signal", "data.diff_signal.csv"))) - 1
        return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--legs", type=int, default=4, help="legs per kind; with --parent_root, processes per tree")
    ap.add_argument("--shapes", default="uniform,ragged")
    ap.add_argument("--parent_root", default=None, help="a built tree of the parent commit (its m6anet_amd package)")
    ap.add_argument("--command_shape", default="3.1GB")
    ap.add_argument("--no_command", action="store_true")
    ap.add_argument("--timeout", type=int, default=600)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r32_signal_ranksum.json"))
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("measure_signal_ranksum: no HIP device visible; nothing is measured without one")
    if a.child:
        return child(a.child, a.steps, a.warmup)
    res = {"steps_per_leg": a.steps, "warmup": a.warmup, "device": torch.cuda.get_device_name(0), "timer": "device events on the context's stream",
           "shapes": {k: {"pairs": v[0], "bag": v[1]} for k, v in SHAPES.items()}}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)

    def write():                             # after every part: a run that is cut short leaves what it measured
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")

    for part in list(SHAPES) + ["site_ranksum_against_parent", "command"]:
        res[part] = "not measured"
    for shape in SHAPES:
        if shape in a.shapes.split(","):
            res[shape] = measure_legs(shape, a.steps, a.warmup, a.legs)
        print(shape, json.dumps(res[shape]), flush=True)
        write()
    if a.parent_root:
        res["site_ranksum_against_parent"] = measure_parent(a.parent_root, a.steps, a.warmup, a.legs, a.timeout)
    print("site_ranksum_against_parent", json.dumps(res["site_ranksum_against_parent"]), flush=True)
    write()
    if not a.no_command:
        res["command"] = measure_command(a.command_shape, a.timeout)
    print("command", json.dumps(res["command"]), flush=True)
    write()
    print("wrote", a.out)


if __name__ == "__main__":
    main()
