#!/usr/bin/env python3
"""What m6a_ks_exact (include/m6a.h) costs beside m6a_site_ks on the same pairs, on resident inputs, and that the calls it stands next to
did not move.  The conditions, the timer and the summaries are tools/measure_ks.py's.

  legs     two synthetic conditions of the same shape lie in device memory (read probabilities uniform in [0, 1)); m6a_site_ks runs once
           and h = max(d_pos, d_neg), n and m are formed on the device.  Two kinds alternate on one context: `ks` = m6a_site_ks on the
           probabilities and `ks_exact` = m6a_ks_exact on (n, m, h).  Every step is timed by a pair of device events on the context's
           stream; per kind the median over all steps and the spread of the legs' medians, their ratio, and the grid cells n m per
           second of the new call.  Before anything is timed p is held bit for bit to the host core (m6a_io_ks_exact) on the distinct
           items among the first --check_items.  Shapes: 1 M items of 20 + 20 reads and 125 k items of 50..500 reads a side.  The new
           kernel carries no speed bar.
  parent   --parent_root DIR (a built tree of the parent commit): m6a_site_ks and m6a_site_signal_ks, in alternating processes of this
           tree and that one, on both shapes; bar: this tree's median within the parent's median plus the parent's own spread.
  bench    with --parent_root: plain `bench.py --gpus 1` in alternating processes of the two trees, with --dump-outputs; bar as above on
           ms_per_step, and the dumped arrays byte-identical.

Writes one JSON file (default profiles/r34_ks_exact.json).  Needs an MI355X; there is no fallback.  What a run leaves out (--shapes, no
--parent_root, --no_bench) is written down as "not measured"."""
import argparse
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import measure_ks as MK  # noqa: E402

SHAPES = MK.SHAPES
CALLS = {c: MK.CALLS[c] for c in ("site_ks", "site_signal_ks")}


def measure_legs(shape, steps, warmup, legs, check_items):
    import numpy as np
    import torch
    S = SHAPES[shape][0]
    eng = MK.engine(REPO)
    from m6anet_amd import _io
    dev = torch.device("cuda:0")
    a, b = MK.conditions(shape, dev)
    pair = torch.arange(S, dtype=torch.int64, device=dev)
    i64, f64 = torch.int64, torch.float64
    ks = [torch.empty(S, dtype=dt, device=dev) for dt in (i64, i64, f64, f64)]

    def site_ks():
        eng.site_ks_ptrs(a["prob"].data_ptr(), a["off"].data_ptr(), S, b["prob"].data_ptr(), b["off"].data_ptr(), S, pair.data_ptr(),
                         pair.data_ptr(), S, *[o.data_ptr() for o in ks])

    site_ks()
    eng.sync()
    n, m = (a["off"][1:] - a["off"][:-1]).contiguous(), (b["off"][1:] - b["off"][:-1]).contiguous()
    h = torch.maximum(ks[0], ks[1]).contiguous()
    p = torch.empty(S, dtype=f64, device=dev)
    torch.cuda.synchronize()

    def ks_exact():
        eng.ks_exact_ptrs(n.data_ptr(), m.data_ptr(), h.data_ptr(), S, p.data_ptr())

    ks_exact()
    eng.sync()
    K = min(S, check_items)
    items = np.stack([x[:K].cpu().numpy() for x in (n, m, h)], axis=1)
    distinct, where = np.unique(items, axis=0, return_inverse=True)
    want = _io.ks_exact(distinct[:, 0], distinct[:, 1], distinct[:, 2])[where.ravel()]
    got = p[:K].cpu().numpy()
    if not MK.same_bits(got, want):
        raise RuntimeError("m6a_ks_exact differs from the host core")
    res = MK.run_legs({"ks": site_ks, "ks_exact": ks_exact}, steps, warmup, legs)
    eng.sync()
    eng.close()
    cells = int((n * m).sum().item())
    res.update(items=S, grid_cells=cells, p_min=float(np.nanmin(got)), p_nan=int(np.isnan(got).sum()),
               agree_with_host_core_bit_for_bit={"items_checked": K, "distinct": int(distinct.shape[0])})
    res["ks_exact_over_ks"] = round(res["ks_exact"]["median_ms"] / res["ks"]["median_ms"], 4)
    res["grid_cells_per_second"] = round(cells / (res["ks_exact"]["median_ms"] * 1e-3), 1)
    return res


def child(root, steps, warmup):
    """m6a_site_ks and m6a_site_signal_ks alone, from the tree at `root`: one JSON line {call: {shape: [ms, ...]}}"""
    import torch
    eng = MK.engine(root)
    dev = torch.device("cuda:0")
    out = {c: {} for c in CALLS}
    for shape, (S, _) in SHAPES.items():
        a, b = MK.conditions(shape, dev)
        pair = torch.arange(S, dtype=torch.int64, device=dev)
        for name, (key, W, n_int) in CALLS.items():
            method = getattr(eng, name + "_ptrs")
            res = [torch.empty(S * W, dtype=torch.int64 if i < n_int else torch.float64, device=dev) for i in range(4)]

            def run():
                method(a[key].data_ptr(), a["off"].data_ptr(), S, b[key].data_ptr(), b["off"].data_ptr(), S, pair.data_ptr(), pair.data_ptr(), S,
                       *[o.data_ptr() for o in res])
            for _ in range(warmup):
                MK.timed_ms(run)
            out[name][shape] = [MK.timed_ms(run) for _ in range(steps)]
            eng.sync()
        del a, b
    eng.close()
    print("CHILD " + json.dumps(out), flush=True)


def measure_parent(parent_root, steps, warmup, rounds, limit):
    per = {c: {s: {"parent": [], "this": []} for s in SHAPES} for c in CALLS}
    for _ in range(rounds):
        for name, root in (("parent", os.path.abspath(parent_root)), ("this", REPO)):
            q = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--child", root, "--steps", str(steps),
                                "--warmup", str(warmup)], capture_output=True, text=True, env=dict(os.environ, PYTHONPATH=root))
            if q.returncode != 0:
                raise RuntimeError("the %s process failed (%d): %s" % (name, q.returncode, q.stderr[-2000:]))
            got = json.loads([ln for ln in q.stdout.splitlines() if ln.startswith("CHILD ")][-1][6:])
            for c in CALLS:
                for s in SHAPES:
                    per[c][s][name].append(got[c][s])
    return {c: {s: MK.against(per[c][s]) for s in SHAPES} for c in CALLS}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--legs", type=int, default=4, help="legs per kind; with --parent_root, processes per tree")
    ap.add_argument("--shapes", default="uniform,ragged")
    ap.add_argument("--check_items", type=int, default=20_000, help="items of m6a_ks_exact held to the host core per shape")
    ap.add_argument("--parent_root", default=None, help="a built tree of the parent commit (its m6anet_amd package and bench.py)")
    ap.add_argument("--no_bench", action="store_true")
    ap.add_argument("--bench_steps", type=int, default=20)
    ap.add_argument("--bench_warmup", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=600)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r34_ks_exact.json"))
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("measure_ks_exact: no HIP device visible; nothing is measured without one")
    if a.child:
        return child(a.child, a.steps, a.warmup)
    res = {"steps_per_leg": a.steps, "warmup": a.warmup, "device": torch.cuda.get_device_name(0), "timer": "device events on the context's stream",
           "shapes": {k: {"items": v[0], "bag": v[1]} for k, v in SHAPES.items()}}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)

    def write():                             # after every part: a run that is cut short leaves what it measured
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")

    for part in list(SHAPES) + ["calls_against_parent", "bench_against_parent"]:
        res[part] = "not measured"
    for shape in SHAPES:
        if shape in a.shapes.split(","):
            res[shape] = measure_legs(shape, a.steps, a.warmup, a.legs, a.check_items)
        print(shape, json.dumps(res[shape]), flush=True)
        write()
    if a.parent_root:
        res["calls_against_parent"] = measure_parent(a.parent_root, a.steps, a.warmup, a.legs, a.timeout)
    print("calls_against_parent", json.dumps(res["calls_against_parent"]), flush=True)
    write()
    if a.parent_root and not a.no_bench:
        res["bench_against_parent"] = MK.measure_bench(a.parent_root, a.bench_steps, a.bench_warmup, a.legs, a.timeout)
    print("bench_against_parent", json.dumps(res["bench_against_parent"]), flush=True)
    write()
    print("wrote", a.out)


if __name__ == "__main__":
    main()
