#!/usr/bin/env python3
"""What m6a_site_ranksum (include/m6a.h) costs beside the inference over the same reads, on resident inputs:

  legs     two synthetic conditions of the same shape are scored once (m6a_infer on device tensors), then the legs alternate on one
           context: `infer` = the two m6a_infer calls that produce the conditions' read probabilities (all the reads the test
           compares), `ranksum` = one m6a_site_ranksum over their read_prob arrays with the pair indices in device memory;
           per kind the median over all steps and the spread of the legs' medians.  Shapes: 1 M pairs of 20 + 20 reads (40 M reads)
           and 125 k pairs of 50..500 reads a side.
  bar      for the 20 + 20 shape: the ranksum median is no longer than the infer median plus the infer legs' own spread -- a
           statistic that costs more than the inference would be the new bottleneck.  The ragged shape carries no bar.
  command  `eventalign_diff` once on a generated eventalign file (--command_shape, default 3.1GB) as both conditions: wall time.

Writes one JSON file (default profiles/r31_site_ranksum.json).  Needs an MI355X; there is no fallback.  What a run leaves out
(--shapes, --no_command) is written down as "not measured"."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(1, os.path.join(REPO, "tools"))

SHAPES = {"uniform": ("HCT116_RNA002", 1_000_000, 20), "ragged": ("HEK293T_RNA004", 125_000, (50, 500))}
N_ITERS = 1000


def condition(shape, seed):
    import torch
    from m6anet_amd import synthetic
    _, S, bag = SHAPES[shape]
    d = synthetic.make_sites(S, bag, seed=seed)
    dev = torch.device("cuda:0")
    X, km, off = (torch.from_numpy(d[k]).to(dev) for k in ("X", "site_kmers", "off"))
    R = int(d["off"][-1])
    bufs = (torch.empty(R, dtype=torch.float32, device=dev), torch.empty(S, dtype=torch.float32, device=dev),
            torch.empty(S, dtype=torch.float64, device=dev))
    return {"off_host": d["off"], "inputs": (X, km, off), "bufs": bufs, "reads": R}


def summary(per_leg):
    flat = [t for l in per_leg for t in l]
    meds = [statistics.median(l) for l in per_leg]
    return {"median_ms": round(statistics.median(flat), 4), "leg_medians_ms": [round(m, 4) for m in meds],
            "spread_ms": round(max(meds) - min(meds), 4), "steps": len(flat)}


def measure_legs(shape, steps, warmup, legs):
    import numpy as np
    import torch
    from m6anet_amd.engine import M6ANetEngine, load_weights
    model, S, _ = SHAPES[shape]
    conds = [condition(shape, 20250328), condition(shape, 20250329)]
    eng = M6ANetEngine(weights=load_weights(model))
    eng.use_torch_stream()
    pair = torch.arange(S, dtype=torch.int64, device="cuda:0")
    out = [torch.empty(S, dtype=torch.int64, device="cuda:0") for _ in range(3)] + [torch.empty(S, dtype=torch.float64, device="cuda:0")]

    def infer_ms():
        t0 = time.perf_counter()
        for c in conds:
            eng.set_host_offsets(c["off_host"])
            eng.infer(*c["inputs"], N_ITERS, out=c["bufs"])
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def ranksum_ms():
        a, b = conds
        t0 = time.perf_counter()
        eng.site_ranksum_ptrs(a["bufs"][0].data_ptr(), a["inputs"][2].data_ptr(), S, b["bufs"][0].data_ptr(), b["inputs"][2].data_ptr(), S,
                              pair.data_ptr(), pair.data_ptr(), S, *[o.data_ptr() for o in out])
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    kinds = {"infer": infer_ms, "ranksum": ranksum_ms}
    times = {k: [] for k in kinds}
    for fn in kinds.values():
        for _ in range(warmup):
            fn()
    for _ in range(legs):
        for k, fn in kinds.items():
            times[k].append([fn() for _ in range(steps)])
    eng.sync()
    z = out[3].cpu().numpy()
    gt = out[0].cpu().numpy()
    eng.close()
    res = {k: summary(v) for k, v in times.items()}
    res["pairs"], res["reads"] = S, sum(c["reads"] for c in conds)
    res["ranksum_over_infer"] = round(res["ranksum"]["median_ms"] / res["infer"]["median_ms"], 4)
    res["defined_pairs"], res["pairs_beyond_z_3"] = int((gt >= 0).sum()), int((np.abs(z) > 3).sum())
    if shape == "uniform":
        res["bar_ms"] = round(res["infer"]["median_ms"] + res["infer"]["spread_ms"], 4)
        res["bar_met"] = res["ranksum"]["median_ms"] <= res["bar_ms"]
    return res


def measure_command(tag, limit):
    import measure_eventalign_inference as M
    with tempfile.TemporaryDirectory(prefix="m6a_ranksum_") as d:
        path, n = M.write_shape(tag, d)
        out = os.path.join(d, "out")
        env = dict(os.environ, PYTHONPATH=REPO)
        t, p = M.timed(["eventalign_diff", "--eventalign_a", path, "--eventalign_b", path, "--out_dir", out] + M.THREADS, limit, env=env)
        if p.returncode != 0:
            raise RuntimeError("eventalign_diff failed (%d): %s" % (p.returncode, p.stderr[-2000:]))
        rows = sum(1 for _ in open(os.path.join(out, "data.diff.csv"))) - 1
        return {"copies": n, "eventalign_GB": os.path.getsize(path) / 1e9, "wall_s": round(t, 3), "diff_rows": rows,
                "stdout": p.stdout.strip().splitlines()[-1]}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--legs", type=int, default=4, help="legs per kind")
    ap.add_argument("--shapes", default="uniform,ragged")
    ap.add_argument("--command_shape", default="3.1GB")
    ap.add_argument("--no_command", action="store_true")
    ap.add_argument("--timeout", type=int, default=600)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r31_site_ranksum.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("measure_ranksum: no HIP device visible; nothing is measured without one")
    res = {"n_iters": N_ITERS, "steps_per_leg": a.steps, "warmup": a.warmup, "device": torch.cuda.get_device_name(0),
           "shapes": {k: {"model": v[0], "pairs": v[1], "bag": v[2]} for k, v in SHAPES.items()}}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)

    def write():                             # after every part: a run that is cut short leaves what it measured
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")

    for shape in SHAPES:
        res[shape] = "not measured"
    res["command"] = "not measured"
    for shape in SHAPES:
        if shape in a.shapes.split(","):
            res[shape] = measure_legs(shape, a.steps, a.warmup, a.legs)
        print(shape, json.dumps(res[shape]), flush=True)
        write()
    if not a.no_command:
        res["command"] = measure_command(a.command_shape, a.timeout)
    print("command", json.dumps(res["command"]), flush=True)
    write()
    print("wrote", a.out)


if __name__ == "__main__":
    main()
