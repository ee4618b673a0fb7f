#!/usr/bin/env python3
"""What `--site_proba expected` (m6a_set_site_mode, include/m6a.h) costs and saves, on resident inputs:

  legs        the step (one m6a_infer on device tensors, host offsets handed over, as bench.py's) at the headline shape
              (1 M sites x 20 reads) and at the ragged shape (125 k sites of 50..500 reads), in both modes, as interleaved legs on one
              context: sampled, expected, sampled, ...; per mode the median over all steps and the spread of the legs' medians
  first_call  the first call on a fresh context in both modes, wall time from before m6a_create to the synchronised result
  parent      the default mode of THIS tree against a built checkout of the parent commit (--parent-tree: its m6anet_amd/ with
              libm6a_hip.so in it, and include/), each in processes of its own, alternating; the bar for "no regression" is the parent's median plus
              the parent's own spread (largest - smallest of its processes' medians)

Writes one JSON file (default profiles/r22_site_expectation.json).  Needs an MI355X; there is no fallback."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.environ.get("M6A_MEASURE_TREE") or REPO)          # a child of the comparison imports the tree it measures

SHAPES = {"uniform": ("HCT116_RNA002", 1_000_000, 20), "ragged": ("HEK293T_RNA004", 125_000, (50, 500))}
N_ITERS = 1000


def resident(shape):
    import torch
    from m6anet_amd import synthetic
    model, S, bag = SHAPES[shape]
    d = synthetic.make_sites(S, bag, seed=20250328)
    dev = torch.device("cuda:0")
    X, km, off = (torch.from_numpy(d[k]).to(dev) for k in ("X", "site_kmers", "off"))
    R = int(d["off"][-1])
    bufs = (torch.empty(R, dtype=torch.float32, device=dev), torch.empty(S, dtype=torch.float32, device=dev),
            torch.empty(S, dtype=torch.float64, device=dev))
    return model, d["off"], (X, km, off), bufs


def step_ms(eng, off_host, inputs, bufs):
    import torch
    eng.set_host_offsets(off_host)
    t0 = time.perf_counter()
    eng.infer(*inputs, N_ITERS, out=bufs)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def leg(eng, off_host, inputs, bufs, steps):
    return [step_ms(eng, off_host, inputs, bufs) for _ in range(steps)]


def summary(per_leg):
    flat = [t for l in per_leg for t in l]
    meds = [statistics.median(l) for l in per_leg]
    return {"median_ms": round(statistics.median(flat), 4), "leg_medians_ms": [round(m, 4) for m in meds],
            "spread_ms": round(max(meds) - min(meds), 4), "steps": len(flat)}


def measure_legs(shape, steps, warmup, legs):
    from m6anet_amd.engine import M6ANetEngine, load_weights
    model, off_host, inputs, bufs = resident(shape)
    eng = M6ANetEngine(weights=load_weights(model))
    eng.use_torch_stream()
    times, variant = {"sampled": [], "expected": []}, {}
    for mode in ("sampled", "expected"):                    # every kernel and table of both modes before the first timed leg
        eng.set_site_mode(mode)
        leg(eng, off_host, inputs, bufs, warmup)
        variant[mode] = eng.last_pool_variant
    for _ in range(legs):
        for mode in ("sampled", "expected"):
            eng.set_site_mode(mode)
            times[mode].append(leg(eng, off_host, inputs, bufs, steps))
    eng.close()
    out = {m: dict(summary(times[m]), pool_variant=variant[m]) for m in times}
    out["expected_over_sampled"] = round(out["expected"]["median_ms"] / out["sampled"]["median_ms"], 4)
    first = {}
    for mode in ("sampled", "expected"):
        t0 = time.perf_counter()
        eng = M6ANetEngine(weights=load_weights(model))
        eng.use_torch_stream()
        if mode == "expected":
            eng.set_site_mode(mode)
        first[mode] = {"create_to_first_result_ms": round((time.perf_counter() - t0) * 1e3 + step_ms(eng, off_host, inputs, bufs), 3),
                       "second_call_ms": round(step_ms(eng, off_host, inputs, bufs), 3)}
        eng.close()
    return {"legs": out, "first_call": first}


def child(steps, warmup):
    """one process, the default mode at the headline shape: prints {"median_ms", "min_ms", "max_ms", "lib"}"""
    from m6anet_amd import _lib
    from m6anet_amd.engine import M6ANetEngine, load_weights
    model, off_host, inputs, bufs = resident("uniform")
    eng = M6ANetEngine(weights=load_weights(model))
    eng.use_torch_stream()
    leg(eng, off_host, inputs, bufs, warmup)
    t = leg(eng, off_host, inputs, bufs, steps)
    eng.close()
    print("M6A_CHILD " + json.dumps({"median_ms": round(statistics.median(t), 4), "min_ms": round(min(t), 4), "max_ms": round(max(t), 4),
                                     "lib": _lib.LIB_PATH}), flush=True)


def measure_parent(parent_tree, steps, warmup, pairs):
    runs = {"parent": [], "this": []}
    for _ in range(pairs):
        for who, tree in (("parent", os.path.abspath(parent_tree)), ("this", REPO)):
            env = dict(os.environ, M6A_MEASURE_TREE=tree)
            env.pop("M6A_HIP_LIB", None)
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--steps", str(steps), "--warmup", str(warmup)],
                               env=env, capture_output=True, text=True, timeout=900)
            if r.returncode != 0:
                raise RuntimeError("child (%s) failed: %s" % (who, r.stderr[-2000:]))
            line = [l for l in r.stdout.splitlines() if l.startswith("M6A_CHILD ")][-1]
            runs[who].append(json.loads(line[len("M6A_CHILD "):]))
    out = {}
    for who in runs:
        meds = [x["median_ms"] for x in runs[who]]
        assert all(os.path.dirname(os.path.dirname(x["lib"])) == (os.path.abspath(parent_tree) if who == "parent" else REPO) for x in runs[who])
        out[who] = {"median_ms": round(statistics.median(meds), 4), "process_medians_ms": meds, "spread_ms": round(max(meds) - min(meds), 4)}
    out["bar_ms"] = round(out["parent"]["median_ms"] + out["parent"]["spread_ms"], 4)
    out["no_regression"] = out["this"]["median_ms"] <= out["bar_ms"]
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--legs", type=int, default=4, help="legs per mode")
    ap.add_argument("--pairs", type=int, default=3, help="processes per tree in the comparison with --parent-tree")
    ap.add_argument("--parent-tree", default=None, help="a built checkout of the parent commit (m6anet_amd/ and include/ are enough)")
    ap.add_argument("--shapes", default="uniform,ragged")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r22_site_expectation.json"))
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        child(a.steps, a.warmup)
        return
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("measure_site_mode: no HIP device visible; nothing is measured without one")
    res = {"n_iters": N_ITERS, "steps_per_leg": a.steps, "warmup": a.warmup, "device": torch.cuda.get_device_name(0),
           "shapes": {k: {"model": v[0], "sites": v[1], "bag": v[2]} for k, v in SHAPES.items()}}
    for shape in a.shapes.split(","):
        res[shape] = measure_legs(shape, a.steps, a.warmup, a.legs)
        print(shape, json.dumps(res[shape]["legs"]), flush=True)
    res["default_mode_against_parent"] = measure_parent(a.parent_tree, a.steps, a.warmup, a.pairs) if a.parent_tree else "not measured"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res["default_mode_against_parent"]))
    print("wrote", a.out)


if __name__ == "__main__":
    main()
