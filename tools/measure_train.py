#!/usr/bin/env python3
"""One training epoch, timed: 100 000 synthetic sites (m6anet_amd/synthetic.py shapes, 20 reads each), batch_size 256, bag 20, an
over-sampled order, through m6a_train_epoch with the data set resident in device memory -- and the same batches (the same read
indices, m6a_train_sample) through the float32 torch restatement of the model (tests/train_torch.py) on the CPUs this process is
granted.  Writes one JSON object (default profiles/r19_train_epoch.json).

    python tools/measure_train.py [--sites 100000] [--cpu_steps 100] [--clip_grad 1.0] [--out profiles/r19_train_epoch.json]

--clip_grad times the step with gradient clipping on (seven launches instead of six; the torch run clips with clip_grad_norm_).

The GPU figure is a host clock around the call and the stream synchronise behind it, the median of --repeats epochs after one warm-up
epoch (same trainer state at the start of each: a new trainer per epoch).  The CPU figure times --cpu_steps steps and scales to
the epoch; its batches are gathered outside the timed window, which favours it.  Needs an MI355X: without one it fails."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sites", type=int, default=100000)
    ap.add_argument("--batch_size", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--cpu_steps", type=int, default=100)
    ap.add_argument("--clip_grad", type=float, default=None, help="max_norm of gradient clipping; not set: the default step")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r19_train_epoch.json"))
    a = ap.parse_args()
    import torch
    import train_torch as TT
    from m6anet_amd import synthetic, training_utils as TU
    from m6anet_amd.engine import M6ANetEngine, init_weights, train_sample
    if not torch.cuda.is_available():
        raise SystemExit("measure_train.py: no GPU visible; nothing is measured on a CPU alone")
    bag, seed = 20, 25
    d = synthetic.make_sites(a.sites, bag)
    X, km, off = d["X"], d["site_kmers"], d["off"]
    g = np.random.Generator(np.random.PCG64(1))
    y = (g.random(a.sites) < 0.1).astype(np.float32)
    order = np.ascontiguousarray(TU.imbalance_over_sampler(y, np.random.RandomState(seed)), np.int64)
    n_steps = -(-len(order) // a.batch_size)
    w = init_weights(0)
    eng = M6ANetEngine(weights=w)
    dev = [torch.from_numpy(v).cuda() for v in (X, km, off, y, order)]
    times, stats = [], None
    for rep in range(a.repeats + 1):
        tr = eng.trainer(w, clip_grad=a.clip_grad) if a.clip_grad is not None else eng.trainer(w)
        s0 = tr.stats()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        loss, _ = tr.epoch(*dev, a.batch_size, bag, seed)
        eng.sync()
        dt = time.perf_counter() - t0
        s1 = tr.stats()
        if rep:
            times.append(dt)
        stats = {k: s1[k] - s0[k] for k in s1}
        last_loss = float(loss[-1])
        tr.close()
    gpu_s = statistics.median(times)

    idx = train_sample(off, order, bag, seed)
    k_steps = min(a.cpu_steps, n_steps)
    batches = []
    for k in range(k_steps):
        o = order[k * a.batch_size:(k + 1) * a.batch_size]
        batches.append((X[idx[k * a.batch_size * bag:(k + 1) * a.batch_size * bag]], km[o], y[o], bag))
    if a.clip_grad is None:
        cpu_run = lambda b: TT.run(w, b, torch.float32)
    else:
        import train_clip_torch as CT
        cpu_run = lambda b: CT.run(w, b, torch.float32, a.clip_grad)
    cpu_run(batches[:3])                                                    # warm-up
    t0 = time.perf_counter()
    cpu_run(batches)
    cpu_s = (time.perf_counter() - t0) / k_steps * n_steps
    res = {"clip_grad": a.clip_grad, "sites": a.sites, "order": int(len(order)), "batch_size": a.batch_size, "bag": bag, "steps": n_steps,
           "gpu_epoch_s": gpu_s, "gpu_epoch_s_all": times, "gpu_us_per_step": gpu_s / n_steps * 1e6,
           "launches_per_epoch": stats["n_launches"], "launches_per_step": (stats["n_launches"] - 2) / n_steps, "syncs_per_epoch": stats["n_syncs"],
           "cpu_threads": torch.get_num_threads(), "cpu_steps_timed": k_steps, "cpu_epoch_s_scaled": cpu_s, "cpu_us_per_step": cpu_s / n_steps * 1e6,
           "speedup": cpu_s / gpu_s, "last_step_loss": last_loss, "device": torch.cuda.get_device_name(0)}
    eng.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
