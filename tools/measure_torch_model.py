#!/usr/bin/env python3
"""A training step at 256 x 20 with resident tensors, three ways, timed on one GPU:

  (a) module   the reference's loop on m6anet_amd.torch_model.MILModel: zero_grad, forward, BCELoss, backward, torch.optim.Adam.step
  (b) torch    the same loop on the pure-torch restatement of the model (tests/train_torch.Restated, float32) on the same GPU
  (c) step     Trainer.step on device tensors: the fused HIP step, its own BCELoss and Adam

--legs interleaved legs of each (a, b, c, a, b, c, ...), every leg --warmup untimed steps and then --steps timed ones under a host
clock that ends behind a stream synchronise.  Writes one JSON object (default profiles/r28_torch_model.json): per way the legs'
us per step, their median and spread (max - min), and the kernels the native library launches per step ((a): 8 -- the k-mer check, 3
forward, 4 backward; torch's own kernels for the loss, the copy of the weights and the optimizer come on top and are not counted).

    python tools/measure_torch_model.py [--legs 5] [--steps 300] [--warmup 30] [--out profiles/r28_torch_model.json]

Needs an MI355X: without one it fails."""
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
    ap.add_argument("--batch_size", type=int, default=256)
    ap.add_argument("--legs", type=int, default=5)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--ways", default="module,torch,step", help="which of the three to time, comma-separated")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r28_torch_model.json"))
    a = ap.parse_args()
    import torch
    import train_torch as TT
    from m6anet_amd import synthetic
    from m6anet_amd.engine import M6ANetEngine, init_weights
    from m6anet_amd.torch_model import MILModel
    if not torch.cuda.is_available():
        raise SystemExit("measure_torch_model.py: no GPU visible; nothing is measured on a CPU alone")
    B, bag = a.batch_size, 20
    d = synthetic.make_sites(B, bag)
    g = np.random.Generator(np.random.PCG64(1))
    y_host = (g.random(B) < 0.5).astype(np.float32)
    X = torch.from_numpy(np.ascontiguousarray(d["X"][:B * bag])).cuda()
    km8 = torch.from_numpy(np.ascontiguousarray(d["site_kmers"][:B])).cuda()
    km64 = km8.to(torch.int64)
    y = torch.from_numpy(y_host).cuda()
    X3 = X.view(B, bag, 9)
    w = init_weights(0)
    crit = torch.nn.BCELoss()

    model = MILModel(w).train()                              # its native contexts are made by its first forward
    opt_a = torch.optim.Adam(model.parameters(), lr=4e-4)
    plain = TT.Restated(w, torch.float32).cuda().train()
    opt_b = torch.optim.Adam(plain.parameters(), lr=4e-4)
    eng = M6ANetEngine(weights=w)
    eng.use_torch_stream()
    tr = eng.trainer(w)

    def step_a():
        opt_a.zero_grad()
        crit(model.forward_bags(X3, km64), y).backward()
        opt_a.step()

    def step_b():
        opt_b.zero_grad()
        crit(plain(X, km64, bag), y).backward()
        opt_b.step()

    def step_c():
        tr.step(X, km8, y, bag)

    ways = {k: v for k, v in {"module": step_a, "torch": step_b, "step": step_c}.items() if k in a.ways.split(",")}
    legs = {k: [] for k in ways}
    for _ in range(a.legs):
        for name, fn in ways.items():
            for _ in range(a.warmup):
                fn()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                fn()
            torch.cuda.synchronize()
            legs[name].append((time.perf_counter() - t0) / a.steps * 1e6)
    if "module" in ways:
        t = model._trainer()
        s0 = t.stats()
        step_a()
        s1 = t.stats()
    if "step" in ways:
        c0 = tr.stats()
        step_c()
        c1 = tr.stats()
    res = {"batch_size": B, "bag": bag, "legs": a.legs, "steps_per_leg": a.steps, "warmup_per_leg": a.warmup,
           "device": torch.cuda.get_device_name(0), "torch_version": torch.__version__}
    for name, v in legs.items():
        res[name] = {"us_per_step_legs": v, "us_per_step_median": statistics.median(v), "us_per_step_spread": max(v) - min(v)}
    if "module" in ways:
        res["module"]["native_launches_per_step"] = s1["n_launches"] - s0["n_launches"]
        res["module"]["waits_per_step"] = s1["n_syncs"] - s0["n_syncs"]
    if "step" in ways:
        res["step"]["native_launches_per_step"] = c1["n_launches"] - c0["n_launches"]
        res["step"]["waits_per_step"] = c1["n_syncs"] - c0["n_syncs"]
    if "module" in ways and "torch" in ways:
        res["module_faster_than_torch"] = res["module"]["us_per_step_median"] < res["torch"]["us_per_step_median"]
    tr.close()
    eng.close()
    model.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
