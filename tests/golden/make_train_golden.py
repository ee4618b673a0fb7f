#!/usr/bin/env python3
"""Generate tests/golden/train_step.npz by IMPORTING the reference (the conventions of make_golden.py: its functions are called on
fixed inputs and inputs / outputs are stored as data; nothing of its source is copied).

    python tests/golden/make_train_golden.py

What the file pins: three steps of the reference's training loop body (m6anet/utils/training_utils.py:175-185) -- MILModel in
train mode from the HCT116 checkpoint, torch.nn.BCELoss (m6anet/utils/builder.py), torch.optim.Adam(lr=4e-4) as
m6anet/scripts/train.py:94 builds it -- on ONE batch of 8 sites x 20 reads: the first 20 reads of the first 8 sites of
bundled_inputs.npz, labels arange(8) % 2.
  X [8][20][9], kmer [8][3], y [8]        the batch
  loss [3], y_pred [3][8]                 of every step
  grad1 [7997]                            the gradient of step 1 in blob order (zeros in the running-statistic slots)
  blob1, blob3 [7997]                     the state_dict after steps 1 and 3 in blob order
"""
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("M6ANET_REFERENCE", "/root/reference")         # the reference checkout, as in make_golden.py

_shim = tempfile.mkdtemp(prefix="m6a_shims_")
with open(os.path.join(_shim, "toml.py"), "w") as f:
    f.write("import tomli\ndef load(p):\n    with open(p,'rb') as f:\n        return tomli.load(f)\n")
with open(os.path.join(_shim, "ujson.py"), "w") as f:
    f.write("from json import *\n")
sys.dont_write_bytecode = True
sys.path[:0] = [_shim, REF, REPO]

import numpy as np  # noqa: E402
import torch  # noqa: E402
import toml  # noqa: E402
from m6anet.model.model import MILModel  # noqa: E402
from m6anet.utils import constants as C  # noqa: E402

torch.set_num_threads(1)

ORDER = ["read_level_encoder.1.embedding_layer.weight", "read_level_encoder.3.layers.0.weight", "read_level_encoder.3.layers.0.bias",
         "read_level_encoder.3.layers.1.weight", "read_level_encoder.3.layers.1.bias", "read_level_encoder.3.layers.1.running_mean",
         "read_level_encoder.3.layers.1.running_var", "read_level_encoder.4.layers.0.weight", "read_level_encoder.4.layers.0.bias",
         "pooling_filter.probability_layer.0.weight", "pooling_filter.probability_layer.0.bias"]


def blob(sd):
    out = np.concatenate([sd[k].detach().cpu().numpy().astype(np.float32).ravel() for k in ORDER])
    assert out.size == 7997
    return out


def main():
    d = np.load(os.path.join(HERE, "bundled_inputs.npz"))
    off = d["off"]
    B, bag = 8, 20
    X = np.stack([d["X"][off[s]:off[s] + bag] for s in range(B)]).astype(np.float32)
    kmer = d["site_kmers"][:B].astype(np.uint8)
    y = (np.arange(B) % 2).astype(np.float32)
    model = MILModel(toml.load(C.DEFAULT_MODEL_CONFIG))
    model.load_state_dict(torch.load(C.DEFAULT_MODEL_WEIGHTS, map_location="cpu"))
    model.train()
    opt = torch.optim.Adam(model.parameters(), lr=4e-4)
    crit = torch.nn.BCELoss()
    batch = {"X": torch.from_numpy(X), "kmer": torch.from_numpy(np.repeat(kmer[:, None, :], bag, axis=1).astype(np.int64))}
    out = {"X": X, "kmer": kmer, "y": y, "loss": [], "y_pred": []}
    params = dict(model.named_parameters())
    for step in (1, 2, 3):
        y_pred = model({k: v for k, v in batch.items()})
        loss = crit(y_pred, torch.from_numpy(y))
        loss.backward()
        if step == 1:
            g = {k: params[k].grad if k in params else torch.zeros_like(v) for k, v in model.state_dict().items()}
            out["grad1"] = blob(g)
        opt.step()
        opt.zero_grad()
        out["loss"].append(np.float32(loss.item()))
        out["y_pred"].append(y_pred.detach().numpy().astype(np.float32))
        if step in (1, 3):
            out["blob%d" % step] = blob(model.state_dict())
        print("step", step, "loss", loss.item())
    out["loss"], out["y_pred"] = np.asarray(out["loss"], np.float32), np.stack(out["y_pred"])
    np.savez_compressed(os.path.join(HERE, "train_step.npz"), **out)
    print("wrote train_step.npz", os.path.getsize(os.path.join(HERE, "train_step.npz")), "bytes")


if __name__ == "__main__":
    main()
