"""`train` sub-command: the flags and the loop of `m6anet train` (m6anet/scripts/train.py:14-131), with the step -- training-mode
forward, backward pass, Adam -- in HIP on an MI355X (include/m6a.h: m6a_train_epoch) and the data set loaded once."""
import hashlib
import json
import os
import shutil
import sys
from argparse import ArgumentDefaultsHelpFormatter, ArgumentParser

import numpy as np

from ..constants import DEFAULT_PRETRAINED_MODELS, N_WEIGHT_FLOATS

DESCRIPTION = """Fits the m6anet.toml model.  --train_config is the reference's TOML file: [loss_function] loss_function_type =
"binary_cross_entropy_loss"; [dataset] root_dir (data.json, data.info and data.info.labelled with the columns modification_status
and set_type = Train | Val | Test), min_reads, norm_path (required), num_neighboring_features = 1; [dataloader.train] batch_size and
sampler = "ImbalanceOverSampler" | "ImbalanceUnderSampler" or shuffle; [dataloader.val] / [dataloader.test] are read for their presence
only (validation runs over the whole split at once).
Differences from the reference's files: train_info.json, train_results.json and val_results.json are JSON where it writes
train_info.toml and joblib files; every checkpoint is model_states/<epoch>/model_states.bin (the flat blob that `inference
--model_state_dict x.bin` takes) and, when torch can be imported, model_states.pt with the reference's state_dict keys beside it; the best
saved epoch by avg_loss, roc_auc and pr_auc is copied to <criterion>.bin (and .pt) and its test metrics are printed and stored as
test_results_<criterion>.json (the reference: .joblib).  Every checkpoint also holds trainer_state.npz -- Adam's m, v and step count,
the sampler's RandomState, the result lists so far and a fingerprint of the run's settings and sites -- and the two result files are
rewritten at every checkpoint; --resume continues the run in --save_dir from its last checkpoint with the bits of a run that was
never interrupted, and refuses a run whose seed, hyper-parameters or Train / Val sites have changed.
The reads of a site are drawn by a counter-based rule (include/m6a.h), not by the reference's DataLoader workers; --n_processes sizes
the loader's threads.  Not built: the weighted loss, the per-motif samplers, more than one GPU."""


def argparser():
    parser = ArgumentParser(formatter_class=ArgumentDefaultsHelpFormatter, add_help=False, description=DESCRIPTION)
    parser.add_argument("--model_config", default=None, help="accepted for compatibility; only the m6anet.toml topology is supported.")
    parser.add_argument("--train_config", required=True, help="path to training config file.")
    parser.add_argument("--save_dir", required=True, help="directory to output training results.")
    parser.add_argument("--device", default="cuda:0", type=str, help="GPU to train on (cuda:N / hip:N). There is no CPU path.")
    parser.add_argument("--lr", default=4e-4, type=float, help="training learning rate.")
    parser.add_argument("--seed", default=25, type=int, help="random seed for training.")
    parser.add_argument("--epochs", default=50, type=int, help="number of training epochs")
    parser.add_argument("--n_processes", default=25, type=int, help="threads of the data loader.")
    parser.add_argument("--save_per_epoch", default=10, type=int, help="number of epoch multiple to save training checkpoint.")
    parser.add_argument("--weight_decay", default=0, type=float, help="weight decay argument to regularize training.")
    parser.add_argument("--num_iterations", default=5, type=int, help="number of pass during evaluation step")
    parser.add_argument("--init", default=None,
                        help="fine-tune instead of starting from init_weights(seed): a pretrained model name (%s), a flat .bin blob or a "
                             "reference .pt checkpoint (needs torch)." % ", ".join(DEFAULT_PRETRAINED_MODELS))
    parser.add_argument("--clip_grad", default=None, type=float,
                        help="clip the gradient's 2-norm to this value before Adam (torch's clip_grad_norm_); not set: no clipping.")
    parser.add_argument("--resume", default=False, action="store_true",
                        help="continue the run in --save_dir from its highest epoch with a trainer_state.npz; --epochs is the total.")
    return parser


class Refusal(Exception):
    pass


def initial_weights(init, seed):
    from ..engine import init_weights, load_weights, weights_from_state_dict
    if init is None:
        return init_weights(seed)
    if init in DEFAULT_PRETRAINED_MODELS:
        return load_weights(init)
    if not os.path.isfile(init):
        raise Refusal("--init %s: not a pretrained model name (%s) and not a file" % (init, ", ".join(DEFAULT_PRETRAINED_MODELS)))
    if str(init).endswith(".bin"):
        w = np.fromfile(init, np.float32)
        if w.size != N_WEIGHT_FLOATS:
            raise Refusal("--init %s holds %d floats, expected %d (layout in include/m6a.h)" % (init, w.size, N_WEIGHT_FLOATS))
        return w
    import torch
    return weights_from_state_dict(torch.load(init, map_location="cpu", weights_only=True))


# what must not change across --resume: the run's settings and its Train / Val sites
FINGERPRINT_KEYS = ("seed", "lr", "weight_decay", "batch_size", "sampler", "min_reads", "clip_grad", "save_per_epoch", "num_iterations",
                    "sites_sha256")
RESULT_KEYS = ("compute_time", "avg_loss", "roc_auc", "pr_auc")          # the per-epoch scalars of both result dictionaries
STATE_FILE = "trainer_state.npz"


def sampler_name(train_loader_config):
    """The name get_sampler's choice goes by in a fingerprint."""
    if train_loader_config.get("sampler") is not None:
        return str(train_loader_config["sampler"])
    return "shuffle" if train_loader_config.get("shuffle", False) else "in_order"


def sites_hash(rows):
    """SHA-256 over the Train, then the Val rows' (transcript, position, label) in file order: the sites an epoch's order and the
    validation metrics are made of."""
    h = hashlib.sha256()
    for split in ("Train", "Val"):
        for r in rows:
            if r[4] == split:
                h.update(("%s\t%s\t%d\t%d\n" % (split, r[0], r[1], r[3])).encode("utf-8"))
    return h.hexdigest()


def fingerprint(args, loader_config, batch_size, min_reads, rows):
    return {"seed": int(args.seed), "lr": float(args.lr), "weight_decay": float(args.weight_decay), "batch_size": int(batch_size),
            "sampler": sampler_name(loader_config), "min_reads": int(min_reads),
            "clip_grad": None if args.clip_grad is None else float(args.clip_grad), "save_per_epoch": int(args.save_per_epoch),
            "num_iterations": int(args.num_iterations), "sites_sha256": sites_hash(rows)}


def save_trainer_state(path, checkpoint, fp):
    """trainer_state.npz: Adam's m, v and t, the epoch, the five fields of the sampler's RandomState.get_state(), the scalar result
    lists so far (train_<key>, val_<key>; not the bulky y_pred) and the fingerprint as JSON.  Written beside and renamed into place."""
    opt, rs = checkpoint["optimizer"], checkpoint["rs_state"]
    arrays = {"m": np.asarray(opt["m"], np.float32), "v": np.asarray(opt["v"], np.float32), "n_steps": np.int64(opt["n_steps"]),
              "epoch": np.int64(checkpoint["epoch"]), "rs_name": np.array(str(rs[0])), "rs_keys": np.asarray(rs[1], np.uint32),
              "rs_pos": np.int64(rs[2]), "rs_has_gauss": np.int64(rs[3]), "rs_cached_gaussian": np.float64(rs[4]),
              "fingerprint": np.array(json.dumps(fp, sort_keys=True))}
    for name, res in (("train", checkpoint["train_results"]), ("val", checkpoint["val_results"])):
        for k in RESULT_KEYS:
            arrays["%s_%s" % (name, k)] = np.asarray(res[k], np.float64)
    with open(path + ".tmp", "wb") as f:
        np.savez(f, **arrays)
    os.replace(path + ".tmp", path)


def load_trainer_state(path):
    """-> {"optimizer", "epoch", "rs_state", "train_results", "val_results" (the scalar lists), "fingerprint"}"""
    with np.load(path, allow_pickle=False) as z:
        rs_state = (str(z["rs_name"]), np.array(z["rs_keys"], np.uint32), int(z["rs_pos"]), int(z["rs_has_gauss"]), float(z["rs_cached_gaussian"]))
        out = {"optimizer": {"m": np.array(z["m"], np.float32), "v": np.array(z["v"], np.float32), "n_steps": int(z["n_steps"])},
               "epoch": int(z["epoch"]), "rs_state": rs_state, "fingerprint": json.loads(str(z["fingerprint"]))}
        for name in ("train", "val"):
            out[name + "_results"] = {k: [float(x) for x in z["%s_%s" % (name, k)]] for k in RESULT_KEYS}
    return out


def find_checkpoint(save_dir):
    """The highest epoch of save_dir/model_states that holds a trainer_state.npz -> (epoch, its directory), or None."""
    root = os.path.join(save_dir, "model_states")
    epochs = [int(e) for e in (os.listdir(root) if os.path.isdir(root) else ())
              if e.isdigit() and os.path.isfile(os.path.join(root, e, STATE_FILE))]
    return (max(epochs), os.path.join(root, str(max(epochs)))) if epochs else None


def plan_resume(args, fp):
    """--resume: the checkpoint to continue from, or a Refusal that names what is wrong.  Reads only."""
    found = find_checkpoint(args.save_dir)
    if found is None:
        raise Refusal("--resume: %s holds no model_states/<epoch>/%s to continue from" % (args.save_dir, STATE_FILE))
    epoch, d = found
    try:
        state = load_trainer_state(os.path.join(d, STATE_FILE))
    except (OSError, ValueError, KeyError) as e:
        raise Refusal("--resume: %s: %s" % (os.path.join(d, STATE_FILE), e))
    if state["epoch"] != epoch:
        raise Refusal("--resume: %s records epoch %d" % (os.path.join(d, STATE_FILE), state["epoch"]))
    for key in FINGERPRINT_KEYS:
        if key not in state["fingerprint"] or state["fingerprint"][key] != fp[key]:
            raise Refusal("--resume: %s differs from the run in %s: the checkpoint of epoch %d has %r, this command %r (a run whose data, "
                          "seed or hyper-parameters changed is not continued)" % (key, args.save_dir, epoch, state["fingerprint"].get(key), fp[key]))
    if epoch >= args.epochs:
        raise Refusal("--resume: %s is already at epoch %d, which is >= --epochs %d (--epochs is the total)" % (args.save_dir, epoch, args.epochs))
    if any(len(state[name][k]) != epoch for name in ("train_results", "val_results") for k in RESULT_KEYS):
        raise Refusal("--resume: %s does not hold %d epochs of results" % (os.path.join(d, STATE_FILE), epoch))
    blob = os.path.join(d, "model_states.bin")
    w = np.fromfile(blob, np.float32) if os.path.isfile(blob) else np.zeros(0, np.float32)
    if w.size != N_WEIGHT_FLOATS:
        raise Refusal("--resume: %s holds %d floats, expected %d" % (blob, w.size, N_WEIGHT_FLOATS))
    state["weights"] = w
    return state


def plan(args):
    """Everything that can be refused, decided before anything is written or a GPU is touched.  -> the run's settings."""
    import tomli
    from ..training_utils import get_sampler, read_labelled
    from .inference import _check_model_config, _device_index
    try:
        if args.model_config is not None:
            _check_model_config(args.model_config)
        device = _device_index(args.device)
    except (ValueError, OSError) as e:
        raise Refusal(str(e))
    if args.epochs < 1 or args.save_per_epoch < 1 or args.save_per_epoch > args.epochs:
        raise Refusal("--epochs >= 1 and 1 <= --save_per_epoch <= --epochs (the reference asserts the latter)")
    if args.num_iterations < 1:
        raise Refusal("--num_iterations must be >= 1")
    if not (args.lr >= 0 and args.weight_decay >= 0):
        raise Refusal("--lr and --weight_decay must be >= 0")
    if not 0 <= int(args.seed) <= 0xffffffff:
        raise Refusal("Seed must be between 0 and 2**32 - 1")
    if args.clip_grad is not None and not (args.clip_grad > 0 and np.isfinite(args.clip_grad)):
        raise Refusal("--clip_grad must be finite and > 0 (leave it out for no clipping)")
    if args.resume and args.init is not None:
        raise Refusal("--resume continues the run in --save_dir from its own checkpoint: it cannot be combined with --init")
    try:
        with open(args.train_config, "rb") as f:
            cfg = tomli.load(f)
    except (OSError, tomli.TOMLDecodeError) as e:
        raise Refusal("--train_config %s: %s" % (args.train_config, e))
    loss = cfg.get("loss_function", {}).get("loss_function_type")
    if loss != "binary_cross_entropy_loss":
        raise Refusal("loss_function_type %r: only binary_cross_entropy_loss is built (the weighted loss is not)" % (loss,))
    ds = cfg.get("dataset", {})
    for key in ("root_dir", "norm_path"):
        if not ds.get(key):
            raise Refusal("[dataset] %s is required" % key)
    if ds.get("num_neighboring_features", 1) != 1:
        raise Refusal("[dataset] num_neighboring_features must be 1 (the m6anet.toml topology)")
    if ds.get("site_info") is not None or isinstance(ds["root_dir"], (list, tuple)):
        raise Refusal("[dataset]: one root_dir with its own data.info.labelled; replicates and site_info are not built")
    min_reads = int(ds.get("min_reads", 20))
    if min_reads < 20:
        raise Refusal("[dataset] min_reads must be >= 20: a step draws 20 reads of every site without replacement")
    loaders = cfg.get("dataloader", {})
    for key in ("train", "val", "test"):
        if key not in loaders:
            raise Refusal("[dataloader.%s] is required" % key)
    batch_size = int(loaders["train"].get("batch_size", 1))
    if batch_size < 1 or batch_size * 20 > (1 << 20):
        raise Refusal("[dataloader.train] batch_size must be in 1..%d" % ((1 << 20) // 20))
    try:
        sampler = get_sampler(loaders["train"])
    except ValueError as e:
        raise Refusal(str(e))
    for name in ("data.json", "data.info", "data.info.labelled"):
        if not os.path.isfile(os.path.join(ds["root_dir"], name)):
            raise Refusal("%s: no such file" % os.path.join(ds["root_dir"], name))
    from ..constants import asset_path
    if not (os.path.isfile(ds["norm_path"]) or os.path.isfile(asset_path(ds["norm_path"]))):
        raise Refusal("[dataset] norm_path %s: no such file" % ds["norm_path"])
    try:
        rows = read_labelled(ds["root_dir"], min_reads)
    except (ValueError, KeyError) as e:
        raise Refusal(str(e))
    from ..data_utils import _read_info
    have = {(r[0], r[1]) for r in _read_info(ds["root_dir"]) if r[4] >= min_reads}
    for r in rows:
        if (r[0], r[1]) not in have:
            raise Refusal("data.info.labelled names %s:%d, which data.info does not hold with >= %d reads" % (r[0], r[1], min_reads))
        if r[4] not in ("Train", "Val", "Test"):
            raise Refusal("data.info.labelled: set_type %s of %s:%d must be Train, Val or Test" % (r[4], r[0], r[1]))
    if len({(r[0], r[1]) for r in rows}) != len(rows):
        raise Refusal("data.info.labelled names a site twice")
    for split in ("Train", "Val", "Test"):
        labels = {r[3] for r in rows if r[4] == split}
        if labels != {0, 1}:
            raise Refusal("data.info.labelled: the %s split needs sites of both classes with >= %d reads" % (split, min_reads))
    fp = fingerprint(args, loaders["train"], batch_size, min_reads, rows)
    resume = plan_resume(args, fp) if args.resume else None
    weights = resume["weights"] if resume else initial_weights(args.init, args.seed)
    return {"cfg": cfg, "device": device, "min_reads": min_reads, "batch_size": batch_size, "sampler": sampler, "rows": rows,
            "weights": weights, "fingerprint": fp, "resume": resume}


def _jsonable(o):
    if isinstance(o, np.ndarray):
        return o.tolist()
    if isinstance(o, (np.floating, np.integer)):
        return o.item()
    raise TypeError(type(o))


def save_blob(path_stem, weights, state_dict):
    np.asarray(weights, np.float32).tofile(path_stem + ".bin")
    try:
        import torch
    except ImportError:
        return
    torch.save({k: torch.from_numpy(np.array(v)) for k, v in state_dict.items()}, path_stem + ".pt")


def main(args):
    try:
        p = plan(args)
    except Refusal as e:
        print("m6anet_amd train: error: %s" % e, file=sys.stderr)
        raise SystemExit(2)
    from ..data_utils import load_sites_native
    from ..engine import M6ANetEngine
    from ..training_utils import join_labels, subset, train, validate
    cfg, ds, save_dir = p["cfg"], p["cfg"]["dataset"], args.save_dir
    batch = load_sites_native([ds["root_dir"]], p["min_reads"], ds["norm_path"], n_threads=args.n_processes)
    X, km, off = np.ascontiguousarray(batch.X), np.ascontiguousarray(batch.site_kmers), np.ascontiguousarray(batch.off)
    y, splits = join_labels(batch.tx_ids, batch.tx_pos, p["rows"])
    print("Saving training information to {}".format(save_dir))
    os.makedirs(save_dir, exist_ok=True)
    info = {"model_config": args.model_config or "m6anet.toml", "train_config": dict(cfg)}
    info["train_config"].update(learning_rate=args.lr, epochs=args.epochs, save_per_epoch=args.save_per_epoch, weight_decay=args.weight_decay,
                                number_of_validation_iterations=args.num_iterations, seed=args.seed, init=args.init, clip_grad=args.clip_grad)
    with open(os.path.join(save_dir, "train_info.json"), "w", encoding="utf-8") as f:
        json.dump(info, f, indent=1)
    resume = p["resume"]
    engine = M6ANetEngine(weights=p["weights"], device=p["device"])
    trainer = engine.trainer(p["weights"], lr=args.lr, weight_decay=args.weight_decay, clip_grad=args.clip_grad)
    make_engine = lambda w: M6ANetEngine(weights=w, device=p["device"])

    def write_results(train_results, val_results):
        for name, res in (("train_results.json", train_results), ("val_results.json", val_results)):
            path = os.path.join(save_dir, name)
            with open(path + ".tmp", "w", encoding="utf-8") as f:
                json.dump(res, f, default=_jsonable)
            os.replace(path + ".tmp", path)

    def save(epoch, weights, state_dict, checkpoint):
        d = os.path.join(save_dir, "model_states", str(epoch))
        os.makedirs(d, exist_ok=resume is not None)       # a run that was cut may have left a directory without its trainer_state.npz
        save_blob(os.path.join(d, "model_states"), weights, state_dict)
        save_trainer_state(os.path.join(d, STATE_FILE), checkpoint, p["fingerprint"])
        write_results(checkpoint["train_results"], checkpoint["val_results"])

    start_epoch, rs_state, results = 0, None, None
    if resume:
        start_epoch, rs_state = resume["epoch"], resume["rs_state"]
        results = (resume["train_results"], resume["val_results"])
        # the bulky lists trainer_state.npz leaves out: y_true is the Val labels every epoch; y_pred is in the val_results.json the
        # run rewrote at every checkpoint (null for an epoch that file does not hold)
        try:
            with open(os.path.join(save_dir, "val_results.json"), encoding="utf-8") as f:
                y_pred = list(json.load(f).get("y_pred", []))[:start_epoch]
        except (OSError, ValueError, AttributeError):
            y_pred = []
        results[1]["y_pred"] = y_pred + [None] * (start_epoch - len(y_pred))
        results[1]["y_true"] = [np.asarray(y[splits["Val"]]).flatten() for _ in range(start_epoch)]
        print("Resuming from epoch %d of %s" % (start_epoch, save_dir))
    try:
        if resume:
            trainer.load_optimizer_state(resume["optimizer"])
        train_results, val_results = train(trainer, make_engine, (X, km, off), y, splits, p["sampler"], args.epochs, p["batch_size"], args.seed,
                                           save_dir=save_dir, save_per_epoch=args.save_per_epoch, n_iterations=args.num_iterations, save=save,
                                           start_epoch=start_epoch, rs_state=rs_state, results=results)
    finally:
        trainer.close()
        engine.close()
    write_results(train_results, val_results)

    test = subset(X, km, off, splits["Test"])
    for criterion in ("avg_loss", "roc_auc", "pr_auc"):
        # the reference's choice (scripts/train.py:110-116), index arithmetic included
        val = [val_results[criterion][i] for i in range(0, len(val_results[criterion]), args.save_per_epoch)]
        best = ((np.argmin(val) if criterion == "avg_loss" else np.argmax(val)) + 1) * args.save_per_epoch
        stem = os.path.join(save_dir, "model_states", str(best), "model_states")
        for ext in (".bin", ".pt"):
            if os.path.exists(stem + ext):
                shutil.copyfile(stem + ext, os.path.join(save_dir, criterion + ext))
        w = np.fromfile(stem + ".bin", np.float32)
        e = make_engine(w)
        try:
            res = validate(e, test[0], test[1], test[2], y[splits["Test"]], n_iterations=args.num_iterations, seed=args.seed)
        finally:
            e.close()
        print("Criteria: {} \tCompute time: {:.3f}".format(criterion, res["compute_time"]))
        print("Test Loss: {:.3f} \tTest ROC AUC: {:.3f} \t Test PR AUC: {:.3f}".format(res["avg_loss"], res["roc_auc"], res["pr_auc"]))
        print("=====================================")
        with open(os.path.join(save_dir, "test_results_%s.json" % criterion), "w", encoding="utf-8") as f:
            json.dump(res, f, default=_jsonable)
