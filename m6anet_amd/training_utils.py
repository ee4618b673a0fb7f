"""Host-side mirror of m6anet/utils/training_utils.py.

`validate` (training_utils.py:213-268) and its metric helpers (:15-45) -- SURVEY.md section 8(f)
rank 4: the same dictionary the reference returns, with the predictions computed by
M6ANetEngine.validate_forward (every read encoded once on the GPU; the reference re-encodes the 20
sampled reads of every site in every pass).

`train_one_epoch` and `train` (training_utils.py:61-210) on engine.Trainer: the forward in training mode, the
backward pass and Adam run in HIP (include/m6a.h: m6a_train_epoch) on the data set held as the flat arrays of
include/m6a.h, and the samplers of m6anet/utils/sampler_utils.py as functions of (labels, RandomState).
DESIGN.md section 8 says what is not built (the weighted loss, the per-motif samplers, more than one GPU).
"""
import os
import time

import numpy as np


def _curve_counts(y_true, y_score):
    """Cumulative true/false positives at every distinct score, highest first
    (sklearn.metrics._ranking._binary_clf_curve for 0/1 labels, which roc_curve and
    precision_recall_curve -- training_utils.py:26,42 -- are built on)."""
    y_true = np.asarray(y_true, np.float64).ravel()
    y_score = np.asarray(y_score, np.float64).ravel()
    order = np.argsort(y_score, kind="mergesort")[::-1]
    y_score, y_true = y_score[order], y_true[order]
    distinct = np.where(np.diff(y_score))[0]
    idx = np.r_[distinct, y_true.size - 1]
    tps = np.cumsum(y_true)[idx]
    fps = 1 + idx - tps
    return fps, tps


def _trapezoid(y, x):
    """sklearn.metrics.auc's area (np.trapz)."""
    y, x = np.asarray(y, np.float64), np.asarray(x, np.float64)
    return float(np.sum((x[1:] - x[:-1]) * (y[1:] + y[:-1]) * 0.5))


def get_roc_auc(y_true, y_pred):
    """auc(roc_curve(y_true, y_pred)) (training_utils.py:26-27); collinear points are not dropped, which
    leaves the trapezoid area unchanged."""
    fps, tps = _curve_counts(y_true, y_pred)
    fps, tps = np.r_[0, fps], np.r_[0, tps]
    if fps[-1] <= 0 or tps[-1] <= 0:
        return float("nan")
    return _trapezoid(tps / tps[-1], fps / fps[-1])


def get_pr_auc(y_true, y_pred):
    """auc(recall, precision) of precision_recall_curve(..., pos_label=1) (training_utils.py:42-43)."""
    fps, tps = _curve_counts(y_true, y_pred)
    ps = tps + fps
    precision = np.where(ps > 0, tps / np.maximum(ps, 1), 0.0)
    recall = tps / tps[-1] if tps[-1] > 0 else np.ones_like(tps)
    precision, recall = np.r_[precision[::-1], 1.0], np.r_[recall[::-1], 0.0]
    return -_trapezoid(precision, recall)


def binary_cross_entropy(y_pred, y_true):
    """torch.nn.BCELoss() (mean reduction, log clamped at -100), what train configs use as criterion."""
    p = np.asarray(y_pred, np.float32)
    y = np.asarray(y_true, np.float32)
    with np.errstate(divide="ignore"):
        lp = np.maximum(np.log(p), np.float32(-100.0))
        lq = np.maximum(np.log1p(-p), np.float32(-100.0))
    return float(np.mean(-(y * lp + (1.0 - y) * lq), dtype=np.float32))


def validate(engine, X, site_kmers, off, y_true, n_iterations=1, seed=0, criterion=binary_cross_entropy):
    """The reference's `validate(model, val_dl, device, criterion, n_iterations)` for a whole validation
    split held as the flat arrays of include/m6a.h (DataLoader order = site order, num_workers=0).
    Returns the same keys: y_pred (list of passes), y_true, compute_time, roc_auc, pr_auc, avg_loss."""
    start = time.time()
    y_pred, y_pred_avg = engine.validate_forward(X, site_kmers, off, n_iterations=n_iterations, seed=seed)
    if hasattr(y_pred, "cpu"):
        y_pred, y_pred_avg = y_pred.cpu().numpy(), y_pred_avg.cpu().numpy()
    compute_time = time.time() - start
    y_true = np.asarray(y_true).flatten()
    return {
        "y_pred": [row for row in y_pred],
        "y_true": y_true,
        "compute_time": compute_time,
        "roc_auc": get_roc_auc(y_true, y_pred_avg),
        "pr_auc": get_pr_auc(y_true, y_pred_avg),
        "avg_loss": criterion(y_pred_avg, y_true),
    }


# ---- training (m6anet/utils/training_utils.py:61-210, m6anet/utils/sampler_utils.py) -------------------------------------------------

def _classes(labels):
    """minority and majority class and their positions, as the reference's samplers find them (sampler_utils.py:36-39)."""
    labels = np.asarray(labels).astype(np.int64).ravel()
    counts = np.unique(labels, return_counts=True)[1]
    minority, majority = np.argmin(counts), np.argmax(counts)
    return np.argwhere(labels == minority).flatten(), np.argwhere(labels == majority).flatten()


def imbalance_over_sampler(labels, rs):
    """ImbalanceOverSampler.__iter__ (sampler_utils.py:93-96): the majority class, as many draws WITH replacement from the
    minority class, shuffled -- with the RandomState `rs` in place of the global one."""
    minority_idx, majority_idx = _classes(labels)
    idx = np.append(majority_idx, rs.choice(minority_idx, len(majority_idx), replace=True))
    rs.shuffle(idx)
    return idx


def imbalance_under_sampler(labels, rs):
    """ImbalanceUnderSampler.__iter__ (sampler_utils.py:45-48): the minority class and as many of the majority class, drawn
    without replacement, shuffled."""
    minority_idx, majority_idx = _classes(labels)
    idx = np.append(minority_idx, rs.choice(majority_idx, len(minority_idx), replace=False))
    rs.shuffle(idx)
    return idx


def shuffled(labels, rs):
    """DataLoader(shuffle=True): every site once, in the order of rs.permutation."""
    return rs.permutation(len(np.asarray(labels).ravel()))


SAMPLERS = {"ImbalanceOverSampler": imbalance_over_sampler, "ImbalanceUnderSampler": imbalance_under_sampler}
REFUSED_SAMPLERS = ("ImbalanceKmerUnderSampler", "ImbalanceKmerOverSampler")


def get_sampler(train_loader_config):
    """The sampler of a [dataloader.train] table: `sampler = "<name>"`, else shuffle = true, else sites in order."""
    name = train_loader_config.get("sampler")
    if name in REFUSED_SAMPLERS:
        raise ValueError("sampler %s (per-motif balancing) is not built here; ImbalanceOverSampler and ImbalanceUnderSampler are" % name)
    if name is not None:
        if name not in SAMPLERS:
            raise ValueError("unknown sampler %s, must be one of %s" % (name, sorted(SAMPLERS)))
        return SAMPLERS[name]
    if train_loader_config.get("shuffle", False):
        return shuffled
    return lambda labels, rs: np.arange(len(np.asarray(labels).ravel()))


def read_labelled(root_dir, min_reads):
    """data.info.labelled as NanopolishDS.initialize_data_info reads it (m6anet/utils/data_utils.py): rows
    (transcript_id, transcript_position, n_reads, modification_status, set_type), rows with n_reads < min_reads dropped."""
    import csv
    rows = []
    path = os.path.join(root_dir, "data.info.labelled")
    with open(path, newline="") as f:
        rd = csv.DictReader(f)
        need = {"transcript_id", "transcript_position", "n_reads", "modification_status", "set_type"}
        if not need <= set(rd.fieldnames or ()):
            raise ValueError("%s: missing column(s) %s" % (path, sorted(need - set(rd.fieldnames or ()))))
        for line, r in enumerate(rd, 2):
            if int(r["n_reads"]) < min_reads:
                continue
            label = float(r["modification_status"])
            if label not in (0.0, 1.0):
                raise ValueError("%s line %d: modification_status %s is not 0 or 1" % (path, line, r["modification_status"]))
            rows.append((r["transcript_id"], int(r["transcript_position"]), int(r["n_reads"]), int(label), r["set_type"]))
    return rows


def join_labels(tx_ids, tx_pos, rows):
    """Labelled rows joined to the loaded sites on (transcript_id, transcript_position).
    -> y float32 [n_sites] (0 where a site has no row: such a site is in no split), {split: site numbers in row order}."""
    where = {(t, int(p)): i for i, (t, p) in enumerate(zip(tx_ids, tx_pos))}
    y = np.zeros(len(where), np.float32)
    splits = {"Train": [], "Val": [], "Test": []}
    seen = set()
    for tx, pos, _, label, set_type in rows:
        i = where.get((tx, pos))
        if i is None:
            raise ValueError("data.info.labelled names %s:%d, which data.info does not hold with enough reads" % (tx, pos))
        if i in seen:
            raise ValueError("data.info.labelled names %s:%d twice" % (tx, pos))
        seen.add(i)
        if set_type not in splits:
            raise ValueError("set_type %s of %s:%d: must be Train, Val or Test" % (set_type, tx, pos))
        y[i] = label
        splits[set_type].append(i)
    return y, {k: np.asarray(v, np.int64) for k, v in splits.items()}


def train_one_epoch(trainer, X, site_kmers, off, y, order, batch_size, seed, bag=20):
    """The reference's train_one_epoch (training_utils.py:148-210) over the sites `order`: one m6a_train_epoch call, every step
    queued back to back on the GPU.  Returns its dictionary: compute_time, avg_loss (the mean of the step losses), roc_auc, pr_auc."""
    start = time.time()
    loss, y_pred = trainer.epoch(X, site_kmers, off, y, order, batch_size, bag=bag, seed=seed)
    if hasattr(loss, "cpu"):
        trainer._engine.sync()
        loss, y_pred = loss.cpu().numpy(), y_pred.cpu().numpy()
    compute_time = time.time() - start
    y_np = y.cpu().numpy() if hasattr(y, "cpu") else np.asarray(y)
    order_np = order.cpu().numpy() if hasattr(order, "cpu") else np.asarray(order)
    y_true = y_np[order_np]
    return {"compute_time": compute_time, "avg_loss": float(np.mean(np.asarray(loss, np.float64))),
            "roc_auc": get_roc_auc(y_true, y_pred), "pr_auc": get_pr_auc(y_true, y_pred)}


def subset(X, site_kmers, off, sites):
    """The flat arrays of the sites `sites` alone (a validation or test split)."""
    sites = np.asarray(sites, np.int64)
    off = np.asarray(off, np.int64)
    n = off[sites + 1] - off[sites]
    rows = np.concatenate([np.arange(off[s], off[s + 1]) for s in sites]) if len(sites) else np.zeros(0, np.int64)
    return np.ascontiguousarray(X[rows]), np.ascontiguousarray(site_kmers[sites]), np.concatenate([[0], np.cumsum(n)]).astype(np.int64)


def _takes_checkpoint(save):
    """Whether a save callback accepts the keyword `checkpoint` (by name or through **kwargs)."""
    import inspect
    try:
        params = inspect.signature(save).parameters.values()
    except (TypeError, ValueError):
        return False
    return any(p.kind is p.VAR_KEYWORD or (p.name == "checkpoint" and p.kind in (p.POSITIONAL_OR_KEYWORD, p.KEYWORD_ONLY)) for p in params)


def train(trainer, make_engine, data, y, splits, sampler, n_epoch, batch_size, seed, save_dir=None, save_per_epoch=10, n_iterations=1,
          save=None, verbose=True, clip_grad=None, start_epoch=0, rs=None, rs_state=None, results=None):
    """The reference's train loop (training_utils.py:61-145).  data = (X, site_kmers, off) of every loaded site, y their labels,
    splits = join_labels' site numbers.  Each epoch: the sampler's order over the Train sites, train_one_epoch, then `validate`
    on a fresh engine made from the trainer's weights (make_engine(weights)) over the Val sites; the per-epoch lists are kept and
    every save_per_epoch epochs save(epoch, weights, state_dict) is called.  Returns (train_results, val_results).

    clip_grad: the reference's clip_grad (clip_grad_norm_ between backward and the optimizer's step; None leaves the trainer as it is).
    Continuing a run: start_epoch = the epochs already done (epochs are numbered start_epoch + 1 .. n_epoch), `rs` the sampler's
    RandomState or `rs_state` its get_state() at that point, `results` = (train_results, val_results) so far, which are extended; the
    trainer is expected to hold that epoch's weights and optimizer state.  A `save` that takes the keyword `checkpoint` also receives
    checkpoint = {"epoch", "optimizer" (Trainer.optimizer_state()), "rs_state", "train_results", "val_results"}."""
    assert save_per_epoch <= n_epoch
    assert 0 <= start_epoch <= n_epoch
    X, site_kmers, off = data
    if rs is None:
        rs = np.random.RandomState(seed)
    if rs_state is not None:
        rs.set_state(rs_state)
    if clip_grad is not None:
        trainer.set_clip(clip_grad)
    train_sites = splits["Train"]
    val = subset(X, site_kmers, off, splits["Val"])
    train_results, val_results = results if results is not None else ({}, {})
    total = 0.0
    with_checkpoint = save is not None and _takes_checkpoint(save)
    for epoch in range(start_epoch + 1, n_epoch + 1):
        order = np.ascontiguousarray(train_sites[sampler(y[train_sites], rs)], np.int64)
        tr = train_one_epoch(trainer, X, site_kmers, off, y, order, batch_size, seed=(int(seed) << 20) + epoch)
        weights = trainer.weights()
        engine = make_engine(weights)
        try:
            va = validate(engine, val[0], val[1], val[2], y[splits["Val"]], n_iterations=n_iterations, seed=seed)
        finally:
            engine.close()
        total += tr["compute_time"] + va["compute_time"]
        if verbose:
            print("Epoch:[%d/%d] \t train time:%.0fs \t val time:%.0fs \t (%.0fs)" % (epoch, n_epoch, tr["compute_time"], va["compute_time"], total))
            print("Train Loss:%.2f\t Train ROC AUC: %.3f\t Train PR AUC: %.3f" % (tr["avg_loss"], tr["roc_auc"], tr["pr_auc"]))
            print("Val Loss:%.2f \t Val ROC AUC: %.3f\t Val PR AUC: %.3f" % (va["avg_loss"], va["roc_auc"], va["pr_auc"]))
            print("=====================================")
        for res, out in ((tr, train_results), (va, val_results)):
            for k, v in res.items():
                out.setdefault(k, []).append(v)
        if save is not None and epoch % save_per_epoch == 0:
            if with_checkpoint:
                save(epoch, weights, trainer.state_dict(),
                     checkpoint={"epoch": epoch, "optimizer": trainer.optimizer_state(), "rs_state": rs.get_state(),
                                 "train_results": train_results, "val_results": val_results})
            else:
                save(epoch, weights, trainer.state_dict())
    return train_results, val_results
