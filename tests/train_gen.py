"""A labelled training directory for the tests of `train`: the bundled data.json / data.info (tests/golden/ref_tests_data) with a
generated data.info.labelled beside them, and a train config in the reference's TOML keys."""
import csv
import os
import shutil

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_tests_data")


def info_rows():
    with open(os.path.join(GOLD, "data.info"), newline="") as f:
        return list(csv.DictReader(f))


def default_labels(rows):
    """Every third site modified; the splits interleaved so that each holds both classes among the sites with >= 20 reads."""
    out, k = [], 0
    for r in rows:
        if int(r["n_reads"]) >= 20:
            out.append((int(k % 3 == 0), ("Train", "Train", "Train", "Train", "Val", "Test", "Train", "Val", "Test")[(k // 3 + k % 3 * 4) % 9]))
            k += 1
        else:
            out.append((k % 2, "Train"))
    return out


def write_dir(path, labels=None, drop=(), extra=()):
    """data.json, data.info and data.info.labelled under `path`.  labels: [(status, set_type)] per data.info row (default_labels);
    drop: row numbers left out of the labelled file; extra: rows (dicts) appended to it."""
    os.makedirs(path, exist_ok=True)
    for name in ("data.json", "data.info"):
        shutil.copyfile(os.path.join(GOLD, name), os.path.join(path, name))
    rows = info_rows()
    labels = default_labels(rows) if labels is None else labels
    with open(os.path.join(path, "data.info.labelled"), "w", newline="") as f:
        w = csv.DictWriter(f, ["transcript_id", "transcript_position", "start", "end", "n_reads", "modification_status", "set_type"])
        w.writeheader()
        for i, (r, (status, set_type)) in enumerate(zip(rows, labels)):
            if i not in drop:
                w.writerow(dict(r, modification_status=status, set_type=set_type))
        for r in extra:
            w.writerow(r)
    return path


def write_config(path, root_dir, batch_size=16, sampler='sampler = "ImbalanceOverSampler"', loss="binary_cross_entropy_loss",
                 norm_path="norm_hct116.npz", dataset_extra=""):
    with open(path, "w") as f:
        f.write('[loss_function]\nloss_function_type = "%s"\n\n[dataset]\nroot_dir = "%s"\nmin_reads = 20\n' % (loss, root_dir))
        if norm_path is not None:
            f.write('norm_path = "%s"\n' % norm_path)
        f.write('num_neighboring_features = 1\n%s\n[dataloader]\n[dataloader.train]\nbatch_size = %d\n%s\n\n' % (dataset_extra, batch_size, sampler))
        f.write('[dataloader.val]\nbatch_size = 256\nshuffle = false\n\n[dataloader.test]\nbatch_size = 256\nshuffle = false\n')
    return str(path)
