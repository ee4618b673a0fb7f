"""The host side of `train` without a GPU: the blob <-> state_dict pair, init_weights, the samplers against a NumPy restatement of
m6anet/utils/sampler_utils.py, the label join, and the command's help text and refusals (exit status 2 before anything is written)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import train_gen as TG
from m6anet_amd import training_utils as TU
from m6anet_amd.engine import STATE_DICT_KEYS, init_weights, load_weights, state_dict_from_weights, weights_from_state_dict

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_state_dict_and_blob_are_inverses():
    w = load_weights("HCT116_RNA002")
    sd = state_dict_from_weights(w, num_batches_tracked=7)
    assert [k for k in sd if "num_batches" not in k] == [k for k, _ in STATE_DICT_KEYS]
    assert all(sd[k].shape == shape and sd[k].dtype == np.float32 for k, shape in STATE_DICT_KEYS)
    nbt = sd["read_level_encoder.3.layers.1.num_batches_tracked"]
    assert nbt.dtype == np.int64 and nbt.shape == () and int(nbt) == 7
    assert weights_from_state_dict(sd).tobytes() == w.tobytes()
    torch = pytest.importorskip("torch")
    t = {k: torch.from_numpy(np.array(v)) for k, v in sd.items()}
    assert weights_from_state_dict(t).tobytes() == w.tobytes()
    with pytest.raises(ValueError):
        state_dict_from_weights(w[:-1])


def test_init_weights_follows_torchs_default_rule():
    a, b = init_weights(3), init_weights(3)
    assert a.tobytes() == b.tobytes() and a.dtype == np.float32 and a.size == 7997
    assert init_weights(4).tobytes() != a.tobytes()
    sd = state_dict_from_weights(a)
    for key, fan_in in (("read_level_encoder.3.layers.0", 15), ("read_level_encoder.4.layers.0", 150), ("pooling_filter.probability_layer.0", 32)):
        for part in ("weight", "bias"):
            v = sd[key + "." + part]
            assert np.abs(v).max() <= 1 / np.sqrt(fan_in) and np.abs(v).max() > 0.6 / np.sqrt(fan_in), (key, part)
    assert np.all(sd["read_level_encoder.3.layers.1.weight"] == 1) and np.all(sd["read_level_encoder.3.layers.1.bias"] == 0)
    assert np.all(sd["read_level_encoder.3.layers.1.running_mean"] == 0) and np.all(sd["read_level_encoder.3.layers.1.running_var"] == 1)
    E = sd["read_level_encoder.1.embedding_layer.weight"]
    assert abs(E.mean()) < 0.3 and 0.7 < E.std() < 1.3 and np.abs(E).max() > 1.5            # N(0, 1), 132 draws


def test_samplers_compose_as_the_references():
    g = np.random.Generator(np.random.PCG64(0))
    for labels in (np.array([0, 0, 0, 1, 0, 1, 0, 0]), (g.random(301) < 0.2).astype(int), (g.random(50) < 0.8).astype(int), np.array([0, 1, 1, 0])):
        counts = np.unique(labels, return_counts=True)[1]
        mino, majo = np.argwhere(labels == np.argmin(counts)).flatten(), np.argwhere(labels == np.argmax(counts)).flatten()
        rs, ref = np.random.RandomState(25), np.random.RandomState(25)
        want = np.append(majo, ref.choice(mino, len(majo), replace=True))
        ref.shuffle(want)
        got = TU.imbalance_over_sampler(labels, rs)
        assert np.array_equal(got, want) and len(got) == 2 * len(majo)
        want = np.append(mino, ref.choice(majo, len(mino), replace=False))                   # the same streams go on
        ref.shuffle(want)
        got = TU.imbalance_under_sampler(labels, rs)
        assert np.array_equal(got, want) and len(got) == 2 * len(mino)
        assert np.array_equal(TU.shuffled(labels, rs), ref.permutation(len(labels)))
    assert TU.get_sampler({"sampler": "ImbalanceOverSampler"}) is TU.imbalance_over_sampler
    assert TU.get_sampler({"sampler": "ImbalanceUnderSampler"}) is TU.imbalance_under_sampler
    assert TU.get_sampler({"shuffle": True}) is TU.shuffled
    assert np.array_equal(TU.get_sampler({"batch_size": 4})(np.zeros(5), None), np.arange(5))
    for name in ("ImbalanceKmerUnderSampler", "ImbalanceKmerOverSampler"):
        with pytest.raises(ValueError, match=name):
            TU.get_sampler({"sampler": name})
    with pytest.raises(ValueError, match="unknown sampler"):
        TU.get_sampler({"sampler": "Nope"})


def test_label_join(tmp_path):
    rows = TG.info_rows()
    kept = [i for i, r in enumerate(rows) if int(r["n_reads"]) >= 20]
    tx_ids, tx_pos = [rows[i]["transcript_id"] for i in kept], [int(rows[i]["transcript_position"]) for i in kept]
    labels = TG.default_labels(rows)
    d = TG.write_dir(str(tmp_path / "a"), drop=(kept[5],))                   # one loaded site is missing from the labelled file
    lab = TU.read_labelled(d, 20)
    assert len(lab) == len(kept) - 1                                          # the rows under 20 reads are dropped, as the reference drops them
    assert len(TU.read_labelled(d, 1)) == len(rows) - 1
    y, splits = TU.join_labels(tx_ids, tx_pos, lab)
    assert y.dtype == np.float32 and y.shape == (len(kept),)
    got = np.sort(np.concatenate(list(splits.values())))
    assert np.array_equal(got, np.delete(np.arange(len(kept)), 5))            # the site without a row is in no split
    for name, sites in splits.items():
        assert len(sites) and all(labels[kept[s]] == (int(y[s]), name) for s in sites)
        assert set(y[sites]) == {0.0, 1.0}
    bad = [(2, "Train") if i == kept[3] else l for i, l in enumerate(labels)]
    with pytest.raises(ValueError, match="not 0 or 1"):
        TU.read_labelled(TG.write_dir(str(tmp_path / "b"), labels=bad), 20)
    ghost = dict(rows[kept[0]], transcript_position=999999, modification_status=1, set_type="Train")
    with pytest.raises(ValueError, match="999999"):
        TU.join_labels(tx_ids, tx_pos, TU.read_labelled(TG.write_dir(str(tmp_path / "c"), extra=[ghost]), 20))
    with pytest.raises(ValueError, match="twice"):
        TU.join_labels(tx_ids, tx_pos, lab + lab[:1])


def run_train(*argv):
    return subprocess.run([sys.executable, "-m", "m6anet_amd", "train"] + [str(a) for a in argv], cwd=REPO, capture_output=True, text=True, timeout=300)


def test_train_help():
    r = run_train("--help")
    assert r.returncode == 0
    for word in ("--model_config", "--train_config", "--save_dir", "--device", "--lr", "--seed", "--epochs", "--n_processes", "--save_per_epoch",
                 "--weight_decay", "--num_iterations", "--init", "train_info.json", "joblib", "ImbalanceOverSampler"):
        assert word in r.stdout, word


def test_every_refusal_is_exit_status_2_before_anything_is_written(tmp_path, capsys):
    from m6anet_amd.__main__ import main
    rows = TG.info_rows()
    kept = [i for i, r in enumerate(rows) if int(r["n_reads"]) >= 20]
    labels = TG.default_labels(rows)
    good = TG.write_dir(str(tmp_path / "good"))
    cfg = lambda name, root=good, **kw: TG.write_config(tmp_path / (name + ".toml"), root, **kw)
    other_topology = tmp_path / "model.toml"
    other_topology.write_text('[[block]]\nblock_type = "DeaggregateNanopolish"\n[[block]]\nblock_type = "Linear"\ninput_channel = 9\noutput_channel = 4\n')
    not_a_blob = tmp_path / "short.bin"
    np.zeros(10, np.float32).tofile(not_a_blob)
    label2 = TG.write_dir(str(tmp_path / "label2"), labels=[(2, "Train") if i == kept[3] else l for i, l in enumerate(labels)])
    ghost = TG.write_dir(str(tmp_path / "ghost"), extra=[dict(rows[kept[0]], transcript_position=999999, modification_status=1, set_type="Train")])
    no_val = TG.write_dir(str(tmp_path / "no_val"), labels=[(s, "Train" if t == "Val" else t) for s, t in labels])
    unlabelled = str(tmp_path / "unlabelled")
    TG.write_dir(unlabelled)
    os.remove(os.path.join(unlabelled, "data.info.labelled"))
    base = ["--epochs", "2", "--save_per_epoch", "1"]
    cases = [
        (["--train_config", cfg("ok"), "--model_config", other_topology] + base, "topology"),
        (["--train_config", cfg("ok"), "--device", "cpu"] + base, "no CPU"),
        (["--train_config", cfg("ok"), "--epochs", "2", "--save_per_epoch", "3"], "save_per_epoch"),
        (["--train_config", cfg("ok"), "--epochs", "0", "--save_per_epoch", "1"], "--epochs"),
        (["--train_config", cfg("ok"), "--lr", "-1"] + base, "--lr"),
        (["--train_config", cfg("ok"), "--init", "NOPE_RNA009"] + base, "--init"),
        (["--train_config", cfg("ok"), "--init", not_a_blob] + base, "10 floats"),
        (["--train_config", tmp_path / "missing.toml"] + base, "missing.toml"),
        (["--train_config", cfg("weighted", loss="weighted_binary_cross_entropy_loss")] + base, "weighted loss"),
        (["--train_config", cfg("nonorm", norm_path=None)] + base, "norm_path is required"),
        (["--train_config", cfg("badnorm", norm_path=str(tmp_path / "nope.joblib"))] + base, "nope.joblib"),
        (["--train_config", cfg("kmer_under", sampler='sampler = "ImbalanceKmerUnderSampler"')] + base, "ImbalanceKmerUnderSampler"),
        (["--train_config", cfg("kmer_over", sampler='sampler = "ImbalanceKmerOverSampler"')] + base, "ImbalanceKmerOverSampler"),
        (["--train_config", cfg("unknown", sampler='sampler = "Nope"')] + base, "unknown sampler"),
        (["--train_config", cfg("ok"), "--num_iterations", "0"] + base, "--num_iterations"),
        (["--train_config", cfg("nn2", dataset_extra="site_info = \"x\"")] + base, "site_info"),
        (["--train_config", cfg("label2", root=label2)] + base, "not 0 or 1"),
        (["--train_config", cfg("ghost", root=ghost)] + base, "999999"),
        (["--train_config", cfg("no_val", root=no_val)] + base, "Val split"),
        (["--train_config", cfg("unlabelled", root=unlabelled)] + base, "data.info.labelled"),
        (["--train_config", cfg("noroot", root=str(tmp_path / "nowhere"))] + base, "no such file"),
    ]
    for k, (argv, word) in enumerate(cases):
        out = tmp_path / ("out%d" % k)
        with pytest.raises(SystemExit) as e:
            main(["train", "--save_dir", str(out)] + [str(a) for a in argv])
        err = capsys.readouterr().err
        assert e.value.code == 2 and word in err, (argv, e.value.code, err[-500:])
        assert not out.exists(), argv
    r = run_train("--save_dir", tmp_path / "out_sub", *cases[1][0])          # and once as the command itself
    assert r.returncode == 2 and "no CPU" in r.stderr and "Traceback" not in r.stderr and not (tmp_path / "out_sub").exists()
