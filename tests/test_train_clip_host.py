"""Gradient clipping, optimizer-state checkpoints and --resume without a GPU: the float64 statement with the clip against torch
float64 (tests/train_clip_torch.py), the conditions of the GPU cases of test_gpu_train_clip.py, trainer_state.npz's round trip of the
sampler's RandomState, training_utils.train's continuation arguments on a stand-in trainer, and the command's help and refusals."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import train_clip_torch as CT
import train_gen as TG
import train_torch as TT
from m6anet_amd import training_utils as TU
from m6anet_amd.engine import load_weights
from m6anet_amd.scripts import train as CMD

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HCT = "HCT116_RNA002"


@pytest.fixture(scope="module")
def bundled():
    return CT.bundled()


def test_the_batches_are_test_gpu_trains(bundled):
    import test_gpu_train as G
    assert CT.SEEDS == G.SEEDS and set(CT.SHAPES) <= set(G.SHAPES)
    for B, bag in CT.SHAPES:
        for s in CT.SEEDS:
            want = G.make_batch(bundled, B, bag, 1000 * B + 10 * bag + s)            # test_step_shapes' batch of that seed
            for got in CT.case_batches(bundled, B, bag, s):
                assert all(np.array_equal(a, b) for a, b in zip(got, want))


@pytest.mark.parametrize("B,bag", [(3, 20), (13, 20), (7, 5)])
@pytest.mark.parametrize("factor", [0.25, 4.0])
def test_statement_with_clip_is_torch_float64_to_rounding(bundled, B, bag, factor):
    w = load_weights(HCT)
    e_ref, e_stmt = [], []
    for s in CT.SEEDS:
        batches = CT.case_batches(bundled, B, bag, s)
        T = CT.first_norm(w, batches)
        stmt = CT.conditions(w, batches, factor * T, clipped=factor < 1)
        f32, f64 = CT.run(w, batches, torch.float32, factor * T), CT.run(w, batches, torch.float64, factor * T)
        e_ref.append(CT.errors(f32, f64))
        e_stmt.append(CT.errors(stmt, f64))
        # the first step's norm, before any Adam step lies between the two: a float64 sum of 7 697 squares, 7 697 * 2^-53 < 1e-12
        assert abs(stmt["norm"][0] - f64["norm"][0]) <= 1e-12 * f64["norm"][0]
        if factor < 1:                                                          # the clipped gradient has the norm max_norm
            n = np.sqrt(np.sum(stmt["grad"] ** 2))
            assert abs(n - factor * T) <= 1e-5 * factor * T and stmt["norm"][-1] > n
    TT.hold("statement clip %g T %dx%d" % (factor, B, bag), TT.pooled(e_ref), TT.pooled(e_stmt))


def test_statement_max_norm_zero_is_the_statement_without_clip(bundled):
    w = load_weights(HCT)
    batches = CT.case_batches(bundled, 13, 20, 11)
    a, b = CT.statement_run(w, batches), TT.statement_run(w, batches)
    assert a["blob"].tobytes() == b["blob"].tobytes() and a["grad"].tobytes() == b["grad"].tobytes()
    # an unclipped step with clipping on multiplies by exactly 1
    c = CT.statement_run(w, batches, max_norm=4 * a["norm"].max())
    assert c["blob"].tobytes() == a["blob"].tobytes() and c["grad"].tobytes() == a["grad"].tobytes()


@pytest.mark.parametrize("B,bag", CT.SHAPES)
def test_conditions_of_the_gpu_cases(bundled, B, bag):
    w = load_weights(HCT)
    for cfg in ({}, {"weight_decay": 1e-2}):
        for s in CT.SEEDS:
            batches = CT.case_batches(bundled, B, bag, s)
            T = CT.first_norm(w, batches, **cfg)
            assert T > 0
            CT.conditions(w, batches, 0.25 * T, clipped=True, **cfg)
            CT.conditions(w, batches, 4 * T, clipped=False, **cfg)


def checkpoint_of(rs, epoch=3):
    g = np.random.Generator(np.random.PCG64(epoch))
    res = lambda: {k: list(g.random(epoch)) for k in CMD.RESULT_KEYS}
    val = res()
    val["y_pred"] = [[np.zeros(4, np.float32)]] * epoch                          # left out of the file
    return {"epoch": epoch, "optimizer": {"m": g.standard_normal(7997).astype(np.float32), "v": g.random(7997).astype(np.float32), "n_steps": 41},
            "rs_state": rs.get_state(), "train_results": res(), "val_results": val}


def test_trainer_state_round_trips_the_random_state(tmp_path):
    labels = (np.arange(200) % 7 == 0).astype(int)
    for draws_before in (0, 1, 5):
        rs = np.random.RandomState(25)
        for _ in range(draws_before):
            TU.imbalance_over_sampler(labels, rs)
        if draws_before == 5:
            rs.standard_normal()                                                # leaves a cached gaussian behind: has_gauss = 1
            assert rs.get_state()[3] == 1
        ck = checkpoint_of(rs)
        fp = {"seed": 25, "lr": 4e-4, "clip_grad": None, "sampler": "ImbalanceOverSampler"}
        path = str(tmp_path / ("state%d.npz" % draws_before))
        CMD.save_trainer_state(path, ck, fp)
        assert os.listdir(tmp_path).count(os.path.basename(path)) == 1 and not os.path.exists(path + ".tmp")
        assert os.path.getsize(path) < 80 * 1024
        back = CMD.load_trainer_state(path)
        rs2 = np.random.RandomState(0)
        rs2.set_state(back["rs_state"])
        assert np.array_equal(TU.imbalance_over_sampler(labels, rs2), TU.imbalance_over_sampler(labels, rs))     # the next draw
        assert rs2.standard_normal() == rs.standard_normal()
        assert back["fingerprint"] == fp and back["epoch"] == 3 and back["optimizer"]["n_steps"] == 41
        assert back["optimizer"]["m"].tobytes() == ck["optimizer"]["m"].tobytes() and back["optimizer"]["v"].tobytes() == ck["optimizer"]["v"].tobytes()
        for name in ("train_results", "val_results"):
            assert set(back[name]) == set(CMD.RESULT_KEYS)
            assert all(back[name][k] == ck[name][k] for k in CMD.RESULT_KEYS)
    with np.load(path, allow_pickle=False) as z:                                # every field is a plain array: nothing is pickled
        assert {"m", "v", "n_steps", "epoch", "rs_name", "rs_keys", "rs_pos", "rs_has_gauss", "rs_cached_gaussian", "fingerprint"} <= set(z.files)


class StandInTrainer:
    """training_utils.train's view of engine.Trainer, on the host: the `weights` are a running hash of everything an epoch is fed."""

    def __init__(self):
        self.w, self.t, self.clip = np.zeros(4, np.float64), 0, None

    def set_clip(self, max_norm):
        self.clip = max_norm

    def epoch(self, X, km, off, y, order, batch_size, bag=20, seed=0):
        n = -(-len(order) // batch_size)
        self.t += n
        self.w = np.array([self.w[0] * 0.5 + float(np.dot(order % 97, np.arange(len(order)) % 13)), self.w[1] + seed, self.t, len(order)], np.float64)
        return np.full(n, 0.5 + 1e-3 * (self.w[0] % 7), np.float32), (0.25 + 0.5 * ((order * 7 + int(self.w[0])) % 11) / 11).astype(np.float32)

    def weights(self):
        return self.w.copy()

    def state_dict(self):
        return {"w": self.w.copy()}

    def optimizer_state(self):
        return {"m": self.w.copy(), "v": self.w.copy(), "n_steps": self.t}


class StandInEngine:
    def __init__(self, w):
        self.w = w

    def validate_forward(self, X, km, off, n_iterations=1, seed=0, **kw):
        S = len(off) - 1
        p = (0.1 + 0.8 * ((np.arange(S) * 5 + int(self.w[0])) % 13) / 13).astype(np.float32)
        return np.tile(p, (n_iterations, 1)), p

    def close(self):
        pass


def stand_in_data(S=60):
    g = np.random.Generator(np.random.PCG64(3))
    off = np.arange(S + 1, dtype=np.int64) * 20
    y = (np.arange(S) % 4 == 0).astype(np.float32)
    sites = np.arange(S)
    splits = {"Train": sites[sites % 3 != 0], "Val": sites[sites % 3 == 0], "Test": sites[:0]}
    return (g.standard_normal((S * 20, 9)).astype(np.float32), np.zeros((S, 3), np.uint8), off), y, splits


def scalars(res):
    return {k: v for k, v in res.items() if k not in ("compute_time", "y_pred", "y_true")}


def test_train_continues_where_a_checkpoint_left_it():
    data, y, splits = stand_in_data()
    seen = {}

    def save(epoch, weights, state_dict, checkpoint):
        assert checkpoint["epoch"] == epoch and checkpoint["optimizer"]["n_steps"] > 0
        seen[epoch] = (weights, checkpoint["rs_state"], {k: list(v) for k, v in checkpoint["train_results"].items()},
                       {k: list(v) for k, v in checkpoint["val_results"].items()})

    args = (StandInEngine, data, y, splits, TU.imbalance_over_sampler)
    whole = StandInTrainer()
    tr_all, va_all = TU.train(whole, *args, 5, 16, 25, save_per_epoch=1, save=save, verbose=False)
    assert sorted(seen) == [1, 2, 3, 4, 5] and len(tr_all["avg_loss"]) == 5
    at2 = seen[2]
    assert all(len(v) == 2 for v in at2[2].values())
    so_far = lambda: ({k: list(v) for k, v in at2[2].items()}, {k: list(v) for k, v in at2[3].items()})       # train extends them

    part = StandInTrainer()
    part.w, part.t = at2[0].copy(), int(at2[0][2])                               # what --resume restores through the library
    old_style = []
    tr2, va2 = TU.train(part, *args, 5, 16, 25, save_per_epoch=1, save=lambda e, w, sd: old_style.append(e), verbose=False,
                        start_epoch=2, rs_state=at2[1], results=so_far(), clip_grad=0.5)
    assert old_style == [3, 4, 5]                                               # a three-argument callback still works; epochs 3 .. 5
    assert part.clip == 0.5 and whole.clip is None
    assert scalars(tr2) == scalars(tr_all) and scalars(va2) == scalars(va_all)
    assert part.weights().tobytes() == whole.weights().tobytes()
    # without the RandomState the orders differ, and so do the results: the check above has teeth
    cold = StandInTrainer()
    cold.w = at2[0].copy()
    tr3, _ = TU.train(cold, *args, 5, 16, 25, save_per_epoch=1, verbose=False, start_epoch=2, results=so_far())
    assert scalars(tr3) != scalars(tr_all)
    # rs= in place of rs_state=
    rs = np.random.RandomState(0)
    rs.set_state(at2[1])
    warm = StandInTrainer()
    warm.w = at2[0].copy()
    tr4, _ = TU.train(warm, *args, 5, 16, 25, save_per_epoch=1, verbose=False, start_epoch=2, rs=rs, results=so_far())
    assert scalars(tr4) == scalars(tr_all)


def run_train(*argv):
    return subprocess.run([sys.executable, "-m", "m6anet_amd", "train"] + [str(a) for a in argv], cwd=REPO, capture_output=True, text=True, timeout=300)


def test_help_names_both_flags():
    r = run_train("--help")
    assert r.returncode == 0
    for word in ("--clip_grad", "--resume", "trainer_state.npz", "test_results_"):
        assert word in r.stdout, word
    not_built = r.stdout[r.stdout.index("Not built"):]
    not_built = not_built[:not_built.index("\n\n")]                             # the description's last sentence
    assert "clipping" not in not_built and "resuming" not in not_built


def listing(root):
    return sorted((os.path.relpath(os.path.join(d, f), root), os.path.getsize(os.path.join(d, f))) for d, _, fs in os.walk(root) for f in fs)


def write_run(save_dir, args, p, epoch, n_results=None):
    """What a run with these settings leaves behind at `epoch`, made without a GPU."""
    d = os.path.join(save_dir, "model_states", str(epoch))
    os.makedirs(d)
    np.zeros(7997, np.float32).tofile(os.path.join(d, "model_states.bin"))
    CMD.save_trainer_state(os.path.join(d, CMD.STATE_FILE), checkpoint_of(np.random.RandomState(args.seed), n_results or epoch) | {"epoch": epoch},
                           p["fingerprint"])


def test_every_new_refusal_is_exit_status_2_with_nothing_written(tmp_path, capsys):
    from m6anet_amd.__main__ import main
    data = TG.write_dir(str(tmp_path / "data"))
    cfg = TG.write_config(tmp_path / "train.toml", data, batch_size=16)
    base = ["--train_config", cfg, "--epochs", "4", "--save_per_epoch", "1", "--seed", "3", "--clip_grad", "0.5"]

    def parsed(extra=(), save_dir="x"):
        a = CMD.argparser().parse_args(base + list(extra) + ["--save_dir", save_dir])
        return a, CMD.plan(a)

    args, p = parsed()
    assert p["resume"] is None and p["fingerprint"]["clip_grad"] == 0.5 and p["fingerprint"]["sampler"] == "ImbalanceOverSampler"
    assert set(p["fingerprint"]) == set(CMD.FINGERPRINT_KEYS) and len(p["fingerprint"]["sites_sha256"]) == 64
    json.dumps(p["fingerprint"])
    run = str(tmp_path / "run")
    write_run(run, args, p, 1)
    write_run(run, args, p, 2)
    os.makedirs(os.path.join(run, "model_states", "3"))                          # a directory the cut left without its trainer_state.npz
    done = str(tmp_path / "done")
    write_run(done, args, p, 4)
    empty = str(tmp_path / "empty")
    os.makedirs(os.path.join(empty, "model_states", "1"))
    short = str(tmp_path / "short")
    write_run(short, args, p, 2, n_results=1)
    pretrained = load_weights(HCT)
    blob = tmp_path / "init.bin"
    pretrained.tofile(blob)
    kept = [k for k, r in enumerate(TG.info_rows()) if int(r["n_reads"]) >= 20]
    assert TG.default_labels(TG.info_rows())[kept[0]] == (1, "Train")
    other = TG.write_dir(str(tmp_path / "other"), drop=(kept[0],))               # one Train site fewer
    swapped = TG.default_labels(TG.info_rows())
    i, j = [k for k, (s, t) in enumerate(swapped) if t == "Val"][:2]
    swapped[i], swapped[j] = (1 - swapped[i][0], "Val"), swapped[j]
    relabelled = TG.write_dir(str(tmp_path / "relabelled"), labels=swapped)      # one Val label flipped
    cases = [
        (run, ["--resume", "--init", str(blob)], ["--init"]),
        (str(tmp_path / "nowhere"), ["--resume"], ["trainer_state.npz"]),
        (empty, ["--resume"], ["trainer_state.npz"]),
        (done, ["--resume"], ["epoch 4", "--epochs 4"]),
        (short, ["--resume"], ["2 epochs of results"]),
        (run, ["--resume", "--seed", "4"], ["seed", "3", "4"]),
        (run, ["--resume", "--lr", "0.001"], ["lr", "0.0004", "0.001"]),
        (run, ["--resume", "--weight_decay", "0.01"], ["weight_decay", "0.0", "0.01"]),
        (run, ["--resume", "--clip_grad", "0.25"], ["clip_grad", "0.5", "0.25"]),
        (run, ["--resume", "--save_per_epoch", "2"], ["save_per_epoch", "1", "2"]),
        (run, ["--resume", "--train_config", TG.write_config(tmp_path / "bs.toml", data, batch_size=32)], ["batch_size", "16", "32"]),
        (run, ["--resume", "--train_config", TG.write_config(tmp_path / "under.toml", data, sampler='sampler = "ImbalanceUnderSampler"')],
         ["sampler", "ImbalanceOverSampler", "ImbalanceUnderSampler"]),
        (run, ["--resume", "--train_config", TG.write_config(tmp_path / "other.toml", other)], ["sites_sha256", p["fingerprint"]["sites_sha256"]]),
        (run, ["--resume", "--train_config", TG.write_config(tmp_path / "relabelled.toml", relabelled)], ["sites_sha256"]),
        (str(tmp_path / "fresh1"), ["--clip_grad", "-1"], ["--clip_grad"]),
        (str(tmp_path / "fresh2"), ["--clip_grad", "nan"], ["--clip_grad"]),
        (str(tmp_path / "fresh3"), ["--clip_grad", "0"], ["--clip_grad"]),
    ]
    for save_dir, extra, words in cases:
        before = listing(save_dir) if os.path.isdir(save_dir) else None
        with pytest.raises(SystemExit) as e:
            main(["train", "--save_dir", save_dir] + base + extra)              # a later flag overrides an earlier one
        err = capsys.readouterr().err
        assert e.value.code == 2 and all(w in err for w in words), (extra, e.value.code, err[-600:])
        assert (listing(save_dir) if os.path.isdir(save_dir) else None) == before, extra
    # the no-clipping fingerprint differs from every clipped one, and min_reads is part of it
    a2 = CMD.argparser().parse_args(base[:-2] + ["--save_dir", run, "--resume"])
    with pytest.raises(CMD.Refusal, match="clip_grad"):
        CMD.plan(a2)
    # what is accepted: the checkpoint of epoch 2, not the directory without a state file
    ok = parsed(["--resume"], run)[1]
    assert ok["resume"]["epoch"] == 2 and ok["weights"].size == 7997 and ok["resume"]["optimizer"]["n_steps"] == 41
    r = run_train("--save_dir", run, *base, "--resume", "--seed", "4")          # and once as the command itself
    assert r.returncode == 2 and "seed" in r.stderr and "Traceback" not in r.stderr
