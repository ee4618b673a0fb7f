"""Gradient clipping, the optimizer state and --resume on the GPU (m6anet_amd/csrc/m6a_train.hip: train_grad_kernel,
train_clip_adam_kernel; include/m6a.h: m6a_train_set_clip, _last_norm, _state_get, _state_set).

The clipped step is held to torch (tests/train_clip_torch.py: clip_grad_norm_ between backward() and step()) under the bar of
tests/train_torch.py, E_hip <= 8 E_ref per tensor over the four seeds of test_gpu_train.py, the total norm being one more judged
quantity.  Everything else here is bit for bit: an unclipped step with clipping on against clipping off, an epoch against its steps,
a trainer rebuilt from weights() and optimizer_state() against the one they were taken from, and `train --resume` against the run
that was never interrupted."""
import json
import os

import numpy as np
import pytest
import torch

import train_clip_torch as CT
import train_torch as TT
from m6anet_amd import _lib
from m6anet_amd.engine import M6ANetEngine, load_weights
from test_gpu_train import epoch_inputs

pytestmark = pytest.mark.gpu
HCT = "HCT116_RNA002"


@pytest.fixture(scope="module")
def eng():
    e = M6ANetEngine(pretrained_model=HCT)
    yield e
    e.close()


@pytest.fixture(scope="module")
def bundled():
    return CT.bundled()


def hip_run(eng, w, batches, max_norm=None, **cfg):
    """max_norm None: a trainer set_clip is never called on."""
    tr = eng.trainer(w, clip_grad=max_norm, **cfg)
    losses, preds, norms = [], [], []
    for X, km, y, bag in batches:
        loss, pred = tr.step(X, km, y, bag)
        losses.append(loss)
        preds.append(pred)
        if max_norm:
            norms.append(tr.last_norm())
    out = {"loss": np.asarray(losses, np.float32), "y_pred": preds, "grad": tr.grads(), "blob": tr.weights(), "norm": np.asarray(norms, np.float64),
           "state": tr.optimizer_state()}
    tr.close()
    return out


def same_bits(a, b, keys=("loss", "grad", "blob")):
    for k in keys:
        assert a[k].tobytes() == b[k].tobytes(), k
    assert all(p.tobytes() == q.tobytes() for p, q in zip(a["y_pred"], b["y_pred"]))
    if "state" in a and "state" in b:
        assert a["state"]["n_steps"] == b["state"]["n_steps"]
        assert a["state"]["m"].tobytes() == b["state"]["m"].tobytes() and a["state"]["v"].tobytes() == b["state"]["v"].tobytes()


def clipped_steps(eng, bundled, B, bag, weight_decay, seeds=CT.SEEDS):
    w = load_weights(HCT)
    e_ref, e_hip = [], []
    for s in seeds:
        batches = CT.case_batches(bundled, B, bag, s)
        max_norm = 0.25 * CT.first_norm(w, batches, weight_decay=weight_decay)
        CT.conditions(w, batches, max_norm, clipped=True, weight_decay=weight_decay)
        f32 = CT.run(w, batches, torch.float32, max_norm, weight_decay=weight_decay)
        f64 = CT.run(w, batches, torch.float64, max_norm, weight_decay=weight_decay)
        got = hip_run(eng, w, batches, np.float32(max_norm), weight_decay=weight_decay)
        assert all(np.isfinite(got[k]).all() for k in ("loss", "grad", "blob", "norm")) and len(got["norm"]) == len(batches)
        assert (got["norm"] > 2 * max_norm * (1 - 1e-3)).all()                  # it clipped
        e_ref.append(CT.errors(f32, f64))
        e_hip.append(CT.errors(got, f64))
    TT.hold("clipped %dx%d wd %g" % (B, bag, weight_decay), TT.pooled(e_ref), TT.pooled(e_hip))


@pytest.mark.parametrize("weight_decay", [0.0, 1e-2])
@pytest.mark.parametrize("B,bag", CT.SHAPES)
def test_clipped_steps(eng, bundled, B, bag, weight_decay):
    """Three steps at 0.25 T; with weight_decay, because clipping precedes the decay term."""
    clipped_steps(eng, bundled, B, bag, weight_decay)


def test_clipped_steps_beyond_one_tile_per_chunk(eng, bundled):
    """8 240 reads: chunks of 64 reads, two tiles each, the last one a full tile and 16 reads (tests/train_regimes.py: chunking).
    train_grad_kernel folds the same 129 parts train_adam_kernel folds with clipping off."""
    clipped_steps(eng, bundled, 412, 20, 0.0)


@pytest.mark.parametrize("B,bag", CT.SHAPES)
def test_unclipped_steps_with_clipping_on_are_the_default_steps_bits(eng, bundled, B, bag):
    """At 4 T the coefficient is exactly 1: the seven-launch path folds in the default path's order."""
    w = load_weights(HCT)
    for s in CT.SEEDS[:2]:
        batches = CT.case_batches(bundled, B, bag, s)
        max_norm = 4 * CT.first_norm(w, batches)
        want_norm = CT.conditions(w, batches, max_norm, clipped=False)["norm"]
        off, on = hip_run(eng, w, batches), hip_run(eng, w, batches, max_norm)
        same_bits(on, off)
        assert np.abs(on["grad"]).max() > 0 and not np.array_equal(on["blob"], w)
        assert np.allclose(on["norm"], want_norm, rtol=1e-3)                   # the norm is reported all the same (judged above)


def test_launch_counts_and_set_clip_zero(eng, bundled):
    w = load_weights(HCT)
    batches = CT.case_batches(bundled, 13, 20, 11)
    X, km, y, bag = batches[0]
    counts = {}
    for name, max_norm in (("off", None), ("zero", 0.0), ("on", 0.5)):
        tr = eng.trainer(w, clip_grad=max_norm)
        s0 = tr.stats()
        tr.step(X, km, y, bag)
        s1 = tr.stats()
        counts[name] = (s1["n_launches"] - s0["n_launches"] - 1, s1["n_syncs"] - s0["n_syncs"])       # - 1: the argument check
        tr.close()
    assert counts["off"][0] == counts["zero"][0] == 6 and counts["on"][0] == 7, counts
    assert counts["off"][1] == counts["zero"][1] == counts["on"][1], counts
    same_bits(hip_run(eng, w, batches, 0.0), hip_run(eng, w, batches))          # set_clip(0): the bits of a trainer never touched
    tr = eng.trainer(w, clip_grad=0.5)                                          # on, then off again: the default chain
    tr.step(X, km, y, bag)
    tr.set_clip(0)
    s0 = tr.stats()
    tr.step(X, km, y, bag)
    assert tr.stats()["n_launches"] - s0["n_launches"] == 1 + 6
    with pytest.raises(_lib.M6AError, match="clipping is off"):
        tr.last_norm()
    tr.close()


def test_same_state_and_batch_give_the_same_bits_with_clipping_on(eng, bundled):
    w = load_weights(HCT)
    batches = CT.case_batches(bundled, 256, 20, 12)
    max_norm = 0.25 * CT.first_norm(w, batches)
    a, b = hip_run(eng, w, batches, max_norm), hip_run(eng, w, batches, max_norm)
    same_bits(a, b)
    assert a["norm"].tobytes() == b["norm"].tobytes() and (a["norm"] > max_norm).all()
    assert not np.array_equal(a["blob"], hip_run(eng, w, batches)["blob"])       # and clipping changed the step


@pytest.mark.parametrize("bs", [16, 101])
def test_epoch_equals_its_steps_bit_for_bit_with_clipping_on(eng, bundled, bs):
    from m6anet_amd.engine import train_sample
    X, km, off, y, order = epoch_inputs(bundled)
    assert len(order) % bs                                                     # the last batch is short
    w, seed, bag, max_norm = load_weights(HCT), 77, 20, 0.05
    idx = train_sample(off, order, bag, seed)
    tr = eng.trainer(w, clip_grad=max_norm)
    s0 = tr.stats()
    loss, pred = tr.epoch(X, km, off, y, order, bs, bag, seed)
    s1 = tr.stats()
    ew, eg, en, es = tr.weights(), tr.grads(), tr.last_norm(), tr.optimizer_state()
    tr.close()
    n_steps = -(-len(order) // bs)
    assert s1["n_steps"] - s0["n_steps"] == n_steps and s1["n_launches"] - s0["n_launches"] == 2 + 7 * n_steps
    assert s1["n_syncs"] - s0["n_syncs"] == 2                                   # host arrays: as with clipping off (test_gpu_train.py)
    tr = eng.trainer(w, clip_grad=max_norm)
    clipped = 0
    for k in range(n_steps):
        o = order[k * bs:(k + 1) * bs]
        l, p = tr.step(X[idx[k * bs * bag:(k + 1) * bs * bag]], km[o], y[o], bag)
        assert np.float32(l).tobytes() == loss[k].tobytes(), k
        assert p.tobytes() == pred[k * bs:(k + 1) * bs].tobytes(), k
        clipped += tr.last_norm() > max_norm
    assert tr.weights().tobytes() == ew.tobytes() and tr.grads().tobytes() == eg.tobytes() and np.float32(tr.last_norm()).tobytes() == np.float32(en).tobytes()
    st = tr.optimizer_state()
    assert st["n_steps"] == es["n_steps"] == n_steps and st["m"].tobytes() == es["m"].tobytes() and st["v"].tobytes() == es["v"].tobytes()
    tr.close()
    assert clipped > 0 and np.isfinite(loss).all() and np.isfinite(ew).all()


def test_epoch_on_device_tensors_waits_once_with_clipping_on(eng, bundled):
    X, km, off, y, order = epoch_inputs(bundled)
    w = load_weights(HCT)
    tr = eng.trainer(w, clip_grad=0.05)
    host = tr.epoch(X, km, off, y, order, 16, 20, 9) + (tr.weights(), tr.grads())
    tr.close()
    dX, dK, dO, dY = (torch.from_numpy(a).cuda() for a in (X, km, off, y))
    syncs = {}
    for n in (32, len(order)):
        tr = eng.trainer(w, clip_grad=0.05)
        s0 = tr.stats()
        loss, pred = tr.epoch(dX, dK, dO, dY, torch.from_numpy(order[:n]).cuda(), 16, 20, 9)
        s1 = tr.stats()
        eng.sync()
        syncs[n] = s1["n_syncs"] - s0["n_syncs"]
        assert s1["n_launches"] - s0["n_launches"] == 2 + 7 * -(-n // 16)
        dev = (loss.cpu().numpy(), pred.cpu().numpy(), tr.weights(), tr.grads())
        tr.close()
    assert syncs[32] == syncs[len(order)] == 1, syncs
    for a, b in zip(host, dev):
        assert a.tobytes() == b.tobytes()


@pytest.mark.parametrize("max_norm", [None, 0.05])
def test_optimizer_state_makes_the_trainer_it_was_taken_from(eng, bundled, max_norm):
    w = load_weights(HCT)
    batches = [CT.make_batch(bundled, 32, 20, 600 + k) for k in range(8)]
    fresh = eng.trainer(w, clip_grad=max_norm)
    st0 = fresh.optimizer_state()
    assert st0["n_steps"] == 0 and st0["m"].shape == st0["v"].shape == (7997,) and not st0["m"].any() and not st0["v"].any()
    for b in batches[:5]:
        fresh.step(*b)
    blob, st = fresh.weights(), fresh.optimizer_state()
    assert st["n_steps"] == 5 and st["m"].any() and (st["v"] >= 0).all() and st["v"].any()
    stat = slice(2832, 3132)                                                    # the 300 running-statistic slots
    assert not st["m"][stat].any() and not st["v"][stat].any()

    def next_three(tr):
        losses, preds = [], []
        for b in batches[5:]:
            loss, pred = tr.step(*b)
            losses.append(loss)
            preds.append(pred)
        out = {"loss": np.asarray(losses, np.float32), "y_pred": preds, "grad": tr.grads(), "blob": tr.weights(), "state": tr.optimizer_state()}
        tr.close()
        return out

    want = next_three(fresh)
    rebuilt = eng.trainer(blob, clip_grad=max_norm)
    rebuilt.load_optimizer_state(st)
    back = rebuilt.optimizer_state()
    assert back["n_steps"] == 5 and back["m"].tobytes() == st["m"].tobytes() and back["v"].tobytes() == st["v"].tobytes()
    got = next_three(rebuilt)
    same_bits(got, want)
    assert got["state"]["n_steps"] == 8
    weights_only = next_three(eng.trainer(blob, clip_grad=max_norm))            # what --init x.bin does: Adam restarts at t = 0
    assert weights_only["state"]["n_steps"] == 3
    assert weights_only["blob"].tobytes() != want["blob"].tobytes()
    assert weights_only["loss"][0].tobytes() == want["loss"][0].tobytes()       # the same weights: the first loss agrees, the update does not
    assert weights_only["loss"][1:].tobytes() != want["loss"][1:].tobytes()


def test_every_new_refusal_then_a_correct_call(eng, bundled):
    """A refused call changes nothing: a twin trainer that never sees the refused calls stays bit-identical throughout."""
    w = load_weights(HCT)
    batch = CT.make_batch(bundled, 8, 20, 700)
    a, twin = eng.trainer(w, clip_grad=0.05), eng.trainer(w, clip_grad=0.05)
    for t in (a, twin):
        t.step(*batch)
    good = a.optimizer_state()
    m_dev, v_dev = torch.zeros(7997, device="cuda"), torch.zeros(7997, device="cuda")
    m_host, v_host = np.zeros(7997, np.float32), np.zeros(7997, np.float32)
    chk, L, h = a._engine._chk, a._L, a._h

    def bad_state(which, index, value, n_steps=1):
        st = {"m": good["m"].copy(), "v": good["v"].copy(), "n_steps": n_steps}
        if which:
            st[which][index] = value
        return lambda: a.load_optimizer_state(st)

    cases = [
        (lambda: a.set_clip(-1.0), "max_norm"), (lambda: a.set_clip(float("nan")), "max_norm"), (lambda: a.set_clip(float("inf")), "max_norm"),
        (lambda: a.set_clip(float("-inf")), "max_norm"),
        (lambda: chk(L.m6a_train_state_get(h, m_dev.data_ptr(), v_host.ctypes.data, None)), "host pointers"),
        (lambda: chk(L.m6a_train_state_get(h, m_host.ctypes.data, v_dev.data_ptr(), None)), "host pointers"),
        (lambda: chk(L.m6a_train_state_set(h, m_dev.data_ptr(), v_host.ctypes.data, 1)), "host pointers"),
        (lambda: chk(L.m6a_train_state_set(h, m_host.ctypes.data, v_dev.data_ptr(), 1)), "host pointers"),
        (bad_state(None, 0, 0, n_steps=-1), "n_steps"),
        (bad_state("v", 10, -1e-30), "v[10]"), (bad_state("v", 7996, np.nan), "v[7996]"), (bad_state("v", 0, np.inf), "v[0]"),
        (bad_state("m", 5, np.nan), "m[5]"), (bad_state("m", 7996, np.inf), "m[7996]"), (bad_state("m", 3000, -np.inf), "m[3000]"),
    ]
    for call, word in cases:
        with pytest.raises(_lib.M6AError) as e:
            call()
        assert e.value.code == -1 and word in str(e.value), str(e.value)
        assert a.last_norm() == twin.last_norm()                                # the clip setting and the norm are still there
        ra, rt = a.step(*batch), twin.step(*batch)                              # ... and the next correct call has the twin's bits
        assert np.float32(ra[0]).tobytes() == np.float32(rt[0]).tobytes() and ra[1].tobytes() == rt[1].tobytes()
        sa, st = a.optimizer_state(), twin.optimizer_state()
        assert a.weights().tobytes() == twin.weights().tobytes() and a.grads().tobytes() == twin.grads().tobytes()
        assert sa["n_steps"] == st["n_steps"] and sa["m"].tobytes() == st["m"].tobytes() and sa["v"].tobytes() == st["v"].tobytes()
    with pytest.raises(_lib.M6AError, match="max_norm"):
        eng.trainer(w, clip_grad=-2.0)
    a.close()
    twin.close()
    plain = eng.trainer(w)                                                      # the default chain does not compute the norm
    plain.step(*batch)
    with pytest.raises(_lib.M6AError, match="clipping is off") as e:
        plain.last_norm()
    assert e.value.code == -1
    plain.set_clip(0.05)
    with pytest.raises(_lib.M6AError, match="no step"):
        plain.last_norm()
    plain.step(*batch)
    assert plain.last_norm() > 0
    plain.close()


def results_but_time(path):
    d = json.load(open(path))
    d.pop("compute_time")
    return d


@pytest.mark.parametrize("clip", [None, "1.0"])
def test_resume_is_the_run_that_was_never_interrupted(tmp_path, capsys, clip):
    import train_gen as TG
    from m6anet_amd.__main__ import main
    data = TG.write_dir(str(tmp_path / "data"))
    cfg = TG.write_config(tmp_path / "train.toml", data, batch_size=16)
    base = ["train", "--train_config", cfg, "--save_per_epoch", "1", "--num_iterations", "2", "--n_processes", "2", "--seed", "3"]
    base += ["--clip_grad", clip] if clip else []
    whole, cut = tmp_path / "whole", tmp_path / "cut"
    main(base + ["--save_dir", str(whole), "--epochs", "4"])
    main(base + ["--save_dir", str(cut), "--epochs", "2"])
    assert sorted(os.listdir(cut / "model_states")) == ["1", "2"] and len(json.load(open(cut / "val_results.json"))["avg_loss"]) == 2
    capsys.readouterr()
    main(base + ["--save_dir", str(cut), "--epochs", "4", "--resume"])
    out = capsys.readouterr().out
    assert "Resuming from epoch 2" in out and out.count("Epoch:[") == 2 and "Epoch:[3/4]" in out and out.count("Test Loss:") == 3
    for e in (1, 2, 3, 4):
        for name in ("model_states.bin", "trainer_state.npz"):
            assert (whole / "model_states" / str(e) / name).is_file() and (cut / "model_states" / str(e) / name).is_file(), (e, name)
        a, b = (open(d / "model_states" / str(e) / "model_states.bin", "rb").read() for d in (whole, cut))
        assert a == b and len(a) == 7997 * 4, e
        za, zb = (np.load(d / "model_states" / str(e) / "trainer_state.npz") for d in (whole, cut))
        assert all(za[k].tobytes() == zb[k].tobytes() for k in za.files if not k.endswith("compute_time")), e
        assert 60e3 < os.path.getsize(whole / "model_states" / str(e) / "trainer_state.npz") < 80e3
    for c in ("avg_loss", "roc_auc", "pr_auc"):
        assert open(whole / (c + ".bin"), "rb").read() == open(cut / (c + ".bin"), "rb").read(), c
        ta, tb = results_but_time(whole / ("test_results_%s.json" % c)), results_but_time(cut / ("test_results_%s.json" % c))
        assert ta == tb and {"y_pred", "y_true", "roc_auc", "pr_auc", "avg_loss"} <= set(ta)
    for name in ("train_results.json", "val_results.json"):
        ra, rb = results_but_time(whole / name), results_but_time(cut / name)
        assert ra == rb and all(len(v) == 4 for v in ra.values()), name
    assert len(json.load(open(cut / "val_results.json"))["compute_time"]) == 4
    info = json.load(open(cut / "train_info.json"))["train_config"]
    assert info["clip_grad"] == (float(clip) if clip else None) and info["epochs"] == 4
