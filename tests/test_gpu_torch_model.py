"""MILModel (m6anet_amd/torch_model.py) on the GPU: the training kernels behind torch autograd, cut at s (include/m6a.h:
m6a_train_forward / m6a_train_backward).  Cases, seeds and the bar: tests/torch_model_cases.py; their conditions, without a GPU:
tests/test_torch_model_host.py.

Forward: s and the running statistics are Trainer.step's bits.  Backward under a given dL/ds = g: per family and tensor,
E_hip = |module.grad - Restated float64| <= 8 E_ref = 8 |Restated float32 - Restated float64| (train_torch.hold).  Every figure is
printed before it is judged and, with M6A_TRAIN_PARITY_JSON set, written to that file (profiles/r28_torch_model_parity.json is one
such run).  Then the losses through autograd, three Adam steps against tests/golden/train_step.npz, and the plumbing: aliasing,
accumulation, retain_graph, tickets, eval mode, refusals."""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

import torch_model_cases as MC
import train_clip_torch as CT
import train_regimes as TR
import train_statement as TS
import train_torch as TT
from m6anet_amd import _lib
from m6anet_amd.engine import STATE_DICT_KEYS, M6ANetEngine, load_weights
from m6anet_amd.torch_model import MILModel

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(REPO, "tests", "golden")
HCT = "HCT116_RNA002"
RUNNING = slice(2832, 3132)


@pytest.fixture(scope="module")
def model():
    m = MILModel(HCT)
    yield m
    m.close()


@pytest.fixture(scope="module")
def eng():
    e = M6ANetEngine(pretrained_model=HCT)
    yield e
    e.close()


def on_device(batch):
    """-> X [B, bag, 9] float32, site_kmers [B, 3] int64, y [B] float32, on the GPU."""
    X, km, y, bag = batch
    return (torch.from_numpy(np.ascontiguousarray(X, np.float32).reshape(-1, bag, 9)).cuda(), torch.from_numpy(np.asarray(km).astype(np.int64)).cuda(),
            torch.from_numpy(np.asarray(y, np.float32)).cuda())


def grad_blob(m):
    """The module's .grad tensors in blob order, zeros in the running-statistic slots (and for a parameter without a .grad)."""
    out, o = np.zeros(TS.N_FLOATS, np.float32), 0
    params = dict(m.named_parameters())
    for key, shape in STATE_DICT_KEYS:
        n = int(np.prod(shape))
        if key in params and params[key].grad is not None:
            out[o:o + n] = params[key].grad.detach().cpu().numpy().ravel()
        o += n
    return out


def forward_backward(m, w, batch, g=None, loss=None):
    """load w, one training-mode forward and one backward -> (s, gradient in blob order, loss value)"""
    m.load_blob(w)
    m.train()
    m.zero_grad(set_to_none=True)
    X, km, y = on_device(batch)
    s = m.forward_bags(X, km)
    value = None
    if g is not None:
        s.backward(torch.from_numpy(g).cuda())
    else:
        value = MC.LOSSES[loss](s, y)
        value.backward()
    return s.detach().cpu().numpy(), grad_blob(m), None if value is None else value.item()


# ---- forward -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,bag", MC.SHAPES)
def test_forward_is_the_step_bit_for_bit(model, eng, B, bag):
    case = MC.family_cases("HCT116", B, bag)[0]
    w, (X, km, y, _) = case["w"], case["batch"]
    tr = eng.trainer(w)
    _, pred = tr.step(X, km, y, bag)
    after = tr.weights()
    tr.close()
    dX, dK, _ = on_device(case["batch"])
    model.load_blob(w)
    model.train()
    bits = []
    for rep in range(2):
        model.load_blob(w, num_batches_tracked=rep)
        s = model({"X": dX, "kmer": dK[:, None, :].expand(B, bag, 3)})            # the reference's dictionary: ids repeated over the reads
        assert s.shape == (B,) and s.dtype == torch.float32 and s.is_cuda and s.requires_grad
        blob = model.blob()
        assert s.detach().cpu().numpy().tobytes() == pred.tobytes()
        assert blob[RUNNING].tobytes() == after[RUNNING].tobytes() and not np.array_equal(blob[RUNNING], w[RUNNING])
        trainable = np.ones(TS.N_FLOATS, bool)
        trainable[RUNNING] = False
        assert blob[trainable].tobytes() == w[trainable].tobytes()              # a forward moves nothing else
        assert int(model.state_dict()["read_level_encoder.3.layers.1.num_batches_tracked"]) == rep + 1
        bits.append((s.detach().cpu().numpy().tobytes(), blob.tobytes()))
    assert bits[0] == bits[1]
    # running statistics move once per forward and not in backward
    s.backward(torch.from_numpy(case["g"]).cuda())
    assert model.blob()[RUNNING].tobytes() == after[RUNNING].tobytes()
    assert int(model.state_dict()["read_level_encoder.3.layers.1.num_batches_tracked"]) == 2


def test_forward_and_backward_launches_and_waits(model):
    case = MC.family_cases("HCT116", 13, 20)[0]
    model.load_blob(case["w"])
    model.train()
    dX, dK, _ = on_device(case["batch"])
    tr = model._trainer()
    s0 = tr.stats()
    s = model.forward_bags(dX, dK)
    s1 = tr.stats()
    s.backward(torch.from_numpy(case["g"]).cuda())
    s2 = tr.stats()
    assert s1["n_launches"] - s0["n_launches"] == 4 and s1["n_syncs"] - s0["n_syncs"] == 1      # the k-mer check and its one wait, 3 kernels
    assert s2["n_launches"] - s1["n_launches"] == 4 and s2["n_syncs"] == s1["n_syncs"]          # the backward half: no wait
    assert s2["n_steps"] == s0["n_steps"]                                                       # Adam's t does not move


# ---- backward under a given dL/ds --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,B,bag", MC.FAMILIES)
def test_backward_under_a_given_upstream_gradient(model, kind, B, bag):
    e_ref, e_hip = [], []
    for case in MC.family_cases(kind, B, bag):
        MC.teeth(case["e_ref"], case["f64"]["grad"])
        s, grad, _ = forward_backward(model, case["w"], case["batch"], g=case["g"])
        assert np.isfinite(grad).all() and np.abs(grad).max() > 0 and not grad[RUNNING].any()
        e_ref.append(case["e_ref"])
        e_hip.append(MC.grad_errors(grad, case["f64"]["grad"]))
    TT.hold(MC.name(kind, B, bag), TT.pooled(e_ref), TT.pooled(e_hip))


# ---- losses through autograd -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("loss", sorted(MC.LOSSES))
@pytest.mark.parametrize("B,bag", MC.LOSS_SHAPES)
def test_losses_through_autograd(model, loss, B, bag):
    e_ref, e_hip = [], []
    for case in MC.loss_cases(loss, B, bag):
        assert TT.statement_run(case["w"], [case["batch"]])["y_pred"][0].max() <= 1 - 1e-3     # test_gpu_train.condition()
        MC.teeth(case["e_ref"], case["f64"]["grad"])
        s, grad, value = forward_backward(model, case["w"], case["batch"], loss=loss)
        assert np.isfinite(value) and np.isfinite(grad).all() and np.abs(grad).max() > 0
        e_ref.append(case["e_ref"])
        e_hip.append(MC.grad_errors(grad, case["f64"]["grad"]))
    TT.hold("%s through autograd %dx%d" % (loss, B, bag), TT.pooled(e_ref), TT.pooled(e_hip))


def test_three_adam_steps_against_the_fixture():
    """BCELoss and torch.optim.Adam on the module, three steps on tests/golden/train_step.npz's batch, against the fixture's own loss,
    y_pred, grad1 and blob3 (the reference's float32 run).  The measure is train_torch.errors per tensor and E_ref is
    |torch float32 - torch float64| as tests/test_train_statement.py forms it for the statement (three steps; the gradient from the
    one-step runs); the bar is the 8 that file holds the statement to against float64, not the 2 it allows a float64 subject beside
    the float32 fixture: the module is a float32 subject."""
    g = np.load(os.path.join(GOLD, "train_step.npz"))
    w = load_weights(HCT)
    batch = (g["X"].reshape(-1, 9), g["kmer"], g["y"], 20)
    threads = torch.get_num_threads()
    torch.set_num_threads(1)                                                    # as the fixture was made
    runs = {n: (TT.run(w, [batch] * n, torch.float32), TT.run(w, [batch] * n, torch.float64)) for n in (1, 3)}
    torch.set_num_threads(threads)
    e_ref = TT.errors(*runs[3])
    e_ref.update({k: v for k, v in TT.errors(*runs[1]).items() if k.startswith("grad.")})
    m = MILModel(w).train()
    opt = torch.optim.Adam(m.parameters(), lr=4e-4, betas=(0.9, 0.999), eps=1e-8)
    crit = torch.nn.BCELoss()
    X, km, y = on_device(batch)
    losses, preds, grad1 = [], [], None
    for k in range(3):
        opt.zero_grad()
        s = m.forward_bags(X, km)
        loss = crit(s, y)
        loss.backward()
        if k == 0:
            grad1 = grad_blob(m)
        opt.step()
        losses.append(np.float32(loss.item()))
        preds.append(s.detach().cpu().numpy())
    got = {"loss": np.asarray(losses), "y_pred": preds, "grad": grad1, "blob": m.blob()}
    m.close()
    want = {"loss": g["loss"], "y_pred": list(g["y_pred"]), "grad": g["grad1"].astype(np.float64), "blob": g["blob3"].astype(np.float64)}
    TT.hold("module, BCELoss + Adam, vs fixture", e_ref, TT.errors(got, want))


# ---- plumbing ----------------------------------------------------------------------------------------------------------------------
def test_after_an_optimizer_step_the_forward_is_a_fresh_module_s(model):
    case = MC.loss_cases("bce", 13, 20)[0]
    X, km, y = on_device(case["batch"])
    model.load_blob(case["w"])
    model.train()
    opt = torch.optim.SGD(model.parameters(), lr=0.05, momentum=0.9)
    for _ in range(2):
        opt.zero_grad()
        MC.weighted_bce(model.forward_bags(X, km), y).backward()
        torch.nn.utils.clip_grad_norm_(model.parameters(), 1.0)
        opt.step()
    blob = model.blob()
    assert not np.array_equal(blob, case["w"])
    fresh = MILModel(blob).train()
    a, b = model.forward_bags(X, km), fresh.forward_bags(X, km)
    assert a.detach().cpu().numpy().tobytes() == b.detach().cpu().numpy().tobytes()
    assert model.blob().tobytes() == fresh.blob().tobytes()
    # p.data = ... and load_state_dict are seen by the next forward too
    other = load_weights("arabidopsis_RNA002")
    key = "read_level_encoder.1.embedding_layer.weight"
    trained_E = fresh.state_dict()[key].clone()                                 # state_dict() hands out views of the storage
    model.load_blob(other)
    model.read_level_encoder._modules["1"].embedding_layer.weight.data = trained_E.clone()
    fresh.load_blob(other)
    fresh.load_state_dict({key: trained_E}, strict=False)
    a, b = model.forward_bags(X, km), fresh.forward_bags(X, km)
    assert a.detach().cpu().numpy().tobytes() == b.detach().cpu().numpy().tobytes()
    assert model.blob().tobytes() == fresh.blob().tobytes() and not np.array_equal(model.blob()[:132], other[:132])
    fresh.close()


def test_gradients_accumulate_and_a_retained_graph_gives_the_same_bits(model):
    ca, cb = MC.family_cases("HCT116", 13, 20)[0], MC.family_cases("HCT116", 7, 5)[1]
    w = ca["w"]
    _, ga, _ = forward_backward(model, w, ca["batch"], g=ca["g"])
    _, gb, _ = forward_backward(model, w, cb["batch"], g=cb["g"])
    model.load_blob(w)
    model.zero_grad(set_to_none=True)
    for case in (ca, cb):
        X, km, _ = on_device(case["batch"])
        model.forward_bags(X, km).backward(torch.from_numpy(case["g"]).cuda())
    assert grad_blob(model).tobytes() == (ga + gb).tobytes()
    # backward twice on one graph
    X, km, _ = on_device(ca["batch"])
    model.zero_grad(set_to_none=True)
    s = model.forward_bags(X, km)
    g = torch.from_numpy(ca["g"]).cuda()
    s.backward(g, retain_graph=True)
    first = grad_blob(model)
    model.zero_grad(set_to_none=True)
    s.backward(g)
    assert first.tobytes() == grad_blob(model).tobytes() == ga.tobytes()


def test_backward_after_a_later_forward_and_the_other_autograd_refusals(model):
    case = MC.family_cases("HCT116", 13, 20)[0]
    X, km, _ = on_device(case["batch"])
    g = torch.from_numpy(case["g"]).cuda()
    model.load_blob(case["w"])
    model.train()
    model.zero_grad(set_to_none=True)
    a = model.forward_bags(X, km)
    b = model.forward_bags(X, km)
    with pytest.raises(RuntimeError, match="a later forward on this trainer overwrote those activations"):
        a.backward(g)
    assert all(p.grad is None for p in model.parameters())
    b.backward(g)                                                               # the latest one is good
    assert np.abs(grad_blob(model)).max() > 0
    with pytest.raises(RuntimeError, match="no gradient with respect to X"):
        model.forward_bags(X.clone().requires_grad_(), km)
    s = model.forward_bags(X, km)
    first = torch.autograd.grad((s * s).sum(), list(model.parameters()), create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable|differentiate twice"):
        sum(t.sum() for t in first).backward()


def test_eval_mode_is_the_inference_engine_under_no_grad(model):
    case = MC.family_cases("HCT116", 13, 20)[0]
    X, km, _ = on_device(case["batch"])
    model.load_blob(case["w"])
    model.train()
    model.forward_bags(X, km)                                                   # moves the running statistics: eval must see them
    model.eval()
    with pytest.raises(RuntimeError, match=r"torch\.no_grad\(\)"):
        model.forward_bags(X, km)
    with torch.no_grad():
        got = model.forward_bags(X, km)
        again = model.forward_bags(X, km)
    e = M6ANetEngine(weights=model.blob())
    want = e.forward(case["batch"][0], case["batch"][1], 20)
    e.close()
    assert got.cpu().numpy().tobytes() == want.tobytes() == again.cpu().numpy().tobytes()
    with torch.no_grad():                                                       # a changed parameter is seen
        for p in model.parameters():
            p.mul_(1.01)
        changed = model.forward_bags(X, km)
    e = M6ANetEngine(weights=model.blob())
    want = e.forward(case["batch"][0], case["batch"][1], 20)
    e.close()
    assert changed.cpu().numpy().tobytes() == want.tobytes() != got.cpu().numpy().tobytes()
    model.train()


def test_refusals_change_nothing(model):
    case = MC.family_cases("HCT116", 13, 20)[0]
    X, km, _ = on_device(case["batch"])
    model.load_blob(case["w"], num_batches_tracked=7)
    model.train()
    model.forward_bags(X, km)
    before = model.blob()

    def refused(exc, word, call):
        with pytest.raises(exc, match=word):
            call()
        assert model.blob().tobytes() == before.tobytes()
        assert int(model.state_dict()["read_level_encoder.3.layers.1.num_batches_tracked"]) == 8

    for bad in (66, -1, 300):
        k2 = km.clone()
        k2[5, 1] = bad
        refused(ValueError, "site 5: k-mer id outside 0..65", lambda: model.forward_bags(X, k2))
    refused(TypeError, "is on cpu", lambda: model.forward_bags(X.cpu(), km))
    refused(TypeError, "is on cpu", lambda: model.forward_bags(X, km.cpu()))
    refused(TypeError, "float32", lambda: model.forward_bags(X.double(), km))
    refused(TypeError, "int64", lambda: model.forward_bags(X, km.int()))
    refused(ValueError, "contiguous", lambda: model.forward_bags(X.transpose(0, 1).contiguous().transpose(0, 1), km))
    refused(ValueError, r"\[B, bag, 9\]", lambda: model.forward_bags(X[:, :, :8].contiguous(), km))
    refused(ValueError, r"\[B, bag, 9\]", lambda: model.forward_bags(X.reshape(-1, 9)[:7], km))
    refused(ValueError, r"site_kmers must be \[13, 3\]", lambda: model.forward_bags(X, km[:12]))
    refused(ValueError, "bag must be in 1..64", lambda: model.forward_bags(torch.zeros(1, 65, 9, device="cuda"), km[:1]))
    refused(ValueError, "at least 2 reads", lambda: model.forward_bags(X[:1, :1].contiguous(), km[:1]))


def test_one_module_over_changing_shapes_is_four_fresh_ones(model):
    """(3, 20), (412, 20), (7, 5), (6, 33) in that order: the scratch grows after use, bag and chunk change between forwards, and a
    stale row of wpart or part would be folded into the next gradient."""
    assert TR.CHANGING_SHAPES == [(3, 20), (412, 20), (7, 5), (6, 33)]
    for B, bag in TR.CHANGING_SHAPES:
        case = MC.family_cases("HCT116", B, bag)[0]
        s, grad, _ = forward_backward(model, case["w"], case["batch"], g=case["g"])
        running = model.blob()[RUNNING]
        fresh = MILModel(case["w"])
        s2, grad2, _ = forward_backward(fresh, case["w"], case["batch"], g=case["g"])
        assert s.tobytes() == s2.tobytes() and grad.tobytes() == grad2.tobytes(), (B, bag)
        assert running.tobytes() == fresh.blob()[RUNNING].tobytes()
        fresh.close()


def test_the_c_calls_on_host_pointers_and_their_refusals(eng):
    """Trainer.forward / backward on NumPy arrays: the device path's bits; a stale ticket, new weights and a step in between are
    M6A_EINVAL with a text that says what overwrote the activations."""
    case = MC.family_cases("HCT116", 13, 20)[0]
    w, (X, km, y, bag), g = case["w"], case["batch"], case["g"]
    ref = eng.trainer(w)
    _, pred = ref.step(X, km, y, bag)
    after = ref.weights()
    ref.close()
    tr = eng.trainer(w)
    s, t1 = tr.forward(X, km, bag)
    grad = tr.backward(t1, g)
    assert tr.backward(t1, g).tobytes() == grad.tobytes() == tr.grads().tobytes()
    # the step's y_pred; its running statistics, moved by the forward and by neither backward; nothing else moved
    assert s.tobytes() == pred.tobytes() and tr.weights()[RUNNING].tobytes() == after[RUNNING].tobytes()
    assert np.delete(tr.weights(), np.arange(RUNNING.start, RUNNING.stop)).tobytes() == np.delete(w, np.arange(RUNNING.start, RUNNING.stop)).tobytes()
    m = MILModel(w)
    s_dev, grad_dev, _ = forward_backward(m, w, case["batch"], g=g)
    m.close()
    assert s.tobytes() == s_dev.tobytes() and grad.tobytes() == grad_dev.tobytes()
    assert tr.running_stats().tobytes() == tr.weights()[RUNNING].tobytes()
    s2, t2 = tr.forward(X, km, bag)
    assert t2 != t1

    def refused(word, call):
        with pytest.raises(_lib.M6AError) as e:
            call()
        assert e.value.code == -1 and word in str(e.value), str(e.value)

    refused("a later forward on this trainer overwrote those activations", lambda: tr.backward(t1, g))
    refused("was not given by m6a_train_forward", lambda: tr.backward(t2 + 1, g))
    with pytest.raises(ValueError, match="one value per site"):
        tr.backward(t2, g[:5])
    k2 = km.copy()
    k2[5, 1] = 66
    before = tr.weights()
    refused("site 5: k-mer id outside 0..65", lambda: tr.forward(X, k2, bag))
    assert tr.weights().tobytes() == before.tobytes() and tr.backward(t2, g).tobytes() == grad.tobytes()   # a refused call changes nothing
    tr.step(X, km, y, bag)
    refused("a step or an epoch on this trainer overwrote", lambda: tr.backward(t2, g))
    _, t3 = tr.forward(X, km, bag)
    tr.set_weights(w)
    refused("the weights were replaced", lambda: tr.backward(t3, g))
    refused("training = 0", lambda: eng._chk(tr._L.m6a_train_forward(tr._h, X.ctypes.data, km.ctypes.data, 13, 20, 0, s.ctypes.data, None)))
    # set_weights puts the first state back: the same forward again, and Adam's t counted the one step only
    s3, t4 = tr.forward(X, km, bag)
    assert s3.tobytes() == s.tobytes() and tr.backward(t4, g).tobytes() == grad.tobytes() and tr.stats()["n_steps"] == 1
    tr.close()


def test_the_fused_step_still_gives_the_recorded_bits(eng):
    """profiles/r21_train_clip.json holds the sha256 of the blob after each of test_gpu_train.test_ten_steps' six lists of ten 64 x 20
    batches, taken before train_fwd2_kernel became one body behind three kernels: the fused instantiation gives them still."""
    recorded = json.load(open(os.path.join(REPO, "profiles", "r21_train_clip.json")))["default_path_bits"]["blob_sha256_per_list"]
    w = load_weights(HCT)
    for s in range(6):
        tr = eng.trainer(w)
        for k in range(10):
            tr.step(*CT.make_batch(CT.bundled(), 64, 20, 300 + 20 * s + k))
        blob = tr.weights()
        tr.close()
        assert hashlib.sha256(blob.tobytes()).hexdigest() == recorded[s], s
