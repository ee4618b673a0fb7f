"""MILModel: the m6anet.toml model as a torch.nn.Module whose training-mode forward and backward are the HIP training kernels
(include/m6a.h: m6a_train_forward / m6a_train_backward; m6anet_amd/csrc/m6a_train.hip).  It stands where the reference builds
`MILModel(model_config)` (m6anet/scripts/train.py), so every loss, sampler, optimizer and scheduler torch has drives the kernels:

    model = MILModel("HCT116_RNA002")                       # or a 7 997-float blob, or None = init_weights(0)
    opt = torch.optim.Adam(model.parameters(), lr=4e-4)
    s = model(batch)                                        # batch: train_collate's {'X' [B, bag, 9] float32, 'kmer' [B, bag, 3] int64}
    criterion(s, y).backward(); opt.step()

The cut is at s: forward returns the site probabilities s [B], backward takes dL/ds [B] from autograd.  There is no gradient with
respect to X and no double backward.  torch here is plumbing -- parameters, autograd's tape, streams -- and nothing in this file
computes a layer; a missing kernel is an error, not a fall-back to eager torch.

Storage.  The nine parameters and the two running statistics are views of one flat 7 997-float tensor in blob order, so the
kernels read what an in-place optimizer step, load_state_dict or a copy_ left there.  A tensor that was moved away (`p.data = ...`,
`.to(...)`) is copied back into a flat tensor at the next forward, and aliases it again from then on.

The reference's 'kmer' repeats a site's three ids over its reads; the module takes kmer[:, 0, :] and does not look at the others.

This module imports torch; `import m6anet_amd` does not import this module.
"""
import numpy as np
import torch
from torch.autograd.function import once_differentiable

from . import _lib
from .constants import N_WEIGHT_FLOATS, PRETRAINED_CONFIGS
from .engine import STATE_DICT_KEYS, M6ANetEngine, init_weights, load_weights

_RUNNING = slice(2832, 3132)                     # running_mean | running_var in the blob
MAX_BAG = 64                                     # M6A_MAX_SAMPLES


class _Node(torch.nn.Module):
    """A container that only gives the parameters the reference's names."""


def _child(node, name):
    if name not in node._modules:
        node.add_module(name, _Node())
    return node._modules[name]


class _Step(torch.autograd.Function):
    """s = forward(weights, batch) on the kernels; backward hands dL/ds to them.  The parameters are inputs so that autograd routes
    their gradients; their values reach the kernels through the flat tensor."""

    @staticmethod
    def forward(ctx, model, X, kmers, bag, *params):
        tr = model._trainer()
        model._engine.use_torch_stream()
        tr.set_weights(model._flat)
        s, ticket = tr.forward(X, kmers, bag)
        tr.running_stats(out=model._flat[_RUNNING])          # the buffers are views of these 300 floats
        model._stat_writes += 1
        model._tracked().add_(1)
        ctx.model, ctx.ticket = model, ticket
        return s

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_s):
        model = ctx.model
        g = grad_s.to(torch.float32).contiguous()
        model._engine.use_torch_stream()
        try:
            G = model._trainer().backward(ctx.ticket, g)
        except _lib.M6AError as e:
            raise RuntimeError("MILModel: backward() of a forward whose activations are gone -- the kernels keep the latest forward's "
                               "only, so call backward() before the next training-mode forward on this module.  %s" % e) from None
        grads, o = [], 0
        for key, shape in STATE_DICT_KEYS:
            n = int(np.prod(shape))
            if "running_" not in key:
                grads.append(G[o:o + n].view(shape))
            o += n
        return (None, None, None, None) + tuple(grads)


class MILModel(torch.nn.Module):
    def __init__(self, weights=None, device=0, bag=20):
        """weights: a 7 997-float blob, a pretrained model's name, or None = init_weights(0).  device: a GPU index or torch device
        ("cpu" builds the module for its state_dict only: a forward needs the GPU).  bag: the reads per site of a 2-D X
        [B * bag, 9]; a 3-D X [B, bag, 9] carries its own."""
        super().__init__()
        if weights is None:
            w = init_weights(0)
        elif isinstance(weights, str):
            if weights not in PRETRAINED_CONFIGS:
                raise ValueError("weights: %r is not a pretrained model (%s)" % (weights, ", ".join(PRETRAINED_CONFIGS)))
            w = load_weights(weights)
        else:
            w = np.ascontiguousarray(weights.detach().cpu().numpy() if torch.is_tensor(weights) else weights, np.float32).ravel()
        if w.size != N_WEIGHT_FLOATS:
            raise ValueError("weights must have %d floats" % N_WEIGHT_FLOATS)
        if not 1 <= int(bag) <= MAX_BAG:
            raise ValueError("bag must be in 1..%d" % MAX_BAG)
        self.bag = int(bag)
        dev = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
        if dev.type == "cuda" and dev.index is None:
            dev = torch.device("cuda", 0)
        self._flat = torch.from_numpy(w.copy()).to(dev)
        self._tensors = []                                   # [(owner node, attribute, offset, shape)] in blob order
        o = 0
        for key, shape in STATE_DICT_KEYS:
            *path, leaf = key.split(".")
            node = self
            for name in path:
                node = _child(node, name)
            n = int(np.prod(shape))
            view = self._flat[o:o + n].view(shape)
            if leaf.startswith("running_"):
                node.register_buffer(leaf, view)
                if leaf == "running_var":
                    node.register_buffer("num_batches_tracked", torch.zeros((), dtype=torch.int64, device=dev))
                    object.__setattr__(self, "_bn", node)        # not a second registration of the node
            else:
                node.register_parameter(leaf, torch.nn.Parameter(view))
            self._tensors.append((node, leaf, o, tuple(shape)))
            o += n
        self._engine = self._tr = self._eval = None
        self._eval_key = None
        self._stat_writes = self._repacks = 0

    # -- storage ----------------------------------------------------------------------------
    def _tracked(self):
        return self._bn.num_batches_tracked

    def _ordered(self):
        return [getattr(node, leaf) for node, leaf, _, _ in self._tensors]

    def _pack(self):
        """The flat tensor, with every parameter and buffer a view of it: a tensor that was moved is copied back in."""
        flat, base = self._flat, self._flat.data_ptr()
        ts = self._ordered()
        if all(t.device == flat.device and t.dtype == torch.float32 and t.is_contiguous() and t.data_ptr() == base + 4 * o
               for t, (_, _, o, _) in zip(ts, self._tensors)):
            return flat
        dev = ts[0].device
        new = torch.empty(N_WEIGHT_FLOATS, dtype=torch.float32, device=dev)
        with torch.no_grad():
            for t, (node, leaf, o, shape) in zip(ts, self._tensors):
                if tuple(t.shape) != shape:
                    raise ValueError("%s has shape %s, not %s" % (leaf, tuple(t.shape), shape))
                view = new[o:o + t.numel()].view(shape)
                view.copy_(t)
                t.data = view
        self._flat = new
        self._repacks += 1
        if self._tracked().device != dev:
            self._bn.num_batches_tracked = self._tracked().to(dev)
        return new

    def blob(self):
        """The 7 997 floats as they stand, running statistics included: what M6ANetEngine(weights=...) takes."""
        return self._pack().detach().cpu().numpy().copy()

    def load_blob(self, weights, num_batches_tracked=0):
        """The inverse of blob(): the 7 997 floats into the parameters and buffers, in place."""
        w = np.ascontiguousarray(weights, np.float32).ravel()
        if w.size != N_WEIGHT_FLOATS:
            raise ValueError("weights must have %d floats" % N_WEIGHT_FLOATS)
        flat = self._pack()
        with torch.no_grad():
            for t, (_, _, o, shape) in zip(self._ordered(), self._tensors):      # through the tensors: autograd sees them change
                t.copy_(torch.from_numpy(w[o:o + t.numel()].reshape(shape)).to(flat.device))
            self._tracked().fill_(int(num_batches_tracked))

    def _device_index(self):
        flat = self._pack()
        if flat.device.type != "cuda":
            raise TypeError("MILModel is on %s: its forward runs HIP kernels and needs the module on a GPU" % flat.device)
        return flat.device.index or 0

    def _trainer(self):
        dev = self._device_index()
        if self._engine is None or self._engine.device != dev:
            self.close()
            self._engine = M6ANetEngine(weights=self.blob(), device=dev)
            self._tr = self._engine.trainer(self.blob())
        return self._tr

    def close(self):
        """Frees the native contexts; the next forward makes new ones."""
        for name in ("_tr", "_eval", "_engine"):
            h = getattr(self, name, None)
            if h is not None:
                h.close()
            setattr(self, name, None)
        self._eval_key = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __getstate__(self):
        """copy.deepcopy and pickle take the tensors; the native contexts are made anew by the copy's first forward."""
        d = self.__dict__.copy()
        d["_engine"] = d["_tr"] = d["_eval"] = d["_eval_key"] = None
        return d

    # -- forward ----------------------------------------------------------------------------
    def _check(self, X, site_kmers):
        """-> (X, uint8 k-mers [B, 3], B, bag) or raises TypeError / ValueError; no kernel has run."""
        for name, t in (("X", X), ("site_kmers", site_kmers)):
            if not torch.is_tensor(t):
                raise TypeError("%s must be a torch tensor, not %s" % (name, type(t).__name__))
        dev = self._device_index()
        for name, t in (("X", X), ("site_kmers", site_kmers)):
            if not t.is_cuda or (t.device.index or 0) != dev:
                raise TypeError("%s is on %s; the module is on cuda:%d" % (name, t.device, dev))
        if X.dtype != torch.float32:
            raise TypeError("X must be float32, not %s" % X.dtype)
        if site_kmers.dtype not in (torch.int64, torch.uint8):
            raise TypeError("site_kmers must be int64 (the reference's) or uint8, not %s" % site_kmers.dtype)
        if X.dim() == 3 and X.shape[2] == 9:
            B, bag = int(X.shape[0]), int(X.shape[1])
        elif X.dim() == 2 and X.shape[1] == 9 and X.shape[0] % self.bag == 0:
            B, bag = int(X.shape[0]) // self.bag, self.bag
        else:
            raise ValueError("X must be [B, bag, 9] (or [B * %d, 9]), not %s" % (self.bag, tuple(X.shape)))
        if not 1 <= bag <= MAX_BAG:
            raise ValueError("bag must be in 1..%d, not %d" % (MAX_BAG, bag))
        if B < 1 or tuple(site_kmers.shape) != (B, 3):
            raise ValueError("site_kmers must be [%d, 3], not %s" % (B, tuple(site_kmers.shape)))
        if not X.is_contiguous() or not site_kmers.is_contiguous():
            raise ValueError("X and site_kmers must be contiguous")
        if site_kmers.dtype == torch.int64:                  # an id outside a byte must not wrap into 0..65: 255 is refused later
            k = site_kmers
            site_kmers = torch.where((k < 0) | (k > 255), torch.full_like(k, 255), k).to(torch.uint8)
        return X, site_kmers, B, bag

    def forward_bags(self, X, site_kmers):
        """X [B, bag, 9] float32, site_kmers [B, 3] int64 or uint8 -> s [B]."""
        X, km, B, bag = self._check(X, site_kmers)
        if self.training:
            if X.requires_grad:
                raise RuntimeError("MILModel: X.requires_grad is set, and the kernels compute no gradient with respect to X")
            if B * bag < 2:
                raise ValueError("a training-mode forward needs at least 2 reads (batch norm over one value is undefined)")
            try:
                return _Step.apply(self, X, km, bag, *[t for t in self._ordered() if isinstance(t, torch.nn.Parameter)])
            except _lib.M6AError as e:
                if e.code == -1:
                    raise ValueError("MILModel.forward: %s" % e) from None
                raise
        if torch.is_grad_enabled():
            raise RuntimeError("MILModel: an eval-mode forward runs the inference kernels, which keep nothing for a backward: "
                               "call it under torch.no_grad()")
        key = (self._flat.data_ptr(), self._repacks, self._stat_writes) + tuple(t._version for t in self._ordered())
        if self._eval is None or key != self._eval_key:
            if self._eval is not None:
                self._eval.close()
            self._eval = M6ANetEngine(weights=self.blob(), device=self._device_index())
            self._eval_key = key
        self._eval.use_torch_stream()
        return self._eval.forward(X, km, bag)

    def forward(self, batch):
        """batch: the reference's train_collate dictionary, 'X' [B, bag, 9] float32 and 'kmer' [B, bag, 3] int64 -> s [B], as the
        reference's MILModel.forward.  Of 'kmer' only [:, 0, :] is read: the reference repeats a site's ids over its reads."""
        X, kmer = batch["X"], batch["kmer"]
        if not torch.is_tensor(kmer):
            raise TypeError("batch['kmer'] must be a torch tensor, not %s" % type(kmer).__name__)
        if kmer.dim() != 3 or kmer.shape[2] != 3 or (torch.is_tensor(X) and X.dim() == 3 and kmer.shape[:2] != X.shape[:2]):
            raise ValueError("batch['kmer'] must be [B, bag, 3] beside X [B, bag, 9], not %s" % (tuple(kmer.shape),))
        return self.forward_bags(X, kmer[:, 0, :].contiguous())
