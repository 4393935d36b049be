"""build_model(args) drop-in (reference: model/build_model.py:5-10 ->
model/all_models.py:29-130) returning a model object with the nn.Module surface
the reference's driver touches (main.py:73-77, 181-184, 218-222, 361-366):
``net(x) -> (feature, logits)``, ``train()/eval()``, ``state_dict()/
load_state_dict()`` with torchvision key names, ``to()/cuda()/cpu()``,
``copy.deepcopy``.

In train mode ``net(x)`` is differentiable: it runs the engine's train-mode
forward and returns outputs whose autograd node, on ``loss.backward()``, runs the
engine's backward into a gradient accumulator (``fm_backward_grads``);
``fedmlp_amd.optim.Adam(net)`` steps the weights from it.  The weights are not
torch tensors, so ``torch.optim.*(net.parameters())`` does not train a HipNet.
The input is a differentiable argument: when ``x`` requires grad, the same
backward also forms d loss / d x (``fm_backward_grads_x``: the stem's data
gradient) and autograd accumulates it into ``x.grad`` -- FGSM / PGD, virtual
adversarial training, input-gradient penalties, saliency.  ``net.freeze_bn()``
makes the train-mode call apply the BatchNorm RUNNING statistics and leave them
untouched (torch: ``m.eval()`` on every BatchNorm2d of a train-mode net): no
image's output or gradient depends on the rest of the batch -- fine-tuning a
checkpoint with small batches, saliency / FGSM / PGD on a trained model.  An
eval-mode call records no graph (the BN-folded eval forward has no backward);
``net.train().freeze_bn()`` with no drop-connect / dropout draws installed is
eval-mode arithmetic with a graph.

A HipNet is a light state container (host copy of the flat state).  The heavy
part -- device weights, optimiser moments, activation workspaces -- lives in the
process-wide HIP engine (fedmlp_amd.engine.get_engine); a net is made resident
on it on demand, so the reference's many ``deepcopy(netglob)`` objects cost a
45 MB host copy each, not a GPU workspace each.
"""
from collections import OrderedDict

import numpy as np
import torch

from . import spec
from .engine import get_engine

# the train-mode call's autograd node needs one input that requires grad, and x usually does not (when it does, the node also
# returns d loss / d x)
_ANCHOR = torch.zeros((), requires_grad=True)


class _TrainCall(torch.autograd.Function):
    """One train-mode net(x): the engine's forward now (own BN batch statistics and one running-statistics update, or --
    net.freeze_bn() -- the running statistics, left as they are), its backward into the engine's gradient accumulator when
    the loss is backpropagated.  The node keeps the input, the engine serial after its forward, the net's weights key, its
    BatchNorm mode and (EfficientNet-B0) its drop-connect / dropout draws: if anything was enqueued on the engine since
    (another net(x), an eval forward, a rebind), it re-binds the net, re-installs the mode and the draws and recomputes the
    forward (fm_forward_recompute: bit-identical saved tensors, running statistics untouched), then restores the caller's.
    `xin` is the caller's x on the device, a differentiable argument; `x` its detached copy, what the engine reads (and reads
    again on a recompute).  The input gradient is asked of the engine only when autograd wants it."""

    @staticmethod
    def forward(ctx, anchor, xin, net, eng, x, max_images):
        feat, logits = net._forward_train(eng, x)
        ctx.frozen, ctx.stats_ver = net.bn_frozen, net._stats_ver
        ctx.mask = net._frozen                   # the requires_grad mask the forward ran under: its backward's, whatever the net says by then
        ctx.set_materialize_grads(False)
        ctx.net, ctx.eng, ctx.x, ctx.max_images = net, eng, x, max_images
        ctx.serial, ctx.key = eng.serial, net._weights_key()
        ctx.draws = (getattr(eng, "_dc", None), getattr(eng, "_dr", None)) if eng.model == "Efficient_b0" else None
        return feat, logits

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dfeat, dlogits):
        net = ctx.net
        if net._weights_key() != ctx.key:
            raise RuntimeError("HipNet: the net's weights changed between its train-mode forward and this backward (an "
                               "optimizer step, load_state_dict or FedAvg); run the forward again")
        if ctx.frozen and net._stats_ver != ctx.stats_ver:
            raise RuntimeError("HipNet: a batch-statistics train-mode call moved the BatchNorm running statistics between this "
                               "frozen-BatchNorm forward and its backward; run the forward again")
        eng = net.bind(ctx.x.shape[2], ctx.x.shape[3], ctx.max_images)
        if getattr(eng, "_grad_owner", None) is not net:     # the accumulator holds another net's gradients
            eng.zero_grad()
            eng._grad_owner = net
        if ctx.draws is not None:
            prev = (getattr(eng, "_dc", None), getattr(eng, "_dr", None))
            eng.set_stochastic(*ctx.draws)
        dx = torch.empty_like(ctx.x) if ctx.needs_input_grad[1] else None
        try:
            if eng is not ctx.eng or eng.serial != ctx.serial:
                was = bool(getattr(eng, "bn_frozen", False))
                if was != ctx.frozen:
                    eng.bn_freeze(ctx.frozen)
                net._install_mask(eng, ctx.mask)
                try:
                    eng.forward_recompute(ctx.x)
                finally:
                    if was != ctx.frozen:
                        eng.bn_freeze(was)
                    net._install_mask(eng)
            if dx is None:
                eng.backward_grads(dlogits, dfeat)
            else:
                eng.backward_grads(dlogits, dfeat, dx=dx)
        finally:
            if ctx.draws is not None:
                eng.set_stochastic(*prev)
        return None, dx, None, None, None, None


_MODEL_ALIASES = {"Resnet18": "Resnet18", "resnet18": "Resnet18", "Efficient_b0": "Efficient_b0"}

# file names torchvision 0.13 / efficientnet-pytorch 0.7.1 download for `pretrained=True`
PRETRAINED_FILES = {"Resnet18": "resnet18-f37072fd.pth", "Efficient_b0": "efficientnet-b0-355c32eb.pth"}


class LoadResult(tuple):
    """(missing_keys, unexpected_keys, mismatched_keys) of a load_state_dict call."""
    def __new__(cls, missing, unexpected, mismatched):
        return super().__new__(cls, (list(missing), list(unexpected), list(mismatched)))
    missing_keys = property(lambda self: self[0])
    unexpected_keys = property(lambda self: self[1])
    mismatched_keys = property(lambda self: self[2])


class HipNet:
    def __init__(self, model, n_classes, flat, counters):
        self.model = _MODEL_ALIASES[model]
        self.n_classes = int(n_classes)
        self.flat = np.ascontiguousarray(flat, dtype=np.float32)
        self.counters = np.ascontiguousarray(counters, dtype=np.int64)
        self.training = True
        self._version = 0
        self._wver = 0                 # bumped when an engine step / optimizer changes the weights (mark_trained)
        self._engine = None            # engine on which (self, _version) is resident
        self.default_max_images = 128
        self.precision = "fp32"        # activation storage of the engine this net binds to
        self.bn_frozen = False         # freeze_bn(): train-mode calls apply the BatchNorm running statistics
        self._stats_ver = 0            # bumped by every call that moves the running statistics alone (a batch-statistics net(x))
        self._frozen = frozenset()     # requires_grad_(False, ...): the frozen parameters' keys (empty = the default mask)

    # ---- nn.Module-like surface ----------------------------------------------------------
    def train(self, mode=True):
        self.training = bool(mode)
        return self

    def eval(self):
        return self.train(False)

    def freeze_bn(self, mode=True):
        """Train-mode calls apply every BatchNorm's running statistics and leave them (and num_batches_tracked) as they are,
        forward and backward -- torch's `for m in net.modules(): if isinstance(m, BatchNorm2d): m.eval()`.  Everything else
        stays in train mode (EfficientNet-B0's drop-connect / dropout draws apply as installed).  Eval-mode calls and the fused
        steps (LocalUpdate.train*, Engine.step_*) are not affected."""
        self.bn_frozen = bool(mode)
        return self

    # ---- per-layer requires_grad -------------------------------------------------------------------
    def _param_keys(self):
        """The trainable keys in state_dict order (running statistics and counters are buffers)."""
        return [k for k, _, _ in spec.entries(self.model, self.n_classes) if spec.is_trainable(k)]

    def _resolve(self, names, what):
        """Trainable keys named by `names`: state_dict keys or dotted prefixes ("fc", "layer4", "layer3.1.bn2", "_blocks.15");
        a prefix matches a key equal to it or starting with it + ".".  A name that matches no trainable key raises."""
        keys = self._param_keys()
        if isinstance(names, str):
            names = [names]
        out = []
        for name in names:
            hit = [k for k in keys if k == name or k.startswith(name + ".")]
            if not hit:
                raise ValueError(f"{what}: {name!r} names no trainable parameter of {self.model} (buffers -- running statistics and "
                                 "counters -- are not parameters)")
            out += [k for k in hit if k not in out]
        return out

    def requires_grad_(self, flag=True, names=None):
        """torch's `p.requires_grad_(flag)` for the parameters named by `names` (state_dict keys or dotted prefixes; None =
        every parameter).  A frozen parameter gets no gradient (net.grads() reports exact zeros) and no optimizer touches it;
        the backward stops behind the first layer that has a trainable parameter unless x.grad is wanted.  The mask is read
        by the next train-mode net(x); a pending forward's backward uses the mask it ran under.  BatchNorm running statistics
        of a frozen layer still move in a batch-statistics forward, as in torch: freeze_bn() is the switch for that."""
        hit = self._param_keys() if names is None else self._resolve(names, "requires_grad_")
        self._frozen = frozenset(self._frozen - set(hit) if flag else self._frozen | set(hit))
        return self

    def trainable(self):
        """OrderedDict key -> requires_grad over the trainable keys in state_dict order."""
        return OrderedDict((k, k not in self._frozen) for k in self._param_keys())

    def _entry_flags(self, frozen):
        return [int(spec.is_trainable(k) and k not in frozen) for k, _, _ in spec.entries(self.model, self.n_classes)]

    def _install_mask(self, eng, frozen=None):
        """Make `frozen` (default: this net's mask) the engine's requires_grad mask; an engine that never saw a mask is not
        called while the mask is the default one."""
        want = self._frozen if frozen is None else frozen
        if getattr(eng, "_frozen_keys", frozenset()) != want:
            eng.set_trainable(self._entry_flags(want))
            eng._frozen_keys = want

    def to(self, *a, **k):
        return self

    def cuda(self, *a, **k):
        return self

    def cpu(self):
        return self

    def state_dict(self):
        self._pull()
        sd = spec.flat_to_state_dict(self.model, self.n_classes, self.flat, self.counters)
        return OrderedDict((k, torch.from_numpy(np.asarray(v))) for k, v in sd.items())

    def load_state_dict(self, sd, strict=True):
        """nn.Module.load_state_dict semantics.  strict=False keeps the current value of every
        missing or shape-mismatched entry (so an ImageNet checkpoint with fc [1000, D] loads into a
        C-class net and the classifier keeps its fresh init, like get_model + modify_last_layer,
        model/all_models.py:99-130) and returns (missing, unexpected, mismatched) key lists."""
        keys = [k for k, _, _ in spec.entries(self.model, self.n_classes)]
        if strict:
            if set(keys) != set(sd.keys()):
                missing = sorted(set(keys) - set(sd.keys())); extra = sorted(set(sd.keys()) - set(keys))
                raise RuntimeError(f"load_state_dict: missing {missing[:4]}..., unexpected {extra[:4]}...")
            self.flat, self.counters = spec.state_dict_to_flat(self.model, self.n_classes, sd)
            self._touch()
            return LoadResult([], [], [])
        self._pull()
        self.flat, self.counters, missing, unexpected, mismatched = spec.merge_state_dict(
            self.model, self.n_classes, sd, self.flat, self.counters)
        self._touch()
        return LoadResult(missing, unexpected, mismatched)

    def parameters(self):
        """Trainable tensors in state_dict order (views of the host copy).  They are copies, not the weights the engine
        trains: torch.optim.*(net.parameters()) does not train a HipNet -- use fedmlp_amd.optim.Adam(net)."""
        self._pull()
        off = 0
        for key, shape, dt in spec.entries(self.model, self.n_classes):
            if dt != "f32":
                continue
            n = int(np.prod(shape))
            if spec.is_trainable(key):
                yield torch.from_numpy(self.flat[off:off + n].reshape(shape))
            off += n

    def __deepcopy__(self, memo):
        self._pull()
        c = HipNet(self.model, self.n_classes, self.flat.copy(), self.counters.copy())
        c.training = self.training
        c.default_max_images = self.default_max_images
        c.precision = self.precision
        c.bn_frozen = self.bn_frozen
        c._frozen = self._frozen
        return c

    def __call__(self, x):
        """net(x) on the HIP engine -> (feature[B,D], logits[B,C]) CUDA tensors.
        Eval mode: the eval-mode forward (utils/local_training.py:983, 1030, 1227; utils/evaluations.py:25).
        Train mode: one train-mode forward (its own BN batch statistics and one running-statistics update; after freeze_bn()
        the running statistics, which then stay as they are) whose outputs carry an autograd node: loss.backward() adds the parameter gradients to the engine's accumulator (grads(),
        zero_grad(), fedmlp_amd.optim.Adam) and, when x requires grad, d loss / d x to x.grad (fp32, the stem's data gradient;
        nothing is computed for an x that does not).  Under torch.no_grad() the train forward runs and nothing is recorded.
        An eval-mode call records no graph either way, so x.grad stays None: for eval-mode arithmetic with a graph use
        net.train().freeze_bn() (and install no drop-connect / dropout draws).  The fused steps (LocalUpdate.train*, Engine.step_*) remain the fast path."""
        x = torch.as_tensor(x, dtype=torch.float32)
        max_images = max(self.default_max_images, x.shape[0])
        eng = self.bind(x.shape[2], x.shape[3], max_images)
        x = x.to(eng.device).contiguous()       # differentiable ops: a gradient flows back to the caller's tensor
        if not self.training:
            return eng.forward_eval(x)
        if not torch.is_grad_enabled():
            return self._forward_train(eng, x)
        return _TrainCall.apply(_ANCHOR, x, self, eng, x.detach(), max_images)

    forward = __call__

    def _forward_train(self, eng, x):
        """The engine's train-mode forward in this net's BatchNorm mode: the engine's flag is set before it and handed back as
        the caller left it (the engine remembers the mode of its pending forward, so the backward needs no flag)."""
        was = bool(getattr(eng, "bn_frozen", False))
        if was != self.bn_frozen:
            eng.bn_freeze(self.bn_frozen)
        self._install_mask(eng)
        try:
            out = eng.forward_train(x)
        finally:
            if was != self.bn_frozen:
                eng.bn_freeze(was)
        if not self.bn_frozen:
            self._stats_ver += 1
            self._mark_dirty()             # the running statistics moved
        return out

    # ---- gradients of the train-mode calls (the engine's accumulator) ---------------------------
    def zero_grad(self, set_to_none=True):
        eng = self._engine
        if eng is not None and eng.h and getattr(eng, "_grad_owner", None) is self:
            eng.zero_grad()

    def grads(self):
        """OrderedDict trainable key -> CUDA tensor (state_dict order, conv weights OIHW): the gradients loss.backward()
        accumulated since zero_grad()."""
        eng = self._engine
        if eng is None or not eng.h:
            raise RuntimeError("HipNet.grads(): the net has not run on an engine yet")
        flat = eng.grads() if getattr(eng, "_grad_owner", None) is self else \
            torch.zeros(eng.nf, device=eng.device, dtype=torch.float32)
        out, off = OrderedDict(), 0
        for key, shape, dt in spec.entries(self.model, self.n_classes):
            if dt != "f32":
                continue
            n = int(np.prod(shape))
            if spec.is_trainable(key):
                out[key] = flat[off:off + n].view(tuple(shape))
            off += n
        return out

    def _weights_key(self):
        """Changes whenever the weights do (load_state_dict, an optimizer / engine step): the autograd node's version check."""
        return self._version, self._wver

    def _bound_engine(self):
        """The engine whose resident state is this net's, or None."""
        eng = self._engine
        if eng is not None and eng.h and getattr(eng, "_owner", None) is self \
                and getattr(eng, "_owner_version", -1) == self._version:
            return eng
        return None

    # ---- residency -------------------------------------------------------------------------
    def _touch(self):
        self._version += 1
        self._engine = None

    def bind(self, in_h, in_w, max_images, device=None):
        """Make this net's state the engine's resident state and return the engine
        (device None = this rank's GPU, fedmlp_amd.launch.default_device)."""
        eng = get_engine(self.model, self.n_classes, in_h, in_w, max_images, device, self.precision)
        if getattr(eng, "_owner", None) is not self or getattr(eng, "_owner_version", -1) != self._version \
                or self._engine is not eng:
            prev = getattr(eng, "_owner", None)
            if prev is not None and prev is not self:
                prev._pull()               # do not lose another net's trained, device-only state
            self._pull()
            eng.set_state(self.flat, self.counters)
            eng._owner, eng._owner_version, eng._dirty = self, self._version, False
            self._engine = eng
        self._install_mask(eng)            # the mask belongs to the net, like the state (the fused steps refuse a non-default one)
        return eng

    def _pull(self):
        """Refresh the host copy if the engine trained this net since it was bound."""
        eng = self._engine
        if eng is not None and eng.h and getattr(eng, "_owner", None) is self and getattr(eng, "_dirty", False):
            self.flat, self.counters = eng.get_state()
            eng._dirty = False

    def mark_trained(self):
        """The engine changed this net's weights (a training step, an optimizer step)."""
        self._wver += 1
        self._mark_dirty()

    def _mark_dirty(self):
        """The engine's copy of this net's state moved (a train-mode forward moves the BN running statistics)."""
        if self._engine is not None:
            self._engine._dirty = True


class ResidentNet(HipNet):
    """A net whose state already lives in an engine (one client per GPU: the model never
    leaves HBM between rounds; FedAvg is an in-place RCCL all-reduce of the engine state).
    bind() hands back that engine without any upload; state_dict() still works (D2H copy)."""

    def __init__(self, engine):
        self.model, self.n_classes = engine.model, engine.n_classes
        self.training = True
        self._version = 0
        self._wver = 0
        self._engine = engine
        self.default_max_images = engine.max_images
        self.precision = engine.precision
        self.bn_frozen = False
        self._stats_ver = 0
        self._frozen = frozenset()
        self.resident = True

    def bind(self, in_h, in_w, max_images, device=None):
        eng = self._engine
        assert (in_h, in_w) == (eng.in_h, eng.in_w) and max_images <= eng.max_images, \
            "resident engine was created for another input size / batch"
        self._install_mask(eng)
        return eng

    def _pull(self):
        self.flat, self.counters = self._engine.get_state()

    def mark_trained(self):
        self._wver += 1

    def _mark_dirty(self):
        pass

    def _weights_key(self):
        # the engine is this net's alone: any write of its weights (set_state, FedAvg in place, a step) counts
        return self._wver, self._engine.weights_version

    def _bound_engine(self):
        return self._engine

    def load_state_dict(self, sd, strict=True):
        if strict:
            flat, cnt = spec.state_dict_to_flat(self.model, self.n_classes, sd)
            res = LoadResult([], [], [])
        else:
            f0, c0 = self._engine.get_state()
            flat, cnt, *lists = spec.merge_state_dict(self.model, self.n_classes, sd, f0, c0)
            res = LoadResult(*lists)
        self._engine.set_state(flat, cnt)
        return res

    def __deepcopy__(self, memo):
        return self          # "deepcopy(netglob)" of a resident net is the resident net


def find_pretrained(name, args=None):
    """Where an ImageNet checkpoint for `name` may already sit on this machine: args.pretrained_path,
    $FEDMLP_PRETRAINED_DIR, then torch hub's checkpoint cache (what `pretrained=True` populates in
    the reference, model/all_models.py:53-54, 73-75).  None if nothing is there (no network here)."""
    import os
    cands = []
    p = getattr(args, "pretrained_path", None) if args is not None else None
    if p:
        cands.append(p if not os.path.isdir(p) else os.path.join(p, PRETRAINED_FILES[name]))
    if os.environ.get("FEDMLP_PRETRAINED_DIR"):
        cands.append(os.path.join(os.environ["FEDMLP_PRETRAINED_DIR"], PRETRAINED_FILES[name]))
    hub = os.environ.get("TORCH_HOME", os.path.join(os.path.expanduser("~"), ".cache", "torch"))
    cands.append(os.path.join(hub, "hub", "checkpoints", PRETRAINED_FILES[name]))
    for c in cands:
        if os.path.isfile(c):
            return c
    return None


def build_model(args):
    """model/build_model.py:5-10: get_model(args.model, args.pretrained) + modify_last_layer.
    Reads args.model, args.n_classes, args.pretrained (default 1 in utils/options.py:26),
    optional args.pretrained_path / args.precision.
    pretrained: the ImageNet state_dict is loaded from a local file (find_pretrained) with
    strict=False, so every backbone entry is taken and the 1000-class classifier is dropped in
    favour of a fresh Linear(D, n_classes) -- exactly what modify_last_layer leaves.  Without a
    file (this image has no network) a warning is raised and training starts from the
    deterministic from-scratch init of spec.init_state seeded with args.seed."""
    import warnings
    name = getattr(args, "model", "Resnet18")
    if name not in _MODEL_ALIASES:
        raise ValueError(f"build_model: model {name!r} is not built (available: Resnet18, Efficient_b0)")
    seed = int(getattr(args, "seed", 1037))
    flat, cnt = spec.init_state(_MODEL_ALIASES[name], args.n_classes, seed)
    net = HipNet(name, args.n_classes, flat, cnt)
    net.default_max_images = 4 * int(getattr(args, "batch_size", 32))
    net.precision = getattr(args, "precision", "fp32")
    if int(getattr(args, "pretrained", 0)):
        path = find_pretrained(net.model, args)
        if path is None:
            warnings.warn(
                f"build_model: args.pretrained={args.pretrained} but no ImageNet checkpoint "
                f"({PRETRAINED_FILES[net.model]}) was found (args.pretrained_path, $FEDMLP_PRETRAINED_DIR, "
                "torch hub cache) and this machine cannot download one: training starts from the "
                "from-scratch init. Pass --pretrained 0 to silence this.", RuntimeWarning, stacklevel=2)
        else:
            import torch as _t
            sd = _t.load(path, map_location="cpu")
            res = net.load_state_dict(sd, strict=False)
            # torchvision's / efficientnet-pytorch's published ImageNet files carry no `num_batches_tracked` entries: torch's
            # BatchNorm leaves a missing counter at 0 (the reference loads such files), and so does merge_state_dict
            bad = [k for k in res.missing_keys + res.mismatched_keys
                   if k not in spec.classifier_keys(net.model) and not k.endswith(".num_batches_tracked")]
            if bad:
                raise RuntimeError(f"build_model: {path} does not match {net.model}: {bad[:6]}")
    return net
