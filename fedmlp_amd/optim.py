"""torch.optim.Adam / AdamW / SGD and gradient clipping for a HipNet / ResidentNet (utils/local_training.py builds a fresh
torch.optim.Adam every round).

The weights, the optimizer's moments and the step count live in the HIP engine the net is bound to, and the gradients are the
engine's accumulator that loss.backward() through a train-mode ``net(x)`` fills (model.HipNet).  So an optimizer takes
the net, not ``net.parameters()``:

    opt = Adam(net, lr=args.base_lr, betas=(0.9, 0.999), weight_decay=5e-4)
    net.train(); feat, logits = net(x); loss = head(feat, logits)
    opt.zero_grad(); loss.backward(); clip_grad_norm_(net, 1.0); opt.step()

Arithmetic: torch's single-tensor updates -- Adam with coupled L2 weight decay (fm_adam_step), AdamW with decoupled decay
(fm_adamw_step), SGD with momentum / dampening / Nesterov (fm_sgd_step); clip_grad_norm_ / clip_grad_value_ as in
torch.nn.utils (fm_clip_grad_norm, fm_clip_grad_value).  One engine holds ONE optimizer's state: a second optimizer on the same
net resets it at its first step.  state_dict() / load_state_dict() move the moments as flat CUDA tensors in ``net.grads()``
layout (state_dict order, conv weights OIHW, zeros at the BatchNorm running statistics).

Parameter groups and frozen layers (fine-tuning a pretrained backbone):

    net.requires_grad_(False).requires_grad_(True, ["layer4", "fc"])
    opt = AdamW(net, lr=1e-3, groups=[{"params": ["fc"]}, {"params": ["layer4"], "lr": 1e-4}])

``groups`` is a list of at most 8 dicts ``{"params": [state_dict keys or dotted prefixes], <overrides of the defaults>}``; a
parameter named by two groups raises, one named by none is not optimized (both as in torch).  ``param_groups[i]`` is the merged
dict with "params" resolved to the key list, read on every step.  A frozen parameter (``net.requires_grad_(False, ...)``) is
skipped by every optimizer -- no update, no weight decay, moments untouched: torch's ``grad is None`` rule -- and its slots of
the gradient accumulator are exact zeros, so the clips' norm is the norm over the trainable parameters.  With ``groups=None``
and no frozen parameter the engine calls are the single-group ones (fm_adam_step / fm_adamw_step / fm_sgd_step); otherwise one
grouped launch (fm_*_step_groups), under a mask with ``groups=None`` over one group of the trainable parameters.

Deviations from torch: the step count stays ONE per engine, not per parameter (a parameter that joins later -- unfrozen, or
a momentum buffer torch would create at its first gradient -- takes the bias corrections / the later-step SGD form of the
engine's count); ``requires_grad=False`` does not stop a batch-statistics BatchNorm from updating its running statistics
(torch's behaviour too): ``net.freeze_bn()`` is the switch for that.
"""
import torch


class _EngineOptimizer:
    """What every optimizer here does around the engine: the bound-engine check, the reset on first use or when the net is
    bound to another engine, the gradient-owner check, ``param_groups`` read on every step, ``mark_trained``; parameter groups and the
    frozen-parameter rule (the module docstring)."""

    _state_keys = ("exp_avg", "exp_avg_sq")

    MAX_GROUPS = 8                   # FM_MAX_GROUPS

    def __init__(self, net, defaults, groups=None):
        self.net = net
        self.defaults = defaults
        # read on every step, so a caller may change lr between steps (param_groups[0]["lr"] = ...)
        if groups is None:
            self.param_groups = [dict(self.defaults)]
        else:
            self.param_groups = self._make_groups(groups)
        self._grouped = groups is not None
        # a fresh torch optimizer: zero moments and step count.  The moments belong to the engine; a net that is not bound
        # yet gets them reset at its first step
        self._engine = None
        self._pending_state = None
        eng = net._bound_engine()
        if eng is not None:
            self._reset(eng)

    def _make_groups(self, groups):
        name = type(self).__name__
        groups = list(groups)
        if not 1 <= len(groups) <= self.MAX_GROUPS:
            raise ValueError(f"{name}: 1 to {self.MAX_GROUPS} parameter groups are supported, got {len(groups)}")
        out, seen = [], set()
        for i, g in enumerate(groups):
            if not isinstance(g, dict) or "params" not in g:
                raise ValueError(f"{name}: parameter group {i} must be a dict with a 'params' list of keys or prefixes")
            unknown = set(g) - set(self.defaults) - {"params"}
            if unknown:
                raise ValueError(f"{name}: parameter group {i} has unknown options {sorted(unknown)}")
            keys = self.net._resolve(g["params"], f"{name} parameter group {i}")
            twice = [k for k in keys if k in seen]
            if twice:
                raise ValueError(f"{name}: some parameters appear in more than one parameter group: {twice[:4]}")
            seen.update(keys)
            merged = dict(self.defaults)
            merged.update({k: v for k, v in g.items() if k != "params"})
            if "betas" in merged:
                merged["betas"] = tuple(merged["betas"])
            merged["params"] = keys
            self._check(merged)
            out.append(merged)
        return out

    def _group_of_entry(self):
        """(group of every state_dict entry: -1 = not optimized, group count).  groups=None under a mask: one group whose
        members are the trainable parameters."""
        from . import spec
        keys = [k for k, _, _ in spec.entries(self.net.model, self.net.n_classes)]
        if not self._grouped:
            frozen = self.net._frozen
            return tuple(0 if spec.is_trainable(k) and k not in frozen else -1 for k in keys), 1
        of = {k: i for i, g in enumerate(self.param_groups) for k in g["params"]}
        return tuple(of.get(k, -1) for k in keys), len(self.param_groups)

    def _reset(self, eng):
        self._engine_reset(eng, self.param_groups[0])
        self._engine = eng

    def _bound(self, what):
        name = type(self).__name__
        eng = self.net._bound_engine()
        if eng is None:
            raise RuntimeError(f"{name}.{what}: the engine does not hold this optimizer's net (another net was bound to it since "
                               f"the backward, or the net never ran); the {name} moments belong to the engine")
        if self._engine is not eng:
            self._reset(eng)
        if self._pending_state is not None:
            step, tensors = self._pending_state
            self._pending_state = None
            eng.set_optim_state(step, *tensors)
        return eng

    def zero_grad(self, set_to_none=True):
        self.net.zero_grad()

    def step(self):
        eng = self._bound("step")
        if getattr(eng, "_grad_owner", None) is not self.net:
            return                      # no gradients: torch skips parameters whose .grad is None
        self.net._install_mask(eng)       # a frozen parameter is skipped: the grouped steps read the engine's mask
        if not self._grouped and not self.net._frozen:
            self._engine_step(eng, self.param_groups[0])
        else:
            table = self._group_of_entry()
            if getattr(eng, "_groups_key", None) != table:
                eng.optim_groups(*table)
                eng._groups_key = table
            for g in self.param_groups:
                self._check(g)
            self._engine_step_groups(eng, self.param_groups)
        self.net.mark_trained()

    def state_dict(self):
        """{"state": {"step", <moments>}, "param_groups": [...]}: the moments as flat CUDA tensors in net.grads() layout."""
        if self._pending_state is not None:
            step, tensors = self._pending_state
        else:
            step, m, v = self._bound("state_dict").optim_state()
            tensors = (m, v)[:len(self._state_keys)]
        state = {"step": int(step)}
        state.update(zip(self._state_keys, tensors))
        return {"state": state, "param_groups": [dict(g) for g in self.param_groups]}

    def load_state_dict(self, sd):
        state = sd["state"]
        missing = [k for k in ("step",) + self._state_keys if k not in state]
        if missing:
            raise ValueError(f"{type(self).__name__}.load_state_dict: the state lacks {missing}")
        from . import spec
        nf = spec.sizes(self.net.model, self.net.n_classes)[0]
        tensors = []
        for k in self._state_keys:
            t = torch.as_tensor(state[k], dtype=torch.float32).reshape(-1)
            if t.numel() != nf:
                raise ValueError(f"{type(self).__name__}.load_state_dict: {k} has {t.numel()} elements, the net's layout has {nf}")
            tensors.append(t.clone())
        groups = sd.get("param_groups")
        if groups:
            if len(groups) != len(self.param_groups):
                raise ValueError(f"{type(self).__name__}.load_state_dict: the state has {len(groups)} parameter groups, this "
                                 f"optimizer has {len(self.param_groups)}")
            for i, (g, mine) in enumerate(zip(groups, self.param_groups)):
                if list(g.get("params", ())) != list(mine.get("params", ())):
                    raise ValueError(f"{type(self).__name__}.load_state_dict: parameter group {i} names other parameters than "
                                     "this optimizer's")
            self.param_groups = [dict(g) for g in groups]
        # installed when the engine holds the net (now, or at the next step)
        self._pending_state = (int(state["step"]), tuple(tensors))
        if self.net._bound_engine() is not None:
            self._bound("load_state_dict")


class Adam(_EngineOptimizer):
    def __init__(self, net, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, groups=None):
        defaults = {"lr": lr, "betas": tuple(betas), "eps": eps, "weight_decay": weight_decay}
        self._check(defaults)
        _EngineOptimizer.__init__(self, net, defaults, groups)

    def _check(self, g):
        lr, betas, eps, wd = g["lr"], g["betas"], g["eps"], g["weight_decay"]
        if lr < 0.0 or eps < 0.0 or wd < 0.0 or not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError(f"{type(self).__name__}: invalid hyper-parameters lr={lr} betas={betas} eps={eps} weight_decay={wd}")

    def _engine_reset(self, eng, g):
        eng.adam_reset(g["lr"], g["betas"], g["eps"], g["weight_decay"])

    def _engine_step(self, eng, g):
        eng.adam_step(g["lr"], g["betas"], g["eps"], g["weight_decay"])

    def _engine_step_groups(self, eng, groups):
        eng.adam_step_groups([(g["lr"], g["betas"], g["eps"], g["weight_decay"]) for g in groups])


class AdamW(Adam):
    """torch.optim.AdamW: p *= 1 - lr * weight_decay, then Adam's update with no L2 term in the gradient."""

    def __init__(self, net, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, groups=None):
        Adam.__init__(self, net, lr, betas, eps, weight_decay, groups)

    def _engine_step(self, eng, g):
        eng.adamw_step(g["lr"], g["betas"], g["eps"], g["weight_decay"])

    def _engine_step_groups(self, eng, groups):
        eng.adamw_step_groups([(g["lr"], g["betas"], g["eps"], g["weight_decay"]) for g in groups])


class SGD(_EngineOptimizer):
    """torch.optim.SGD; the momentum buffer is the engine's first moment arena (momentum 0 does not touch it)."""

    _state_keys = ("momentum_buffer",)

    def __init__(self, net, lr, momentum=0, dampening=0, weight_decay=0, nesterov=False, groups=None):
        defaults = {"lr": lr, "momentum": momentum, "dampening": dampening, "weight_decay": weight_decay, "nesterov": bool(nesterov)}
        self._check(defaults)
        super().__init__(net, defaults, groups)

    def _check(self, g):
        lr, momentum, weight_decay = g["lr"], g["momentum"], g["weight_decay"]
        if lr < 0.0 or momentum < 0.0 or weight_decay < 0.0:
            raise ValueError(f"SGD: invalid hyper-parameters lr={lr} momentum={momentum} weight_decay={weight_decay}")
        if g["nesterov"] and (momentum <= 0 or g["dampening"] != 0):
            raise ValueError("SGD: Nesterov momentum requires a momentum and zero dampening")

    def _engine_reset(self, eng, g):
        eng.sgd_reset(g["lr"], g["momentum"], g["dampening"], g["weight_decay"], g["nesterov"])

    def _engine_step(self, eng, g):
        eng.sgd_step(g["lr"], g["momentum"], g["dampening"], g["weight_decay"], g["nesterov"])

    def _engine_step_groups(self, eng, groups):
        eng.sgd_step_groups([(g["lr"], g["momentum"], g["dampening"], g["weight_decay"], g["nesterov"]) for g in groups])


def _grad_engine(net):
    """The engine whose accumulator holds this net's gradients, or None."""
    eng = net._bound_engine()
    return eng if eng is not None and getattr(eng, "_grad_owner", None) is net else None


def clip_grad_norm_(net, max_norm, norm_type=2.0):
    """torch.nn.utils.clip_grad_norm_ over the net's accumulated gradients: scaled in place by min(1, max_norm / (norm + 1e-6)).
    Returns the total norm before clipping as a 0-dim tensor (zero when the net has no gradients).  Only the L2 norm."""
    if float(norm_type) != 2.0:
        raise ValueError(f"clip_grad_norm_: only norm_type=2 is supported, got {norm_type}")
    if not float(max_norm) >= 0.0:
        raise ValueError(f"clip_grad_norm_: max_norm must be >= 0, got {max_norm}")
    eng = _grad_engine(net)
    if eng is None:
        return torch.zeros(())
    return eng.clip_grad_norm(float(max_norm))


def clip_grad_value_(net, clip_value):
    """torch.nn.utils.clip_grad_value_: the net's accumulated gradients clamped in place to [-clip_value, clip_value]."""
    if not float(clip_value) >= 0.0:
        raise ValueError(f"clip_grad_value_: clip_value must be >= 0, got {clip_value}")
    eng = _grad_engine(net)
    if eng is not None:
        eng.clip_grad_value(float(clip_value))
