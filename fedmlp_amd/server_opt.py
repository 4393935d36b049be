"""Server optimizers: FedAvgM, FedAdagrad, FedAdam and FedYogi (Reddi et al., Adaptive Federated Optimization, ICLR 2021) on the
global model.

A round's aggregation leaves the weighted mean ``a`` of the client models in the engine.  With ``x`` the global model the round
started from, ``d = a - x`` is a pseudo-gradient and the server takes a momentum or adaptive step from ``x``::

    m  : AVGM     m = beta1*m + d
         others   m = beta1*m + (1 - beta1)*d
    v  : ADAGRAD  v = v + d*d
         ADAM     v = beta2*v + (1 - beta2)*d*d
         YOGI     v = v - (1 - beta2)*d*d*sign(v - d*d)
    x' : AVGM     x' = x + lr*m
         others   x' = x + lr*m / (sqrt(v) + tau)

in fp32, every operation rounded on its own, no bias correction (include/fedmlp_hip_server.h has the order of the operations).
``m`` starts at zero, ``v`` at ``tau*tau``.  Only parameters are stepped: the BatchNorm running statistics and the
``num_batches_tracked`` counters stay the aggregate's plain averages.

This module holds the ctypes wrappers of the engine's one launch (functions that take the engine: ``Engine``'s own method list is
closed), the four classes built on them, and ``apply``, a host drop-in beside ``fedavg.FedAvg`` for callers that aggregate
``state_dict``s on the CPU as the reference does.  On fp32 entries ``apply`` and the kernel give the same bits.
"""
import ctypes as C
import math
from collections import OrderedDict

import torch

from . import _lib, spec

RULES = ("avgm", "adagrad", "adam", "yogi")           # fm_server_opt.rule = the index


# ---- the entry points, on the engine's stream ------------------------------------------------------------------------------
def _flat(engine, t, what):
    if not torch.is_tensor(t) or t.dtype != torch.float32 or not t.is_cuda or not t.is_contiguous() or t.numel() != engine.nf:
        raise ValueError(f"{what}: a contiguous float32 device tensor of {engine.nf} elements (net.grads() layout) is needed")
    return C.c_void_p(t.data_ptr())


def server_begin(engine, rule, lr, beta1=0.0, beta2=0.0, tau=0.0):
    """Install a server optimizer (fm_server_opt_begin): m = 0, v = tau^2, step count 0.  rule: a name of RULES or its index."""
    engine._check_stream()
    engine._enqueue()
    hp = _lib.FmServerOpt(RULES.index(rule) if isinstance(rule, str) else int(rule), lr, beta1, beta2, tau)
    _lib.check(engine.lib.fm_server_opt_begin(engine.h, C.byref(hp)))


def server_step(engine, old_global, norm=True):
    """One server step (fm_server_opt_step): the engine's state, which holds the aggregate, becomes x'.  old_global: the model
    the round started from, a device tensor of state_tensor()'s layout (not the engine's own).  -> |aggregate - old_global|_2
    over the parameters as a 0-dim float64 device tensor (None with norm=False); enqueued, not synchronised."""
    engine._check_stream()
    ns = getattr(engine, "_ns", None)
    if ns is None:
        ns = engine._ns = engine.state_tensor().numel()
    if (not torch.is_tensor(old_global) or old_global.dtype != torch.float32 or not old_global.is_cuda
            or not old_global.is_contiguous() or old_global.numel() != ns):
        raise ValueError(f"server_step: old_global must be a contiguous float32 device tensor of {ns} elements (state_tensor() layout)")
    out = torch.empty((), device=engine.device, dtype=torch.float64) if norm else None
    engine._enqueue(weights=True)
    _lib.check(engine.lib.fm_server_opt_step(engine.h, C.c_void_p(old_global.data_ptr()),
                                             None if out is None else C.c_void_p(out.data_ptr())))
    return out


def server_get_state(engine):
    """(steps, m, v): the step count and the two moments as flat device tensors in net.grads() layout (v zeros under AVGM)"""
    engine._check_stream()
    engine._enqueue()
    m = torch.empty(engine.nf, device=engine.device, dtype=torch.float32)
    v = torch.empty(engine.nf, device=engine.device, dtype=torch.float32)
    steps = C.c_int64()
    _lib.check(engine.lib.fm_server_opt_get_state(engine.h, C.c_void_p(m.data_ptr()), C.c_void_p(v.data_ptr()), C.byref(steps)))
    return steps.value, m, v


def server_set_state(engine, steps, m, v=None):
    """The inverse of server_get_state (fm_server_opt_set_state); v None: AVGM only."""
    engine._check_stream()
    engine._enqueue()
    _lib.check(engine.lib.fm_server_opt_set_state(engine.h, _flat(engine, m, "server_set_state"),
                                                  None if v is None else _flat(engine, v, "server_set_state"), int(steps)))


def server_end(engine):
    engine._check_stream()
    engine._enqueue()
    _lib.check(engine.lib.fm_server_opt_end(engine.h))


def server_active(engine):
    return bool(engine.lib.fm_server_opt_active(engine.h))


# ---- the four methods -----------------------------------------------------------------------------------------------------
def _f32(x):
    return torch.tensor(float(x), dtype=torch.float32)


class ServerOptimizer:
    """Common part of the four classes.  The object owns the optimizer's state -- the step count and the two moments -- wherever it
    lives: in the engine between begin() and end() (the device path), on the host between calls of apply() (the host path), or
    as the flat tensors load_state_dict() was given until one of the two paths takes them."""
    rule = None
    adaptive = True
    second = True                      # reads beta2

    def __init__(self, lr, beta1, beta2, tau):
        self._set_hyper(lr, beta1, beta2, tau)
        self.steps = 0
        self.last_norm = None          # what the most recent step() returned
        self._engine = None            # the engine that holds the state (begin .. end)
        self._flat = None              # (m, v) flat, net.grads() layout: loaded or taken back from an engine, not yet installed
        self._host = None              # the host path's moments: [(key, shape, [m, v] or None for a buffer)] in state_dict order

    def _set_hyper(self, lr, beta1, beta2, tau):
        """the four hyper-parameters, checked as fm_server_opt_begin checks them (the constructor and load_state_dict)"""
        lr, beta1, beta2, tau = float(lr), float(beta1), float(beta2), float(tau)
        name = type(self).__name__
        if not (lr >= 0.0 and math.isfinite(lr)):
            raise ValueError(f"{name}: lr must be finite and >= 0")
        if not 0.0 <= beta1 < 1.0:
            raise ValueError(f"{name}: beta1 must lie in [0, 1)")
        if self.second and not 0.0 <= beta2 < 1.0:
            raise ValueError(f"{name}: beta2 must lie in [0, 1)")
        if self.adaptive and not (tau > 0.0 and math.isfinite(tau)):
            raise ValueError(f"{name}: tau must be finite and > 0")
        self.lr, self.beta1, self.beta2, self.tau = lr, beta1, beta2, tau

    # -- device path
    def begin(self, engine):
        server_begin(engine, self.rule, self.lr, self.beta1, self.beta2, self.tau)
        self._engine = engine
        flat = self._take_flat()
        if flat is not None:
            m, v = (t.to(engine.device) for t in flat)
            server_set_state(engine, self.steps, m, v if self.adaptive else None)

    def step(self, engine, old_global):
        """-> |aggregate - old_global|_2 as a 0-dim device tensor, not synchronised"""
        self.last_norm = server_step(engine, old_global)
        self.steps += 1
        return self.last_norm

    def end(self, engine):
        """uninstall; the state comes back to the object (state_dict() keeps working, a later begin() resumes)"""
        self.steps, m, v = server_get_state(engine)
        self._flat = (m, v)
        server_end(engine)
        self._engine = None

    # -- state
    def hyper(self):
        return {"rule": self.rule, "lr": self.lr, "beta1": self.beta1, "beta2": self.beta2, "tau": self.tau}

    def _take_flat(self):
        """the state outside an engine as flat tensors, which the caller now owns (None: a fresh optimizer)"""
        if self._host is not None:
            ms, vs = [], []
            for key, shape, mv in self._host:
                z = torch.zeros(int(torch.Size(shape).numel()))
                ms.append(z if mv is None else mv[0].reshape(-1))
                vs.append(z if mv is None or mv[1] is None else mv[1].reshape(-1))
            self._flat, self._host = (torch.cat(ms), torch.cat(vs)), None
        flat, self._flat = self._flat, None
        return flat

    def state_dict(self):
        """{"hyper": {...}, "step", "m", "v"}: the moments as flat tensors in net.grads() layout (None before the first state)"""
        if self._engine is not None:
            self.steps, m, v = server_get_state(self._engine)
        else:
            flat = self._take_flat()
            self._flat = flat
            m, v = flat if flat is not None else (None, None)
        return {"hyper": self.hyper(), "step": int(self.steps), "m": m, "v": v}

    def load_state_dict(self, sd):
        """The state's hyper-parameters replace this object's (the file wins, as torch's optimizers have it) after the
        constructor's checks; nothing is changed when they, the rule or the moments' sizes are refused."""
        name = type(self).__name__
        hyper = sd["hyper"]
        if hyper["rule"] != self.rule:
            raise ValueError(f"{name}.load_state_dict: the state is a {hyper['rule']!r} optimizer's, this one is {self.rule!r}")
        if sd["m"] is not None and sd["v"] is not None and torch.as_tensor(sd["m"]).numel() != torch.as_tensor(sd["v"]).numel():
            raise ValueError(f"{name}.load_state_dict: m and v differ in size")
        if int(sd["step"]) < 0:
            raise ValueError(f"{name}.load_state_dict: step must be >= 0")
        self._set_hyper(*(hyper[k] for k in ("lr", "beta1", "beta2", "tau")))
        self.steps = int(sd["step"])
        self._host = None
        if sd["m"] is None:
            self._flat = None
        else:
            m = torch.as_tensor(sd["m"], dtype=torch.float32).reshape(-1).clone()
            v = torch.zeros_like(m) if sd["v"] is None else torch.as_tensor(sd["v"], dtype=torch.float32).reshape(-1).clone()
            self._flat = (m, v)
        if self._engine is not None and self._flat is not None:
            eng = self._engine
            m, v = (t.to(eng.device) for t in self._take_flat())
            server_set_state(eng, self.steps, m, v if self.adaptive else None)

    # -- the rule on the host: torch CPU fp32, one rounded operation per line (include/fedmlp_hip_server.h)
    def _rule(self, x, a, m, v):
        lr, b1 = _f32(self.lr), _f32(self.beta1)
        d = a - x
        if self.rule == "avgm":
            t = b1 * m
            m = t + d
            t = lr * m
            return x + t, m, None
        omb1 = _f32(1.0) - b1
        t = b1 * m
        u = omb1 * d
        m = t + u
        q = d * d
        if self.rule == "adagrad":
            v = v + q
        else:
            b2 = _f32(self.beta2)
            omb2 = _f32(1.0) - b2
            if self.rule == "adam":
                t = b2 * v
                u = omb2 * q
                v = t + u
            else:
                s = torch.sign(v - q)
                u = omb2 * q
                u = u * s
                v = v - u
        r = torch.sqrt(v)
        r = r + _f32(self.tau)
        t = lr * m
        t = t / r
        return x + t, m, v


class FedAvgM(ServerOptimizer):
    """server momentum (Hsu et al. 2019): m = momentum*m + d, x' = x + lr*m"""
    rule, adaptive, second = "avgm", False, False

    def __init__(self, lr=1.0, momentum=0.9):
        super().__init__(lr, momentum, 0.0, 0.0)


class FedAdagrad(ServerOptimizer):
    rule, second = "adagrad", False

    def __init__(self, lr=1e-2, beta1=0.9, tau=1e-3):
        super().__init__(lr, beta1, 0.0, tau)


class FedAdam(ServerOptimizer):
    rule = "adam"

    def __init__(self, lr=1e-2, beta1=0.9, beta2=0.99, tau=1e-3):
        super().__init__(lr, beta1, beta2, tau)


class FedYogi(FedAdam):
    rule = "yogi"


CLASSES = {"avgm": FedAvgM, "adagrad": FedAdagrad, "adam": FedAdam, "yogi": FedYogi}


def make(rule, lr=None, beta1=None, beta2=None, tau=None):
    """the class of `rule` with the given hyper-parameters; None: the class's own default"""
    kw = {"lr": lr, "beta1": beta1, "beta2": beta2, "tau": tau}
    if rule == "avgm":
        kw = {"lr": lr, "momentum": beta1}
    elif rule == "adagrad":
        kw.pop("beta2")
    return CLASSES[rule](**{k: v for k, v in kw.items() if v is not None})


def _trainable(key, t):
    return torch.is_tensor(t) and t.is_floating_point() and spec.is_trainable(key)


def apply(opt, w_glob_old, w_avg):
    """The host drop-in: the new global state_dict from the round's starting one and the clients' average (fedavg.FedAvg's
    output).  Parameters take one step of `opt`'s rule in torch CPU fp32; buffers and counters take w_avg's values.  The moments
    live in `opt` (state_dict() / load_state_dict() carry them in net.grads() layout)."""
    if opt._engine is not None:
        raise RuntimeError("server_opt.apply: the optimizer's state lives in an engine (end() first)")
    prev = opt._host
    flat = opt._take_flat() if prev is None else None
    host, off = [], 0
    if flat is not None:                                   # a loaded state: cut in w_avg's key order
        total = sum(t.numel() for t in w_avg.values() if torch.is_tensor(t) and t.is_floating_point())
        if flat[0].numel() != total:
            raise ValueError(f"server_opt.apply: the loaded state has {flat[0].numel()} elements, the state_dict has {total}")
    out = OrderedDict()
    for key, a in w_avg.items():
        if not (torch.is_tensor(a) and a.is_floating_point()):
            out[key] = a.clone() if torch.is_tensor(a) else a
            continue
        n = a.numel()
        if not _trainable(key, a):
            out[key] = a.clone()
            host.append((key, tuple(a.shape), None))
            off += n
            continue
        a32 = a.detach().to("cpu", torch.float32)
        x32 = w_glob_old[key].detach().to("cpu", torch.float32)
        if flat is not None:
            m = flat[0][off:off + n].reshape(a.shape).cpu()
            v = flat[1][off:off + n].reshape(a.shape).cpu() if opt.adaptive else None
        elif prev is not None:
            m, v = prev[len(host)][2]
        else:
            m = torch.zeros_like(a32)
            v = (_f32(opt.tau) * _f32(opt.tau)).expand(a.shape).clone() if opt.adaptive else None
        x1, m, v = opt._rule(x32, a32, m, v)
        out[key] = x1.to(a.dtype)
        host.append((key, tuple(a.shape), [m, v]))
        off += n
    opt._host = host
    opt.steps += 1
    return out
