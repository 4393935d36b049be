"""Client-drift correction for the federated trainers: FedProx and SCAFFOLD on the engine's optimizer steps.

The engine offers one mechanism (include/fedmlp_hip_drift.h): while a correction is installed, one launch in front of every
optimizer step -- the fused ``step_*`` as well as the autograd path's ``adam_step`` / ``adamw_step`` / ``sgd_step`` and the grouped
steps -- writes a corrected copy of the gradient and the optimizer reads that copy::

    r = g  [+ mu * (p - anchor)]  [+ shift]          S += g   (track)

in fp32, every operation rounded on its own.  The raw gradient ``g`` is never written.  This module holds the ctypes wrappers
(functions that take the engine: ``Engine``'s own method list is closed) and the two methods built on them.

FedProx(mu)
    ``begin(engine)`` anchors the proximal term mu/2 |w - w_glob|^2 at the model the engine holds -- the global model the
    driver has just loaded -- and ``end(engine)`` uninstalls it.

Scaffold(n_params, n_clients, device)
    Control variates as flat device tensors in ``net.grads()`` layout: ``c_global`` and one ``c_local[i]`` per client this rank
    trains.  ``begin(engine, i)`` installs the shift c_global - c_local[i] and has the engine sum the raw gradients;
    ``end(engine, i)`` takes their mean over the round's K steps as the new c_local[i] and returns the change.
    ``server_update(deltas)`` adds sum(deltas) / n_clients to c_global (summed over the ranks).

    The new control variate is DEFINED as the mean of the raw minibatch gradients of the round.  For plain SGD with step eta
    this equals the paper's option II, c_i - c + (x - y_i) / (K eta): the K updates sum to x - y_i = eta sum_k (g_k + c - c_i).
    Unlike option II it keeps its meaning under Adam, which every fused step uses and whose updates are not proportional to
    the gradient.  The global step size is 1: the models are aggregated by the driver's FedAvg, with its sample-count weights
    (the paper averages uniformly).

Deviations shared by both: the correction is added at the optimizer step, after any clipping of the
accumulator; the loss a step reports is the data loss, without the proximal term; with gradient accumulation on the autograd
path the correction is applied once per ``step()``, to the accumulated gradient.
"""
import ctypes as C

import torch

from . import _lib


# ---- the four entry points, as plain work on the engine's stream (none of them moves the weights) ------------------------
def _flat(engine, t, what):
    if t.dtype != torch.float32 or not t.is_cuda or not t.is_contiguous() or t.numel() != engine.nf:
        raise ValueError(f"{what}: a contiguous float32 device tensor of {engine.nf} elements (net.grads() layout) is needed")
    return C.c_void_p(t.data_ptr())


def drift_begin(engine, mu=0.0, shift=None, track=False):
    """Install a correction (fm_drift_begin): the anchor is the model the engine holds now.  shift: None or a flat device
    tensor in grads() layout (copied by the call); track: keep the running sum of raw gradients for drift_end."""
    engine._check_stream()
    engine._enqueue()
    _lib.check(engine.lib.fm_drift_begin(engine.h, C.c_float(mu), None if shift is None else _flat(engine, shift, "drift_begin"),
                                         int(bool(track))))


def drift_last(engine):
    """The corrected gradient the most recent optimizer step read, in grads() layout; enqueued, not synchronised."""
    engine._check_stream()
    engine._enqueue()
    out = torch.empty(engine.nf, device=engine.device, dtype=torch.float32)
    _lib.check(engine.lib.fm_drift_last(engine.h, C.c_void_p(out.data_ptr())))
    return out


def drift_end(engine, mean=True):
    """Uninstall (fm_drift_end) -> (mean raw gradient of the steps since drift_begin in grads() layout -- zeros without track
    or without a step; None with mean=False --, the number of steps)."""
    engine._check_stream()
    engine._enqueue()
    out = torch.empty(engine.nf, device=engine.device, dtype=torch.float32) if mean else None
    steps = C.c_int64()
    _lib.check(engine.lib.fm_drift_end(engine.h, None if out is None else C.c_void_p(out.data_ptr()), C.byref(steps)))
    return out, steps.value


def drift_active(engine):
    return bool(engine.lib.fm_drift_active(engine.h))


# ---- FedProx ------------------------------------------------------------------------------------------------------------
class FedProx:
    """Li et al., Federated Optimization in Heterogeneous Networks: local steps on loss + mu/2 |w - w_glob|^2"""

    def __init__(self, mu):
        mu = float(mu)
        if not (mu > 0.0 and mu != float("inf")):
            raise ValueError("FedProx: mu must be positive and finite")
        self.mu = mu

    def begin(self, engine):
        drift_begin(engine, mu=self.mu)

    def end(self, engine):
        drift_end(engine, mean=False)


# ---- SCAFFOLD -----------------------------------------------------------------------------------------------------------
def _rank_sum_(t):
    """t <- its sum over the ranks (torch.distributed, when a job of more than one rank is up), as tao_allreduce forms its sums"""
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        dist.all_reduce(t, op=dist.ReduceOp.SUM)
    return t


class Scaffold:
    """Karimireddy et al., SCAFFOLD: Stochastic Controlled Averaging for Federated Learning; see the module docstring for the
    definition of the new control variate and for what is left to the driver."""

    def __init__(self, n_params, n_clients, device):
        self.n_params, self.n_clients, self.device = int(n_params), int(n_clients), torch.device(device)
        self.c_global = torch.zeros(self.n_params, device=self.device)
        self.c_local = {}                 # client -> its control variate, created (zero) at the client's first round
        self.deltas = []                  # what end() returned since the last server_update()

    def _local(self, i):
        if i not in self.c_local:
            self.c_local[i] = torch.zeros(self.n_params, device=self.device)
        return self.c_local[i]

    def begin(self, engine, i):
        drift_begin(engine, mu=0.0, shift=self.c_global - self._local(i), track=True)

    def end(self, engine, i):
        """c_local[i] <- mean raw gradient of the round; returns (and notes) delta c_i = new - old"""
        new, _ = drift_end(engine)
        delta = new - self._local(i)
        self.c_local[i] = new
        self.deltas.append(delta)
        return delta

    def server_update(self, deltas=None):
        """c_global += sum_i delta c_i / n_clients, the sum running over this rank's deltas (default: those noted since the
        last call) and then over the ranks.  -> c_global"""
        if deltas is None:
            deltas = self.deltas
        total = torch.zeros_like(self.c_global)
        for d in deltas:
            total += d
        self.deltas = []
        self.c_global += _rank_sum_(total) / self.n_clients
        return self.c_global

    def client(self, i):
        """begin(engine) / end(engine) for client i: what LocalUpdate.drift holds"""
        return _ScaffoldClient(self, i)


class _ScaffoldClient:
    def __init__(self, scaffold, i):
        self.scaffold, self.i = scaffold, i

    def begin(self, engine):
        self.scaffold.begin(engine, self.i)

    def end(self, engine):
        return self.scaffold.end(engine, self.i)
