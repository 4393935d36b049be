"""Bookkeeping of the train-mode net(x) autograd node (fedmlp_amd.model._TrainCall), driven without a GPU: a fake engine
records what the node asks of it.  The arithmetic behind those calls is tests/test_autograd_gpu.py's."""
import numpy as np
import pytest
import torch

from fedmlp_amd import model as M
from fedmlp_amd import spec
from fedmlp_amd.optim import Adam

C_, HW = 5, 64


class FakeEngine:
    """The Engine surface the node, HipNet and optim.Adam use; every call is logged, serial / weights_version as Engine."""

    def __init__(self, model="Resnet18"):
        self.model, self.n_classes, self.in_h, self.in_w = model, C_, HW, HW
        self.max_images, self.precision, self.device, self.h = 16, "fp32", torch.device("cpu"), 1
        self.nf, self.ni = spec.sizes(model, C_)
        self.feature_dim = spec.FEATURE_DIM[model]
        self.serial = self.weights_version = 0
        self.log = []
        self.pending = None
        self.running_updates = 0

    def _enqueue(self, weights=False):
        self.serial += 1
        self.weights_version += int(weights)

    def set_state(self, flat, counters):
        self._enqueue(weights=True)
        self.log.append("set_state")

    def get_state(self):
        return np.zeros(self.nf, np.float32), np.zeros(self.ni, np.int64)

    def set_stochastic(self, dc=None, dr=None):
        self._dc, self._dr = dc, dr

    def forward_eval(self, x):
        self._enqueue()
        self.log.append("forward_eval")
        return torch.zeros(x.shape[0], self.feature_dim), torch.zeros(x.shape[0], C_)

    def forward_train(self, x1, x2=None):
        self._enqueue()
        self.pending = float(x1[0, 0, 0, 0])
        self.running_updates += 1
        self.log.append(("forward_train", self.pending))
        return torch.zeros(x1.shape[0], self.feature_dim), torch.zeros(x1.shape[0], C_)

    def forward_recompute(self, x1, x2=None):
        self._enqueue()
        self.pending = float(x1[0, 0, 0, 0])
        self.log.append(("recompute", self.pending))

    def backward_grads(self, dlogits=None, dfeat=None):
        assert self.pending is not None, "backward without a pending forward"
        self._enqueue()
        self.log.append(("backward", self.pending, dlogits is not None, dfeat is not None))
        self.pending = None

    def zero_grad(self):
        self.log.append("zero_grad")

    def adam_reset(self, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=5e-4):
        self._enqueue()
        self.log.append("adam_reset")

    def adam_step(self, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0):
        self._enqueue(weights=True)
        self.log.append(("adam_step", lr))


def _x(v, B=4):
    return torch.full((B, 3, HW, HW), float(v))


def _hipnet(monkeypatch, eng):
    monkeypatch.setattr(M, "get_engine", lambda *a, **k: eng)
    flat, cnt = spec.init_state("Resnet18", C_, 1037)
    return M.HipNet("Resnet18", C_, flat, cnt)


def test_latest_node_direct_other_node_recomputes():
    eng = FakeEngine()
    net = M.ResidentNet(eng).train()
    f1, z1 = net(_x(1))
    f2, z2 = net(_x(2))
    assert z1.grad_fn is not None and f2.grad_fn is not None
    eng.log.clear()
    (z1.sum() + z2.sum() + 0.5 * f1.pow(2).sum()).backward()
    # the later node runs first and finds its forward still the engine's last call; the earlier one recomputes
    # (the first backward claims the engine's gradient accumulator for this net: emptied once)
    assert eng.log == ["zero_grad", ("backward", 2.0, True, False), ("recompute", 1.0), ("backward", 1.0, True, True)], eng.log
    assert eng.running_updates == 2          # one running-statistics update per call, none for the recompute


def test_unused_logits_pass_none():
    eng = FakeEngine()
    net = M.ResidentNet(eng).train()
    f, _ = net(_x(3))
    eng.log.clear()
    f.pow(2).mean().backward()
    assert eng.log == ["zero_grad", ("backward", 3.0, False, True)], eng.log


def test_state_change_between_forward_and_backward_raises():
    eng = FakeEngine()
    net = M.ResidentNet(eng).train()
    opt = Adam(net, lr=1e-3)
    _, z1 = net(_x(1))
    _, z2 = net(_x(2))
    z2.sum().backward()
    opt.step()
    assert ("adam_step", 1e-3) in eng.log
    with pytest.raises(RuntimeError, match="weights changed"):
        z1.sum().backward()


def test_load_state_dict_between_forward_and_backward_raises(monkeypatch):
    eng = FakeEngine()
    net = _hipnet(monkeypatch, eng).train()
    _, z = net(_x(1))
    flat, cnt = spec.init_state("Resnet18", C_, 7)
    net.load_state_dict({k: torch.as_tensor(np.asarray(v)) for k, v in spec.flat_to_state_dict("Resnet18", C_, flat, cnt).items()})
    with pytest.raises(RuntimeError, match="weights changed"):
        z.sum().backward()


def test_rebind_then_recompute(monkeypatch):
    """Another net bound to the engine between the forward and the backward (an eval-mode teacher call): the node binds its
    net again and recomputes before the backward."""
    eng = FakeEngine()
    net = _hipnet(monkeypatch, eng).train()
    glob = _hipnet(monkeypatch, eng).eval()
    _, z = net(_x(1))
    glob(_x(1))
    eng.log.clear()
    z.sum().backward()
    assert eng.log == ["set_state", "zero_grad", ("recompute", 1.0), ("backward", 1.0, True, False)], eng.log
    assert eng._owner is net and eng._grad_owner is net


def test_no_grad_records_nothing():
    eng = FakeEngine()
    net = M.ResidentNet(eng).train()
    with torch.no_grad():
        f, z = net(_x(1))
    assert f.grad_fn is None and z.grad_fn is None
    assert eng.log == [("forward_train", 1.0)] and eng.running_updates == 1


def test_eval_mode_unchanged():
    eng = FakeEngine()
    net = M.ResidentNet(eng).eval()
    f, z = net(_x(1))
    assert f.grad_fn is None and eng.log == ["forward_eval"]


def test_adam_refuses_another_bound_net(monkeypatch):
    eng = FakeEngine()
    net = _hipnet(monkeypatch, eng).train()
    other = _hipnet(monkeypatch, eng).eval()
    opt = Adam(net, lr=1e-3)
    _, z = net(_x(1))
    z.sum().backward()
    other(_x(2))                             # the engine now holds another net's state
    with pytest.raises(RuntimeError, match="Adam moments belong to the engine"):
        opt.step()


def test_adam_reads_param_groups_each_step():
    eng = FakeEngine()
    net = M.ResidentNet(eng).train()
    opt = Adam(net, lr=1e-3, weight_decay=5e-4)
    assert eng.log == ["adam_reset"]         # a fresh optimizer: moments and step count reset
    for lr in (1e-3, 5e-4):
        opt.param_groups[0]["lr"] = lr
        opt.zero_grad()
        _, z = net(_x(1))
        z.sum().backward()
        opt.step()
    assert [e for e in eng.log if isinstance(e, tuple) and e[0] == "adam_step"] == [("adam_step", 1e-3), ("adam_step", 5e-4)]
