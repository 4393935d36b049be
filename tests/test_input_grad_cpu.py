"""The input-gradient bookkeeping of the train-mode net(x) autograd node (fedmlp_amd.model._TrainCall), driven without a
GPU: a fake engine records what the node asks of it and fills dx with a value that names the forward it belongs to.  The
arithmetic behind those calls is tests/test_input_grad_gpu.py's."""
import inspect

import numpy as np
import torch

from fedmlp_amd import _lib
from fedmlp_amd import model as M
from fedmlp_amd import spec
from fedmlp_amd.engine import Engine

C_, HW = 5, 64


class FakeEngine:
    """The Engine surface the node uses; `strict` refuses the dx keyword like an engine that only knows the two-argument form."""

    def __init__(self, strict=False):
        self.model, self.n_classes, self.in_h, self.in_w = "Resnet18", C_, HW, HW
        self.max_images, self.precision, self.device, self.h = 16, "fp32", torch.device("cpu"), 1
        self.nf, self.ni = spec.sizes("Resnet18", C_)
        self.feature_dim = spec.FEATURE_DIM["Resnet18"]
        self.serial = self.weights_version = 0
        self.log = []
        self.pending = None
        self.strict = strict

    def _enqueue(self):
        self.serial += 1

    def get_state(self):
        return np.zeros(self.nf, np.float32), np.zeros(self.ni, np.int64)

    def forward_train(self, x1, x2=None):
        assert not x1.requires_grad, "the engine is handed the detached copy"
        self._enqueue()
        self.pending = float(x1[0, 0, 0, 0])
        self.log.append(("forward_train", self.pending))
        return torch.zeros(x1.shape[0], self.feature_dim), torch.zeros(x1.shape[0], C_)

    def forward_recompute(self, x1, x2=None):
        assert not x1.requires_grad
        self._enqueue()
        self.pending = float(x1[0, 0, 0, 0])
        self.log.append(("recompute", self.pending))

    def backward_grads(self, dlogits=None, dfeat=None, **kw):
        assert self.pending is not None, "backward without a pending forward"
        assert not (self.strict and kw), "the two-argument form was expected"
        assert set(kw) <= {"dx"}
        self._enqueue()
        dx = kw.get("dx")
        if dx is not None:
            assert dx.dtype == torch.float32 and dx.is_contiguous() and tuple(dx.shape[1:]) == (3, HW, HW)
            dx.fill_(10.0 * self.pending)
        self.log.append(("backward", self.pending, "dx" in kw))
        self.pending = None

    def zero_grad(self):
        pass


def _x(v, B=4, grad=False):
    return torch.full((B, 3, HW, HW), float(v)).requires_grad_(grad)


def test_dx_is_requested_only_when_x_requires_grad():
    eng = FakeEngine()
    net = M.ResidentNet(eng).train()
    x = _x(3, grad=True)
    f, z = net(x)
    z.sum().backward()
    assert eng.log[-1] == ("backward", 3.0, True), eng.log
    assert x.grad is not None and x.grad.shape == x.shape and x.grad.dtype == x.dtype
    assert torch.equal(x.grad, torch.full_like(x, 30.0))          # the engine's dx, in x's position


def test_two_argument_call_when_x_does_not_require_grad():
    eng = FakeEngine(strict=True)
    net = M.ResidentNet(eng).train()
    x = _x(2)
    f, z = net(x)
    (z.sum() + f.sum()).backward()
    assert eng.log[-1] == ("backward", 2.0, False), eng.log
    assert x.grad is None


def test_recompute_path_returns_each_nodes_own_dx():
    eng = FakeEngine()
    net = M.ResidentNet(eng).train()
    x1, x2, x3 = _x(1, grad=True), _x(2, grad=True), _x(5)
    f1, z1 = net(x1)
    f2, z2 = net(x2)
    f3, z3 = net(x3)
    eng.log.clear()
    (z1.sum() + z2.sum() + z3.sum()).backward()
    assert eng.log == [("backward", 5.0, False), ("recompute", 2.0), ("backward", 2.0, True), ("recompute", 1.0),
                       ("backward", 1.0, True)], eng.log
    assert torch.equal(x1.grad, torch.full_like(x1, 10.0)) and torch.equal(x2.grad, torch.full_like(x2, 20.0))
    assert x3.grad is None


def test_second_backward_accumulates_in_torch():
    eng = FakeEngine()
    net = M.ResidentNet(eng).train()
    x = _x(4, grad=True)
    net(x)[1].sum().backward()
    net(x)[1].sum().backward()
    assert torch.equal(x.grad, torch.full_like(x, 80.0))           # the engine writes dx, autograd adds


def test_gradient_reaches_a_tensor_upstream_of_x():
    eng = FakeEngine()
    net = M.ResidentNet(eng).train()
    base = _x(1, grad=True)
    f, z = net(2.0 * base)                                         # x itself is not a leaf
    z.sum().backward()
    assert torch.equal(base.grad, torch.full_like(base, 40.0))


def test_export_is_declared_and_engine_takes_dx():
    assert len(_lib.SYMBOLS["fm_backward_grads_x"][1]) == len(_lib.SYMBOLS["fm_backward_grads"][1]) + 2
    sig = inspect.signature(Engine.backward_grads)
    assert list(sig.parameters)[1:] == ["dlogits", "dfeat", "dx"] and sig.parameters["dx"].default is None
