"""Bookkeeping of HipNet.freeze_bn() (frozen BatchNorm statistics for the differentiable train-mode net(x)), driven without a
GPU: a fake engine records what HipNet and the autograd node ask of it, and in which BatchNorm mode.  The arithmetic behind
those calls is tests/test_freeze_bn_gpu.py's."""
import copy

import numpy as np
import pytest
import torch

from fedmlp_amd import _lib
from fedmlp_amd import model as M
from fedmlp_amd import spec
from fedmlp_amd.engine import Engine

C_, HW = 5, 64


class FakeEngine:
    """The Engine surface the node and HipNet use, with the bn_freeze flag; forwards log the flag they ran under."""

    def __init__(self):
        self.model, self.n_classes, self.in_h, self.in_w = "Resnet18", C_, HW, HW
        self.max_images, self.precision, self.device, self.h = 16, "fp32", torch.device("cpu"), 1
        self.nf, self.ni = spec.sizes("Resnet18", C_)
        self.feature_dim = spec.FEATURE_DIM["Resnet18"]
        self.serial = self.weights_version = 0
        self.log = []
        self.pending = None
        self.bn_frozen = False
        self._dirty = False

    def _enqueue(self, weights=False):
        self.serial += 1
        self.weights_version += int(weights)

    def set_state(self, flat, counters):
        self._enqueue(weights=True)
        self.log.append("set_state")

    def get_state(self):
        return np.zeros(self.nf, np.float32), np.zeros(self.ni, np.int64)

    def bn_freeze(self, on=True):
        self.bn_frozen = bool(on)
        self.log.append(("bn_freeze", self.bn_frozen))

    def forward_eval(self, x):
        self._enqueue()
        self.log.append("forward_eval")
        return torch.zeros(x.shape[0], self.feature_dim), torch.zeros(x.shape[0], C_)

    def forward_train(self, x1, x2=None):
        self._enqueue()
        self.pending = (float(x1[0, 0, 0, 0]), self.bn_frozen)
        self.log.append(("forward_train",) + self.pending)
        return torch.zeros(x1.shape[0], self.feature_dim), torch.zeros(x1.shape[0], C_)

    def forward_recompute(self, x1, x2=None):
        self._enqueue()
        self.pending = (float(x1[0, 0, 0, 0]), self.bn_frozen)
        self.log.append(("recompute",) + self.pending)

    def backward_grads(self, dlogits=None, dfeat=None, dx=None):
        assert self.pending is not None, "backward without a pending forward"
        self._enqueue()
        self.log.append(("backward",) + self.pending)       # the engine's backward runs in the pending forward's mode
        self.pending = None

    def zero_grad(self):
        self.log.append("zero_grad")


def _x(v, B=4):
    return torch.full((B, 3, HW, HW), float(v))


def _hipnet(monkeypatch, eng):
    monkeypatch.setattr(M, "get_engine", lambda *a, **k: eng)
    flat, cnt = spec.init_state("Resnet18", C_, 1037)
    return M.HipNet("Resnet18", C_, flat, cnt)


def test_freeze_bn_returns_self_and_defaults_off():
    eng = FakeEngine()
    net = M.ResidentNet(eng)
    assert net.bn_frozen is False
    assert net.freeze_bn() is net and net.bn_frozen is True
    assert net.freeze_bn(False) is net and net.bn_frozen is False


def test_train_call_sets_the_flag_before_forward_train():
    eng = FakeEngine()
    net = M.ResidentNet(eng).train().freeze_bn()
    f, z = net(_x(1))
    assert f.grad_fn is not None and z.grad_fn is not None            # the same node as a batch-statistics call
    # ... and the engine is handed back with the flag its caller left
    assert eng.log == [("bn_freeze", True), ("forward_train", 1.0, True), ("bn_freeze", False)], eng.log
    # a batch-statistics call on an engine whose flag somebody set clears it for its own forward
    eng.log.clear()
    eng.bn_frozen = True
    net.freeze_bn(False)
    net(_x(2))
    assert eng.log == [("bn_freeze", False), ("forward_train", 2.0, False), ("bn_freeze", True)], eng.log


def test_frozen_call_does_not_mark_running_statistics_dirty(monkeypatch):
    eng = FakeEngine()
    net = _hipnet(monkeypatch, eng).train().freeze_bn()
    net(_x(1))
    assert eng._dirty is False              # nothing moved on the engine: state_dict() needs no download
    net.freeze_bn(False)
    net(_x(1))
    assert eng._dirty is True


def test_node_reinstalls_its_mode_around_a_recompute_and_restores_the_callers():
    eng = FakeEngine()
    net = M.ResidentNet(eng).train()
    _, z1 = net(_x(1))                      # batch-statistics node
    net.freeze_bn(True)
    _, z2 = net(_x(2))                      # frozen node
    for flag in (True, False):              # whatever the engine's flag is when the backward runs
        eng.bn_frozen = flag
        eng.log.clear()
        (z1.sum() + z2.sum()).backward(retain_graph=flag)
        # node 2 finds its forward pending (the engine knows its mode); node 1 recomputes in ITS mode and hands the engine back
        want = [("backward", 2.0, True)]
        want += [("bn_freeze", False), ("recompute", 1.0, False), ("bn_freeze", True)] if flag else [("recompute", 1.0, False)]
        want += [("backward", 1.0, False)]
        if flag:
            assert eng.log == ["zero_grad"] + want, eng.log
        else:       # second backward of the same graph: node 2's forward is no longer pending, it recomputes frozen
            assert eng.log == [("bn_freeze", True), ("recompute", 2.0, True), ("bn_freeze", False), ("backward", 2.0, True),
                               ("recompute", 1.0, False), ("backward", 1.0, False)], eng.log
        assert eng.bn_frozen is flag


def test_frozen_node_refuses_moved_running_statistics():
    eng = FakeEngine()
    net = M.ResidentNet(eng).train().freeze_bn()
    _, z1 = net(_x(1))
    net.freeze_bn(False)
    net(_x(2))                              # one running-statistics update: the frozen forward cannot be recomputed any more
    with pytest.raises(RuntimeError, match="running statistics"):
        z1.sum().backward()


def test_same_mode_recompute_leaves_the_flag_alone():
    eng = FakeEngine()
    net = M.ResidentNet(eng).train().freeze_bn()
    _, z1 = net(_x(1))
    _, z2 = net(_x(2))
    eng.bn_frozen = True                    # the caller's flag is already the node's mode
    eng.log.clear()
    (z1.sum() + z2.sum()).backward()
    assert eng.log == ["zero_grad", ("backward", 2.0, True), ("recompute", 1.0, True), ("backward", 1.0, True)], eng.log


def test_deepcopy_keeps_the_mode(monkeypatch):
    eng = FakeEngine()
    net = _hipnet(monkeypatch, eng).train().freeze_bn()
    c = copy.deepcopy(net)
    assert c is not net and c.bn_frozen is True and c.training is True
    assert copy.deepcopy(net.freeze_bn(False)).bn_frozen is False
    res = M.ResidentNet(eng).freeze_bn()
    assert copy.deepcopy(res) is res and res.bn_frozen is True


def test_eval_mode_call_is_unchanged():
    eng = FakeEngine()
    net = M.ResidentNet(eng).eval().freeze_bn()
    f, z = net(_x(1))
    assert f.grad_fn is None and z.grad_fn is None and eng.log == ["forward_eval"]


def test_no_grad_runs_the_frozen_forward_and_records_nothing():
    eng = FakeEngine()
    net = M.ResidentNet(eng).train().freeze_bn()
    with torch.no_grad():
        f, z = net(_x(1))
    assert f.grad_fn is None and z.grad_fn is None
    assert eng.log == [("bn_freeze", True), ("forward_train", 1.0, True), ("bn_freeze", False)], eng.log


def test_engine_surface_and_abi_table():
    assert callable(getattr(Engine, "bn_freeze")) and isinstance(getattr(Engine, "bn_frozen"), property)
    assert len(_lib.SYMBOLS["fm_bn_freeze"][1]) == 2 and len(_lib.SYMBOLS["fm_bn_frozen"][1]) == 1
