"""fedmlp_amd.optim's SGD / AdamW / clip functions and the optimizer state_dict, driven without a GPU: a fake engine records
what they ask of it (tests/test_autograd_cpu.py's style).  The arithmetic behind those calls is tests/test_optim_gpu.py's."""
import ctypes as C

import pytest
import torch

from fedmlp_amd import _lib
from fedmlp_amd import model as M
from fedmlp_amd.optim import SGD, Adam, AdamW, clip_grad_norm_, clip_grad_value_
from tests.test_autograd_cpu import FakeEngine as _AutogradFakeEngine
from tests.test_autograd_cpu import _hipnet, _x


class FakeEngine(_AutogradFakeEngine):
    """test_autograd_cpu's fake engine plus the calls of the new optimizers, the clips and the optimizer state."""

    def __init__(self, model="Resnet18"):
        super().__init__(model)
        self.opt_state = None

    def sgd_reset(self, lr=0.0, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False):
        self._enqueue()
        self.log.append("sgd_reset")

    def sgd_step(self, lr, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False):
        self._enqueue(weights=True)
        self.log.append(("sgd_step", lr, momentum, dampening, weight_decay, nesterov))

    def adamw_step(self, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2):
        self._enqueue(weights=True)
        self.log.append(("adamw_step", lr, weight_decay))

    def clip_grad_norm(self, max_norm):
        self.log.append(("clip_grad_norm", max_norm))
        return torch.tensor(3.0)

    def clip_grad_value(self, clip_value):
        self.log.append(("clip_grad_value", clip_value))

    def optim_state(self):
        return 7, torch.full((self.nf,), 1.0), torch.full((self.nf,), 2.0)

    def set_optim_state(self, step, m, v=None):
        self.log.append(("set_optim_state", step, v is not None))
        self.opt_state = (step, m, v)


def _steps(log, name):
    return [e for e in log if isinstance(e, tuple) and e[0] == name]


def _net():
    eng = FakeEngine()
    return eng, M.ResidentNet(eng).train()


def _backward(net, v=1):
    _, z = net(_x(v))
    z.sum().backward()


# ---- hyper-parameter validation ---------------------------------------------------------------------------------
def test_invalid_hyper_parameters_raise():
    eng, net = _net()
    with pytest.raises(ValueError):
        SGD(net, lr=-1e-3)
    with pytest.raises(ValueError):
        AdamW(net, lr=-1e-3)
    with pytest.raises(ValueError):
        SGD(net, lr=0.1, nesterov=True)                                 # Nesterov without momentum
    with pytest.raises(ValueError):
        SGD(net, lr=0.1, momentum=0.9, dampening=0.1, nesterov=True)    # Nesterov with dampening
    with pytest.raises(ValueError):
        clip_grad_norm_(net, -1.0)
    with pytest.raises(ValueError):
        clip_grad_norm_(net, 1.0, norm_type=1)
    with pytest.raises(ValueError):
        clip_grad_norm_(net, 1.0, norm_type=float("inf"))
    with pytest.raises(ValueError):
        clip_grad_value_(net, -0.5)
    assert not _steps(eng.log, "clip_grad_norm") and not _steps(eng.log, "clip_grad_value")
    SGD(net, lr=0.1, momentum=0.9, nesterov=True)                       # the valid form passes


# ---- the shared base: bound-engine check, reset, gradient owner, param_groups ---------------------------------------
@pytest.mark.parametrize("cls,kw,word", [(SGD, {"lr": 1e-2, "momentum": 0.9}, "SGD"), (AdamW, {"lr": 1e-3}, "AdamW")])
def test_refuses_another_bound_net(monkeypatch, cls, kw, word):
    eng = FakeEngine()
    net = _hipnet(monkeypatch, eng).train()
    other = _hipnet(monkeypatch, eng).eval()
    opt = cls(net, **kw)
    _backward(net)
    other(_x(2))                             # the engine now holds another net's state
    with pytest.raises(RuntimeError, match=f"{word}.step: the engine does not hold this optimizer's net .* the {word} moments belong "
                                           "to the engine"):
        opt.step()


def test_fresh_optimizer_resets_the_engine_state():
    eng, net = _net()
    SGD(net, lr=1e-2, momentum=0.9)
    AdamW(net)
    assert eng.log == ["sgd_reset", "adam_reset"]


def test_param_groups_read_each_step():
    eng, net = _net()
    sgd = SGD(net, lr=1e-2, momentum=0.9, dampening=0.1, weight_decay=5e-4)
    for lr in (1e-2, 5e-3):
        sgd.param_groups[0]["lr"] = lr
        sgd.zero_grad()
        _backward(net)
        sgd.step()
    assert _steps(eng.log, "sgd_step") == [("sgd_step", 1e-2, 0.9, 0.1, 5e-4, False), ("sgd_step", 5e-3, 0.9, 0.1, 5e-4, False)]
    adamw = AdamW(net, lr=1e-3)
    assert adamw.defaults["weight_decay"] == 1e-2
    for lr in (1e-3, 2e-3):
        adamw.param_groups[0]["lr"] = lr
        adamw.zero_grad()
        _backward(net)
        adamw.step()
    assert _steps(eng.log, "adamw_step") == [("adamw_step", 1e-3, 1e-2), ("adamw_step", 2e-3, 1e-2)]
    assert not _steps(eng.log, "adam_step")          # AdamW never takes the coupled-L2 step


@pytest.mark.parametrize("cls,kw,name", [(SGD, {"lr": 1e-2}, "sgd_step"), (AdamW, {}, "adamw_step"), (Adam, {}, "adam_step")])
def test_step_without_gradients_is_a_noop(cls, kw, name):
    eng, net = _net()
    opt = cls(net, **kw)
    wv = eng.weights_version
    key = net._weights_key()
    opt.step()                               # no backward ran: the accumulator is not this net's
    assert not _steps(eng.log, name) and eng.weights_version == wv and net._weights_key() == key
    _backward(net)
    opt.step()
    assert len(_steps(eng.log, name)) == 1 and net._weights_key() != key


# ---- clipping acts only on the net that owns the accumulator ---------------------------------------------------
def test_clip_needs_the_gradient_owner():
    eng, net = _net()
    n = clip_grad_norm_(net, 1.0)
    clip_grad_value_(net, 0.5)
    assert float(n) == 0.0 and eng.log == []
    _backward(net)
    n = clip_grad_norm_(net, 1.0)
    clip_grad_value_(net, 0.5)
    assert float(n) == 3.0
    assert eng.log[-2:] == [("clip_grad_norm", 1.0), ("clip_grad_value", 0.5)]


# ---- optimizer state ------------------------------------------------------------------------------------------
def test_state_dict_keys_and_load():
    eng, net = _net()
    sd = Adam(net, lr=1e-3).state_dict()
    assert set(sd) == {"state", "param_groups"} and set(sd["state"]) == {"step", "exp_avg", "exp_avg_sq"}
    assert sd["state"]["step"] == 7 and sd["param_groups"][0]["lr"] == 1e-3
    assert set(AdamW(net).state_dict()["state"]) == {"step", "exp_avg", "exp_avg_sq"}
    sgd = SGD(net, lr=1e-2, momentum=0.9)
    sd = sgd.state_dict()
    assert set(sd["state"]) == {"step", "momentum_buffer"} and sd["state"]["momentum_buffer"].numel() == eng.nf
    sd["param_groups"][0]["lr"] = 0.5
    sgd2 = SGD(net, lr=1e-2, momentum=0.9)
    sgd2.load_state_dict(sd)
    assert eng.log[-1] == ("set_optim_state", 7, False) and sgd2.param_groups[0]["lr"] == 0.5
    assert torch.equal(eng.opt_state[1], sd["state"]["momentum_buffer"])
    adam = Adam(net)
    adam.load_state_dict(Adam(net).state_dict())
    assert eng.log[-1] == ("set_optim_state", 7, True)


def test_load_state_dict_wrong_length_raises():
    eng, net = _net()
    opt = SGD(net, lr=1e-2, momentum=0.9)
    sd = opt.state_dict()
    sd["state"]["momentum_buffer"] = sd["state"]["momentum_buffer"][:-1]
    with pytest.raises(ValueError, match="momentum_buffer has"):
        opt.load_state_dict(sd)
    with pytest.raises(ValueError, match="lacks"):
        Adam(net).load_state_dict({"state": {"step": 1, "exp_avg": torch.zeros(eng.nf)}})
    assert not _steps(eng.log, "set_optim_state")


def test_state_loaded_before_the_net_is_bound_is_installed_at_the_first_step(monkeypatch):
    eng = FakeEngine()
    net = _hipnet(monkeypatch, eng).train()         # not bound yet: the net never ran
    opt = SGD(net, lr=1e-2, momentum=0.9)
    assert eng.log == []
    opt.load_state_dict({"state": {"step": 3, "momentum_buffer": torch.ones(eng.nf)}, "param_groups": [dict(opt.param_groups[0])]})
    assert eng.log == [] and opt.state_dict()["state"]["step"] == 3
    _backward(net)
    opt.step()
    i = eng.log.index("sgd_reset")
    assert eng.log[i + 1] == ("set_optim_state", 3, False) and eng.log[i + 2][0] == "sgd_step"


# ---- the ctypes table ---------------------------------------------------------------------------------------------
def test_symbols_of_the_new_entry_points():
    P, F32, I64 = C.c_void_p, C.c_float, C.c_int64
    want = {
        "fm_sgd_reset": [P, C.POINTER(_lib.FmSgd)],
        "fm_sgd_step": [P, C.POINTER(_lib.FmSgd)],
        "fm_adamw_step": [P, C.POINTER(_lib.FmAdam)],
        "fm_grad_norm": [P, P],
        "fm_clip_grad_norm": [P, F32, P],
        "fm_clip_grad_value": [P, F32],
        "fm_optim_get_state": [P, P, P, C.POINTER(I64)],
        "fm_optim_set_state": [P, P, P, I64],
    }
    for name, args in want.items():
        res, got = _lib.SYMBOLS[name]
        assert res is C.c_int and got == args, name
    # the struct the header declares beside them: typedef struct fm_sgd { float lr, momentum, dampening, weight_decay; int32_t nesterov; }
    assert [(n, t) for n, t in _lib.FmSgd._fields_] == [("lr", F32), ("momentum", F32), ("dampening", F32), ("weight_decay", F32),
                                                        ("nesterov", C.c_int32)]
    assert C.sizeof(_lib.FmSgd) == 20
