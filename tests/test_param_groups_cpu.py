"""net.requires_grad_ / net.trainable and the optimizers' parameter groups, driven without a GPU: a fake engine records what
they ask of it (tests/test_optim_cpu.py's style).  The arithmetic behind those calls is tests/test_param_groups_gpu.py's."""
import copy
import ctypes as C

import pytest
import torch

from fedmlp_amd import _lib, spec
from fedmlp_amd import model as M
from fedmlp_amd.optim import SGD, Adam, AdamW
from tests.test_autograd_cpu import _hipnet, _x
from tests.test_optim_cpu import FakeEngine as _OptimFakeEngine

C_ = 5


class FakeEngine(_OptimFakeEngine):
    """test_optim_cpu's fake engine plus the mask, the group table and the grouped steps."""

    def set_trainable(self, flags):
        self.log.append(("set_trainable", tuple(int(f) for f in flags)))

    def optim_groups(self, group_of_entry, n_groups):
        self.log.append(("optim_groups", tuple(group_of_entry), n_groups))

    def adam_step_groups(self, hps):
        self._enqueue(weights=True)
        self.log.append(("adam_step_groups", [tuple(h) for h in hps]))

    def adamw_step_groups(self, hps):
        self._enqueue(weights=True)
        self.log.append(("adamw_step_groups", [tuple(h) for h in hps]))

    def sgd_step_groups(self, hps):
        self._enqueue(weights=True)
        self.log.append(("sgd_step_groups", [tuple(h) for h in hps]))


def _net(model="Resnet18"):
    eng = FakeEngine(model)
    return eng, M.ResidentNet(eng).train()


def _backward(net, v=1):
    _, z = net(_x(v))
    z.sum().backward()


def _named(log, name):
    return [e for e in log if isinstance(e, tuple) and e[0] == name]


def _keys(model="Resnet18"):
    return [k for k, _, _ in spec.entries(model, C_)]


# ---- prefix resolution ----------------------------------------------------------------------------------------------
def test_prefix_matches_whole_components_only():
    _, net = _net()
    assert net._resolve(["fc"], "t") == ["fc.weight", "fc.bias"]
    assert net._resolve("layer3.1.bn2", "t") == ["layer3.1.bn2.weight", "layer3.1.bn2.bias"]
    assert net._resolve(["conv1.weight"], "t") == ["conv1.weight"]
    l1 = net._resolve(["layer1"], "t")
    assert l1 and all(k.startswith("layer1.") for k in l1)
    assert len(l1) == 2 * (2 + 4)                      # two blocks: two conv weights, two BatchNorm (weight, bias) each
    assert not any("running" in k or "num_batches" in k for k in l1)
    # a prefix is a run of whole dotted components: "layer" is the head of every "layerN" and names nothing; "bn" neither
    for bad in ("layer", "layer1.0.bn", "f", "conv"):
        with pytest.raises(ValueError, match="names no trainable parameter"):
            net._resolve([bad], "t")
    _, eff = _net("Efficient_b0")
    assert eff._resolve(["_fc"], "t") == ["_fc.weight", "_fc.bias"]
    with pytest.raises(ValueError):
        eff._resolve(["fc"], "t")                      # "fc" is not "_fc"
    b1 = eff._resolve(["_blocks.1"], "t")
    assert b1 and all(k.startswith("_blocks.1.") for k in b1)          # not _blocks.10 .. _blocks.15
    assert eff._resolve(["_conv_head"], "t") == ["_conv_head.weight"]


def test_requires_grad_and_trainable():
    _, net = _net()
    keys = [k for k in _keys() if spec.is_trainable(k)]
    assert list(net.trainable()) == keys and all(net.trainable().values())
    assert net.requires_grad_(False) is net and not any(net.trainable().values())
    net.requires_grad_(True, ["layer4", "fc"])
    t = net.trainable()
    assert [k for k in keys if t[k]] == [k for k in keys if k.startswith("layer4.") or k.startswith("fc.")]
    net.requires_grad_(False, ["fc.bias"])
    assert not net.trainable()["fc.bias"] and net.trainable()["fc.weight"]
    net.requires_grad_()                               # flag=True, names=None: every parameter
    assert all(net.trainable().values()) and net._frozen == frozenset()


def test_unknown_and_buffer_names_raise():
    _, net = _net()
    for bad in ("nope", "bn1.running_mean", "layer1.0.bn1.num_batches_tracked", "bn1.running_var"):
        with pytest.raises(ValueError, match="names no trainable parameter"):
            net.requires_grad_(False, [bad])
    assert all(net.trainable().values())               # nothing was changed by the failed calls
    with pytest.raises(ValueError):
        Adam(net, groups=[{"params": ["bn1.running_mean"]}])


def test_deepcopy_carries_the_mask(monkeypatch):
    eng = FakeEngine()
    net = _hipnet(monkeypatch, eng).train().requires_grad_(False, ["layer1", "conv1"])
    c = copy.deepcopy(net)
    assert c is not net and c.trainable() == net.trainable() and not c.trainable()["conv1.weight"]
    c.requires_grad_(True)
    assert not net.trainable()["conv1.weight"]         # the copy's mask is its own


# ---- the mask reaches the engine ----------------------------------------------------------------------------------
def test_mask_is_installed_before_the_forward_and_only_when_it_changes():
    eng, net = _net()
    _backward(net)
    assert not _named(eng.log, "set_trainable")        # the default mask: an engine that never saw one is not called
    net.requires_grad_(False).requires_grad_(True, ["fc"])
    eng.log.clear()
    _backward(net)
    want = tuple(int(k in ("fc.weight", "fc.bias")) for k in _keys())
    assert eng.log[0] == ("set_trainable", want) and eng.log[1][0] == "forward_train"
    eng.log.clear()
    _backward(net, 2)
    assert not _named(eng.log, "set_trainable")
    net.requires_grad_(True)
    _backward(net, 3)
    assert _named(eng.log, "set_trainable") == [("set_trainable", tuple(int(spec.is_trainable(k)) for k in _keys()))]


def test_recompute_runs_under_the_mask_of_its_forward():
    eng, net = _net()
    net.requires_grad_(False, ["conv1"])
    m1 = tuple(int(spec.is_trainable(k) and k != "conv1.weight") for k in _keys())
    _, z1 = net(_x(1))
    net.requires_grad_(True).requires_grad_(False, ["fc"])
    m2 = tuple(int(spec.is_trainable(k) and not k.startswith("fc.")) for k in _keys())
    _, z2 = net(_x(2))
    eng.log.clear()
    (z1.sum() + z2.sum()).backward()
    # the later node's forward is still pending (the engine remembers its mask); the earlier one recomputes under ITS mask,
    # and the net's own comes back afterwards
    i = eng.log.index(("recompute", 1.0))
    assert eng.log[i - 1] == ("set_trainable", m1) and eng.log[i + 1] == ("set_trainable", m2)
    assert eng.log[i + 2][:2] == ("backward", 1.0)


# ---- parameter groups -----------------------------------------------------------------------------------------------
def test_overlapping_groups_raise():
    _, net = _net()
    with pytest.raises(ValueError, match="more than one parameter group"):
        Adam(net, groups=[{"params": ["layer4"]}, {"params": ["layer4.1.conv2.weight"]}])
    with pytest.raises(ValueError, match="more than one parameter group"):
        SGD(net, lr=0.1, groups=[{"params": ["fc", "fc.bias"]}, {"params": ["fc.bias"]}])
    with pytest.raises(ValueError, match="parameter groups are supported"):
        Adam(net, groups=[{"params": [k]} for k in [k for k in _keys() if spec.is_trainable(k)][:9]])
    with pytest.raises(ValueError, match="unknown options"):
        Adam(net, groups=[{"params": ["fc"], "momentum": 0.9}])
    with pytest.raises(ValueError, match="invalid hyper-parameters"):
        AdamW(net, groups=[{"params": ["fc"], "lr": -1.0}])


def test_unnamed_parameters_are_not_optimized_and_groups_merge_defaults():
    eng, net = _net()
    opt = AdamW(net, lr=1e-3, weight_decay=1e-2, groups=[{"params": ["fc"]}, {"params": ["layer4"], "lr": 1e-4, "betas": [0.8, 0.9]}])
    assert opt.param_groups[0] == {"lr": 1e-3, "betas": (0.9, 0.999), "eps": 1e-8, "weight_decay": 1e-2,
                                   "params": ["fc.weight", "fc.bias"]}
    assert opt.param_groups[1]["lr"] == 1e-4 and opt.param_groups[1]["betas"] == (0.8, 0.9)
    assert opt.param_groups[1]["params"] == net._resolve(["layer4"], "t")
    _backward(net)
    opt.step()
    (_, of, n), = _named(eng.log, "optim_groups")
    assert n == 2
    for k, g in zip(_keys(), of):
        assert g == (0 if k.startswith("fc.") else 1 if k.startswith("layer4.") and spec.is_trainable(k) else -1), k
    assert _named(eng.log, "adamw_step_groups") == [("adamw_step_groups", [(1e-3, (0.9, 0.999), 1e-8, 1e-2), (1e-4, (0.8, 0.9), 1e-8, 1e-2)])]
    assert not _named(eng.log, "adamw_step") and not _named(eng.log, "adam_step")
    opt.zero_grad(); _backward(net, 2); opt.step()
    assert len(_named(eng.log, "optim_groups")) == 1   # the table is sent once, not per step


def test_param_groups_are_read_at_every_step():
    eng, net = _net()
    opt = SGD(net, lr=1e-2, momentum=0.9, groups=[{"params": ["fc"]}, {"params": ["layer4"], "lr": 1e-3, "momentum": 0.0}])
    for lr in (1e-2, 5e-3):
        opt.param_groups[0]["lr"] = lr
        opt.zero_grad(); _backward(net); opt.step()
    assert _named(eng.log, "sgd_step_groups") == [
        ("sgd_step_groups", [(1e-2, 0.9, 0, 0, False), (1e-3, 0.0, 0, 0, False)]),
        ("sgd_step_groups", [(5e-3, 0.9, 0, 0, False), (1e-3, 0.0, 0, 0, False)])]
    opt.param_groups[1]["lr"] = -1.0
    _backward(net)
    with pytest.raises(ValueError):
        opt.step()


def test_mask_without_groups_steps_one_group_of_the_trainable_parameters():
    eng, net = _net()
    net.requires_grad_(False).requires_grad_(True, ["layer4", "fc"])
    opt = Adam(net, lr=2e-3)
    assert "params" not in opt.param_groups[0]
    _backward(net)
    opt.step()
    (_, of, n), = _named(eng.log, "optim_groups")
    live = net.trainable()
    assert n == 1 and of == tuple(0 if live.get(k, False) else -1 for k in _keys())
    assert _named(eng.log, "adam_step_groups") == [("adam_step_groups", [(2e-3, (0.9, 0.999), 1e-8, 0)])]
    assert not _named(eng.log, "adam_step")
    net.requires_grad_(True)                           # back to the default mask: the single-group call again
    opt.zero_grad(); _backward(net, 2); opt.step()
    assert _named(eng.log, "adam_step") == [("adam_step", 2e-3)] and len(_named(eng.log, "adam_step_groups")) == 1


def test_state_dict_round_trip_with_three_groups():
    eng, net = _net()
    groups = [{"params": ["fc"]}, {"params": ["layer4"], "lr": 1e-4}, {"params": ["layer3", "conv1"], "weight_decay": 0.0}]
    opt = AdamW(net, lr=1e-3, groups=groups)
    sd = opt.state_dict()
    assert len(sd["param_groups"]) == 3 and [g["params"] for g in sd["param_groups"]] == [g["params"] for g in opt.param_groups]
    assert sd["state"]["step"] == 7 and sd["state"]["exp_avg"].numel() == eng.nf        # two flat tensors, net.grads() layout
    sd["param_groups"][1]["lr"] = 0.5
    opt2 = AdamW(net, lr=1e-3, groups=groups)
    opt2.load_state_dict(sd)
    assert eng.log[-1] == ("set_optim_state", 7, True)
    assert opt2.param_groups[1]["lr"] == 0.5 and opt2.param_groups[2]["weight_decay"] == 0.0
    assert opt2.param_groups[0]["params"] == ["fc.weight", "fc.bias"]
    # mismatches: the group count, and the parameters a group names
    with pytest.raises(ValueError, match="parameter groups"):
        AdamW(net, groups=groups[:2]).load_state_dict(sd)
    with pytest.raises(ValueError, match="parameter groups"):
        AdamW(net).load_state_dict(sd)
    with pytest.raises(ValueError, match="names other parameters"):
        AdamW(net, groups=[groups[1], groups[0], groups[2]]).load_state_dict(sd)
    with pytest.raises(ValueError, match="names other parameters"):
        AdamW(net, groups=groups).load_state_dict({"state": sd["state"], "param_groups": [{"lr": 1e-3}] * 3})
    n = len(_named(eng.log, "set_optim_state"))
    assert n == 1                                      # no failed load reached the engine


# ---- nothing changes while no mask or group is installed -----------------------------------------------------------
def _one_step(make, with_new_arguments):
    eng, net = _net()
    if with_new_arguments:
        net.requires_grad_(True, None)
    opt = make(net, with_new_arguments)
    opt.zero_grad()
    _backward(net)
    opt.step()
    return eng.log


@pytest.mark.parametrize("cls,kw", [(Adam, {"lr": 1e-3, "weight_decay": 5e-4}), (AdamW, {"lr": 1e-3}),
                                    (SGD, {"lr": 1e-2, "momentum": 0.9, "nesterov": True})])
def test_default_path_issues_the_same_engine_calls(cls, kw):
    """groups=None and the default mask: the engine-call log of one step is the log of the same step taken without the new
    arguments (recorded here, from an optimizer built the old way)."""
    old = _one_step(lambda net, new: cls(net, **kw), False)
    new = _one_step(lambda net, new: cls(net, groups=None, **kw), True)
    assert new == old
    step = {"Adam": "adam_step", "AdamW": "adamw_step", "SGD": "sgd_step"}[cls.__name__]
    assert len(_named(old, step)) == 1
    for name in ("set_trainable", "optim_groups", step + "_groups"):
        assert not _named(old, name) and not _named(new, name)


# ---- the ctypes table -------------------------------------------------------------------------------------------------
def test_symbols_of_the_new_entry_points():
    P, I32 = C.c_void_p, C.c_int32
    want = {
        "fm_set_trainable": [P, P, I32],
        "fm_get_trainable": [P, P, I32],
        "fm_optim_groups": [P, P, I32, I32],
        "fm_adam_step_groups": [P, C.POINTER(_lib.FmAdam), I32],
        "fm_adamw_step_groups": [P, C.POINTER(_lib.FmAdam), I32],
        "fm_sgd_step_groups": [P, C.POINTER(_lib.FmSgd), I32],
    }
    for name, args in want.items():
        res, got = _lib.SYMBOLS[name]
        assert res is C.c_int and got == args, name
    assert _lib.FM_MAX_GROUPS == 8 == Adam.MAX_GROUPS
