"""FedLSR / FedIRM without a GPU: the float64 restatement of the heads (tests/irm_lsr_ref.py) against the reference's own
building blocks (tests/golden/irm_lsr_kat.npz, recorded by tests/golden/make_irm_lsr_golden.py), FedAvg_rela bit for bit, the
C ABI's new names, the driver's parser, the host mirror's schedules, and the statement of include/fedmlp_hip.h that torch's
fp32 autograd of the FedLSR chain is NaN once p rounds to 1 while the rational form is finite."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from tests import irm_lsr_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["fm_loss_fedlsr", "fm_loss_fedirm_sup", "fm_loss_fedirm_rel", "fm_step_fedlsr", "fm_teacher_ema_params"]


@pytest.fixture(scope="module")
def kat():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "irm_lsr_kat.npz")))


def _close(got, want):
    """float64 rounding: a few ulps of the largest magnitude involved (the operation order may differ)"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape
    assert np.abs(got - want).max() <= 64 * np.finfo(np.float64).eps * max(1.0, np.abs(want).max())


def test_restatement_against_the_reference_functions(kat):
    t = torch.from_numpy
    z1, z2, y, conf = (t(kat[k]) for k in ("z1", "z2", "y", "conf"))
    q1 = torch.clamp(torch.sigmoid(z1 * 3), min=1e-6, max=1.0)
    q2 = torch.clamp(torch.sigmoid(z2 * 3), min=1e-6, max=1.0)
    _close(R.js(q1, q2).numpy(), kat["js"])
    p = torch.sigmoid(z1) * 0.3 + torch.sigmoid(z2) * 0.7
    _close(R.anti_sigmoid(p).numpy(), kat["anti_sigmoid"])
    _close(R.confuse_matrix(z1, y).numpy(), kat["confuse_y"])
    assert (kat["confuse_y"][3] == 0.5).all()                  # the class without positives: 0 / 1e-8 -> sigmoid(0)
    pr = torch.sigmoid(conf)
    rows = torch.where(torch.all((pr > 0.7) | (pr < 0.3), dim=1))[0]
    assert rows.tolist() == kat["find_rows"].tolist()
    Q = R.confuse_matrix(conf[rows], pr[rows] > 0.5)
    _close(Q.numpy(), kat["confuse_pseudo"])
    _close(R.kd_loss(Q, t(kat["mats"][0])).numpy(), kat["kd"])
    _close(R.sigmoid_mse(z1, z2).numpy(), kat["mse"])


def test_fedavg_rela_bit_for_bit(kat):
    from fedmlp_amd.fedavg import FedAvg_rela
    P = [torch.from_numpy(m.astype(np.float32)) for m in kat["mats"]]
    active = [[int(c) for c in row if c >= 0] for row in kat["rela_active"]]
    assert sorted(len(a) for a in active)[0] == 1              # a class with a single active client
    out = FedAvg_rela(P, [int(w) for w in kat["rela_weight"]], active)
    assert out.dtype == torch.float32
    assert np.array_equal(out.numpy().view(np.uint32), kat["rela"].view(np.uint32))


def test_new_names_declared_exported_and_bound():
    from fedmlp_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "fedmlp_hip.h")).read()
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), f"{name} is not declared in include/fedmlp_hip.h"
        assert name in _lib.SYMBOLS and _lib.SYMBOLS[name][0] is C.c_int, name
    assert len(_lib.SYMBOLS["fm_loss_fedlsr"][1]) == 9 and len(_lib.SYMBOLS["fm_loss_fedirm_sup"][1]) == 11
    assert len(_lib.SYMBOLS["fm_loss_fedirm_rel"][1]) == 14 and len(_lib.SYMBOLS["fm_step_fedlsr"][1]) == 9
    assert _lib.SYMBOLS["fm_teacher_ema_params"][1] == [C.c_void_p, C.c_double]
    lib = _lib.load()                                          # the built library: loads without a GPU
    for name in NEW:
        assert hasattr(lib, name), f"{name} is not exported by {_lib.LIB_PATH}"
    from fedmlp_amd.engine import Engine
    from fedmlp_amd.local_training import LocalUpdate
    for m in ("loss_fedlsr", "loss_fedirm_sup", "loss_fedirm_rel", "step_fedlsr", "teacher_ema_params"):
        assert callable(getattr(Engine, m))
    assert callable(LocalUpdate.train_FedLSR) and callable(LocalUpdate.train_FedIRM)


def test_driver_parser_takes_the_new_methods():
    from fedmlp_amd import driver
    a = driver.args_parser(["--exp", "FedLSR"])
    assert a.exp == "FedLSR" and a.t_w == 40
    a = driver.args_parser(["--exp", "FedIRM"])
    assert (a.exp, a.rounds_FedIRM_sup, a.consistency, a.consistency_rampup, a.ema_decay) == ("FedIRM", 20, 1, 30, 0.99)
    a = driver.args_parser(["--exp", "FedIRM", "--rounds_FedIRM_sup", "1", "--ema_decay", "0.9", "--t_w", "3"])
    assert (a.rounds_FedIRM_sup, a.ema_decay, a.t_w) == (1, 0.9, 3)
    with pytest.raises(SystemExit):
        driver.args_parser(["--exp", "RoFL"])


def test_schedules_of_train_fedirm():
    """alpha = min(1 - 1 / (step + 1), ema_decay) over the persistent iter_num; cw = consistency * sigmoid_rampup(rnd, rampup)"""
    from fedmlp_amd.local_training import LocalUpdate
    assert [LocalUpdate.ema_alpha(s, 0.99) for s in (0, 1, 3, 98, 99, 100, 5000)] == \
        [0.0, 0.5, 0.75, 1 - 1 / 99, 0.99, 0.99, 0.99]
    assert LocalUpdate.sigmoid_rampup(5, 0) == 1.0
    assert LocalUpdate.sigmoid_rampup(0, 30) == float(np.exp(-5.0))
    assert LocalUpdate.sigmoid_rampup(30, 30) == 1.0 and LocalUpdate.sigmoid_rampup(45, 30) == 1.0
    assert LocalUpdate.sigmoid_rampup(15, 30) == float(np.exp(-5.0 * 0.25))


def test_gradients_of_the_restatement_against_finite_differences():
    """the float64 autograd gradients of the three heads against central differences of their own loss values"""
    rs = np.random.RandomState(5)
    B, Cn = 4, 5
    z = rs.uniform(-3, 3, (2 * B, Cn))
    z[:B] = np.where(z[:B] >= 0, 1.0, -1.0) * rs.uniform(2.5, 4.0, (B, Cn))        # every row selected (5 H(sigmoid 2.5) < 2)
    zt, y = rs.uniform(-3, 3, (B, Cn)), (rs.rand(B, Cn) < 0.4).astype(np.float64)
    pw, act = rs.uniform(0.5, 4, Cn), [1, 0, 1, 1, 0]
    target = 1 / (1 + np.exp(-rs.standard_normal((Cn, Cn))))
    heads = {
        "fedlsr": lambda zz: R.loss_fedlsr(zz, y, pw, 0.3, 0.4)[:2],
        "sup": lambda zz: R.loss_fedirm_sup(zz, y, pw, act, 3, 8)[:2],
        "rel": lambda zz: R.loss_fedirm_rel(zz, zt, y, pw, act, 3, 8, 0.7, target)[:2],
    }
    assert R.loss_fedirm_rel(z, zt, y, pw, act, 3, 8, 0.7, target)[3] == B
    h = 1e-6
    for name, f in heads.items():
        _, dz = f(z)
        for (r, c) in [(0, 0), (1, 3), (B - 1, 4), (B, 1), (2 * B - 1, 2)]:
            zp, zm = z.copy(), z.copy()
            zp[r, c] += h
            zm[r, c] -= h
            fd = (f(zp)[0] - f(zm)[0]) / (2 * h)
            assert abs(fd - dz[r, c]) <= 1e-7 * max(1.0, abs(fd)), (name, r, c, fd, dz[r, c])


def test_torch_fp32_chain_is_nan_where_p_rounds_to_one_and_the_rational_form_is_not():
    """the one stated deviation of fm_loss_fedlsr, confirmed on the CPU: with both logits at 20 the fp32 sigmoid is exactly 1,
    log(p / (1 - p)) is inf and its backward forms 0 * inf; p^2 / (p^2 + (1 - p)^2) gives a finite loss and zero slope there"""
    z = np.array([[20.0, 1.0], [30.0, -2.0]])                  # B = 1, C = 2: element 0 saturates in both views
    y, pw = np.array([[1.0, 0.0]]), np.array([2.0, 1.0])
    loss, dz = R.loss_fedlsr(z, y, pw, 0.3, 0.4, dtype=torch.float32)
    assert np.isnan(dz).any()
    loss, dz = R.loss_fedlsr(z, y, pw, 0.3, 0.4, dtype=torch.float32, rational=True)
    assert np.isfinite(loss) and np.isfinite(dz).all()
    # and the two forms are one function: equal to float64 rounding where nothing saturates
    zs = np.random.RandomState(2).uniform(-8, 8, (12, 5))
    ys = (np.random.RandomState(3).rand(6, 5) < 0.4).astype(np.float64)
    a = R.loss_fedlsr(zs, ys, np.ones(5), 0.6, 0.4)
    b = R.loss_fedlsr(zs, ys, np.ones(5), 0.6, 0.4, rational=True)
    assert abs(a[0] - b[0]) < 1e-12 and np.abs(a[1] - b[1]).max() < 1e-10
