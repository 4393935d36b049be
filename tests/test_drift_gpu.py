"""Client-drift correction on a real MI355X (include/fedmlp_hip_drift.h, fedmlp_amd/csrc/drift.hip, fedmlp_amd/drift.py): the launch
in front of every optimizer step against tests/drift_ref.py, element for element, over the engines' full arenas (ResNet-18
11.2 M floats, EfficientNet-B0 4 M with its padded channels) at tests/test_optim_gpu.py's shapes: 5 classes (fc.bias, 5 floats, and
fc.weight, 2 560, sit at odd element offsets), 32 x 32 input, batch 4, EfficientNet draws off.

Everything is compared in net.grads() layout (flat, state_dict order, zeros at the BatchNorm running statistics).  To give the
proximal term something to do, a test installs the correction at one model (the anchor) and then loads another one: fm_set_state
leaves the anchor alone."""
import ctypes as C

import numpy as np
import pytest
import torch

from fedmlp_amd import _lib, spec
from fedmlp_amd.drift import drift_active, drift_begin, drift_end, drift_last
from fedmlp_amd.engine import Engine
from fedmlp_amd.model import ResidentNet
from fedmlp_amd.optim import Adam
from tests import drift_ref as R
from tests.test_optim_gpu import _adamw_ref, _backward, _batch, _excess, _f32, _sgd_ref, _trainable, _weights

pytestmark = pytest.mark.gpu

C_, HW, B = 5, 32, 4
MODELS = ["Resnet18", "Efficient_b0"]
MU = 0.1
SEED_ANCHOR, SEED_MODEL = 7, 1037


def _entries(model):
    return spec.entries(model, C_)


def _params(model):
    return [i for i, (k, _, dt) in enumerate(_entries(model)) if dt == "f32" and spec.is_trainable(k)]


def _flags(model, on):
    on = set(on)
    return [int(i in on) for i in range(len(_entries(model)))]


def _flat_mask(model, idx):
    """bool [nf]: the flat positions of the given state entries"""
    m, off, idx = torch.zeros(spec.sizes(model, C_)[0], dtype=torch.bool), 0, set(idx)
    for i, (k, shape, dt) in enumerate(_entries(model)):
        if dt != "f32":
            continue
        n = int(np.prod(shape))
        if i in idx:
            m[off:off + n] = True
        off += n
    return m


class _Lines:
    """Engines by (model, slot), put back on every get(): the model's initial state, a fresh optimizer, nothing installed, the
    default mask, no group table."""

    def __init__(self):
        self.engines = {}

    def get(self, model, slot=0, seed=SEED_MODEL):
        eng = self.engines.get((model, slot))
        if eng is None:
            eng = self.engines[(model, slot)] = Engine(model, C_, HW, HW, B)
            eng.stochastic = False
        if drift_active(eng):
            drift_end(eng, mean=False)
        flat, cnt = spec.init_state(model, C_, seed)
        eng.set_state(flat, cnt)
        eng.adam_reset(1e-3, (0.9, 0.999), 1e-8, 5e-4)
        eng.zero_grad()
        eng.set_trainable(_flags(model, _params(model)))
        eng.optim_groups(None, 0)
        eng._grad_owner, eng._frozen_keys, eng._groups_key = None, frozenset(), None
        return eng, ResidentNet(eng).train()

    def close(self):
        for eng in self.engines.values():
            eng.close()
        self.engines.clear()


@pytest.fixture(scope="module")
def lines():
    ln = _Lines()
    yield ln
    ln.close()


def _shift(eng, seed=50, scale=1e-3):
    g = torch.Generator().manual_seed(seed)
    return (scale * torch.randn(eng.nf, generator=g)).cuda()


def _install(eng, model, mu, shift, track):
    """install at the anchor model, then load the model the step runs from -> (anchor, weights) flat fp32 numpy"""
    a, cnt = spec.init_state(model, C_, SEED_ANCHOR)
    eng.set_state(a, cnt)
    drift_begin(eng, mu=mu, shift=shift, track=track)
    p, cnt = spec.init_state(model, C_, SEED_MODEL)
    eng.set_state(p, cnt)
    return np.asarray(a, np.float32), np.asarray(p, np.float32)


def _snap(eng):
    step, m, v = eng.optim_state()
    return {"w": eng.state_tensor().clone(), "m": m, "v": v, "step": step, "cnt": eng.counters().copy()}


def _same_snap(a, b):
    assert a["step"] == b["step"] and np.array_equal(a["cnt"], b["cnt"])
    for k in ("w", "m", "v"):
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), k


ADAM = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=5e-4)
ADAMW = dict(ADAM, weight_decay=1e-2)
SGD = dict(lr=1e-2, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False)
GROUPS = [dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2),
          dict(lr=1e-4, betas=(0.8, 0.99), eps=1e-8, weight_decay=0.0),
          dict(lr=1e-2, betas=(0.95, 0.9), eps=1e-6, weight_decay=5e-2)]


def _adam_ref(p, g, m, v, step, hp):
    """torch.optim.Adam (coupled L2): the decay joins the gradient, then AdamW's update without decay"""
    return _adamw_ref(p, g + _f32(hp["weight_decay"]) * p, m, v, step, dict(hp, weight_decay=0.0))


def _aw(hp):
    return (hp["lr"], hp["betas"], hp["eps"], hp["weight_decay"])


# 1, 2 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("kind", ["sgd", "adam", "adamw", "adamw_groups"])
def test_rule_bits_and_the_optimizer_reads_them(lines, model, kind):
    """One forward and backward on the autograd path, one step with mu = 0.1, a random shift and track.  fm_drift_last is the
    reference rule applied to net.grads(), the weights read before the step, the anchor and the shift, element for element (as
    values: -0 == +0); net.grads() is unchanged by the step; the mean after exactly one step is the raw gradient.  The weights
    after the step meet torch's float64 formula evaluated on fm_drift_last within tests/test_optim_gpu.py's bound,
    4 ulp_fp32(|want|) + 1e-5 |want - old| (first step after a reset: zero moments)."""
    eng, net = lines.get(model)
    s = _shift(eng)
    a, p0 = _install(eng, model, MU, s, True)
    _backward(net, None, 100)
    tr = _trainable(model)
    g = eng.grads()
    pre = eng.get_state()[0]                        # the forward moved the BatchNorm running statistics, nothing else
    assert np.array_equal(pre[tr.numpy()], p0[tr.numpy()])
    params = _params(model)
    members = [[i for j, i in enumerate(params) if j % 3 == k] for k in range(3)]
    if kind == "sgd":
        eng.sgd_step(*[SGD[k] for k in ("lr", "momentum", "dampening", "weight_decay", "nesterov")])
    elif kind == "adam":
        eng.adam_step(*_aw(ADAM))
    elif kind == "adamw":
        eng.adamw_step(*_aw(ADAMW))
    else:
        of = [-1] * len(_entries(model))
        for j, i in enumerate(params):
            of[i] = j % 3
        eng.optim_groups(of, 3)
        eng.adamw_step_groups([_aw(h) for h in GROUPS])
    last = drift_last(eng)
    assert torch.equal(eng.grads().view(torch.int32), g.view(torch.int32)), "the step wrote the raw gradient"
    mean, K = drift_end(eng)
    assert K == 1 and not drift_active(eng)
    g_h, last_h, s_h = g.cpu().numpy(), last.cpu().numpy(), s.cpu().numpy()
    want = R.correct(g_h, p0, a, MU, s_h)
    trn = tr.numpy()
    bad = (last_h != want) & trn
    assert not bad.any(), f"{int(bad.sum())} corrected gradients differ from the reference rule"
    assert not last_h[~trn].any() and not mean.cpu().numpy()[~trn].any()
    assert np.array_equal(mean.cpu().numpy()[trn], g_h[trn]), "the mean of one step is not the raw gradient"
    assert int(((last_h != g_h) & trn).sum()) > 0.9 * int(trn.sum()), "the correction corrected nothing"
    # the optimizer consumed the corrected gradient
    p1 = torch.from_numpy(eng.get_state()[0])
    p64, r64 = torch.from_numpy(p0).double(), last.cpu().double()
    z = torch.zeros_like(p64)
    if kind == "sgd":
        want_p, _ = _sgd_ref(p64, r64, z, 0, SGD)
    elif kind == "adam":
        want_p, _, _ = _adam_ref(p64, r64, z, z, 0, ADAM)
    elif kind == "adamw":
        want_p, _, _ = _adamw_ref(p64, r64, z, z, 0, ADAMW)
    else:
        want_p = p64.clone()
        for k, hp in enumerate(GROUPS):
            sel = _flat_mask(model, members[k])
            want_p[sel] = _adamw_ref(p64[sel], r64[sel], z[sel], z[sel], 0, hp)[0]
    assert torch.equal(p1[~tr], torch.from_numpy(pre)[~tr]), "the step moved BN running statistics"
    assert float((p1[tr].double() - p64[tr]).abs().max()) > 0
    worst = _excess(p1[tr], want_p[tr], p64[tr])
    print(f"\n[drift] {model} {kind}: weights after the step, max error / bound {worst:.3f}")
    assert worst <= 1.0, worst


# 3 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
def test_fused_step(lines, model):
    """One fm_step_bce with the install active: fm_drift_last is the rule applied to the mean fm_drift_end returns (K = 1: the raw
    gradient), the weights before the step, the anchor and the shift.  A twin that runs the same step under mu = 0, a zero shift
    and track ends with the weights, moments and step count of an engine with nothing installed."""
    x, y = _batch(300)
    pw = [1.0 + 0.5 * c for c in range(C_)]
    loss = torch.zeros(1, device="cuda")
    eng, _ = lines.get(model)
    s = _shift(eng, 51)
    a, p0 = _install(eng, model, MU, s, True)
    eng.step_bce(x, y, pw, B, loss)
    last = drift_last(eng).cpu().numpy()
    mean, K = drift_end(eng)
    assert K == 1 and np.isfinite(float(loss))
    trn = _trainable(model).numpy()
    g = mean.cpu().numpy()
    assert float(np.abs(g[trn]).max()) > 0
    want = R.correct(g, p0, a, MU, s.cpu().numpy())
    assert not ((last != want) & trn).any() and not last[~trn].any()
    moved = _snap(eng)
    # the twin and the plain engine
    eng, _ = lines.get(model)
    eng.step_bce(x, y, pw, B, loss)
    plain = _snap(eng)
    eng2, _ = lines.get(model, 1)
    drift_begin(eng2, mu=0.0, shift=torch.zeros(eng2.nf, device="cuda"), track=True)
    eng2.step_bce(x, y, pw, B, loss)
    twin_mean, K = drift_end(eng2)
    assert K == 1
    _same_snap(_snap(eng2), plain)
    assert not torch.equal(moved["w"], plain["w"]), "mu and the shift changed nothing"
    # ... and the twin's mean is the gradient the plain step's Adam read, which the first run saw at other weights
    assert float(twin_mean.abs().max()) > 0


# 4 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
def test_launch_only_while_installed(lines, model):
    eng, net = lines.get(model)
    x, y = _batch(310)
    loss = torch.zeros(1, device="cuda")
    pw = [1.0] * C_

    def count(fn):
        eng.profile_ops(True, read=True)
        fn()
        rows = eng.profile_ops(False, read=True)
        return sum(n for lab, n, _ in rows if lab.startswith("drift_correct"))

    def two_fused_one_autograd():
        eng.step_bce(x, y, pw, B, loss)
        eng.step_bce(x, y, pw, B, loss)
        _backward(net, None, 311)
        eng.adamw_step(*_aw(ADAMW))

    assert count(two_fused_one_autograd) == 0
    drift_begin(eng, mu=MU)
    assert drift_active(eng)
    assert count(two_fused_one_autograd) == 3
    _, K = drift_end(eng)
    assert K == 3
    assert count(two_fused_one_autograd) == 0


# 5 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
def test_mask(lines, model):
    """Every other parameter frozen (adjacent entries alternate), the accumulator filled under the default mask so that the frozen
    entries' raw gradients are NOT zero: their corrected gradient and their mean are exact zeros and their weights do not move;
    the trainable entries carry the flat form's bits."""
    params = _params(model)
    on = [i for j, i in enumerate(params) if j % 2 == 0]
    off = [i for j, i in enumerate(params) if j % 2 == 1]
    m_on, m_off = _flat_mask(model, on).numpy(), _flat_mask(model, off).numpy()
    res = {}
    for form in ("flat", "masked"):
        eng, net = lines.get(model)
        s = _shift(eng, 52)
        a, p0 = _install(eng, model, MU, s, True)
        _backward(net, None, 320)
        g = eng.grads().cpu().numpy()
        eng.optim_groups([0 if i in set(params) else -1 for i in range(len(_entries(model)))], 1)
        if form == "masked":
            eng.set_trainable(_flags(model, on))
        eng.sgd_step_groups([(1e-2, 0.0, 0.0, 0.0, False)])
        last = drift_last(eng).cpu().numpy()
        mean, K = drift_end(eng)
        res[form] = (last, mean.cpu().numpy(), eng.get_state()[0])
        assert K == 1
    assert float(np.abs(g[m_off]).max()) > 0
    (lf, mf, pf), (lm, mm, pm) = res["flat"], res["masked"]
    assert not lm[m_off].any() and not mm[m_off].any(), "a frozen entry has a corrected gradient or a sum"
    assert np.array_equal(lm[m_on].view(np.int32), lf[m_on].view(np.int32))
    assert np.array_equal(mm[m_on].view(np.int32), mf[m_on].view(np.int32))
    assert np.array_equal(lf[m_on | m_off], R.correct(g, p0, a, MU, s.cpu().numpy())[m_on | m_off])
    assert np.array_equal(pm[m_off], p0[m_off]), "a frozen weight moved"
    assert np.array_equal(pm[m_on], pf[m_on]) and int((pm[m_on] != p0[m_on]).sum()) > 0


# 6 ------------------------------------------------------------------------------------------------------------------------
def test_padding_stays_zero(lines):
    """EfficientNet-B0: three corrected Adam steps (mu, a random shift, track); then weights and moments through state_dict() into a
    FRESH engine, whose padding is zero by construction; one more identical step on both gives the same bits
    (tests/test_optim_gpu.py::test_padding_stays_zero's method)."""
    model = "Efficient_b0"
    eng, net = lines.get(model)
    opt = Adam(net, lr=1e-3, weight_decay=5e-4)
    drift_begin(eng, mu=MU, shift=_shift(eng, 53, 1e-2), track=True)
    for it in range(3):
        _backward(net, opt, 330 + it)
        opt.step()
    _, K = drift_end(eng)
    assert K == 3
    eng2 = Engine(model, C_, HW, HW, B)
    try:
        eng2.stochastic = False
        net2 = ResidentNet(eng2).train()
        opt2 = Adam(net2, lr=1e-3, weight_decay=5e-4)
        net2.load_state_dict(net.state_dict())
        opt2.load_state_dict(opt.state_dict())
        for n_, o_ in ((net, opt), (net2, opt2)):
            _backward(n_, o_, 340)
            o_.step()
        pa, ca = _weights(net)
        pb, cb = _weights(net2)
        assert torch.equal(pa, pb), f"weights differ at {int((pa != pb).sum())} positions"
        assert torch.equal(ca, cb)
        sa, sb = opt.state_dict()["state"], opt2.state_dict()["state"]
        assert sa["step"] == sb["step"] == 4
        for k in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(sa[k], sb[k]), k
    finally:
        eng2.close()


# 7 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
def test_scaffold_identity(lines, model):
    """K = 3 plain SGD steps (lr eta, no momentum, no decay) under a shift s: (x - y) / (K eta) = mean(g) + s, per element within
    K ulp_fp32(max |p|) / (K eta): each of the K weight updates is rounded once to fp32, at most one ulp of the largest weight."""
    K, eta = 3, _f32(1e-2)
    eng, net = lines.get(model)
    s = _shift(eng, 54, 1e-2)
    drift_begin(eng, mu=0.0, shift=s, track=True)
    x = eng.get_state()[0].astype(np.float64)
    for it in range(K):
        _backward(net, None, 350 + it)
        eng.sgd_step(1e-2)
    mean, steps = drift_end(eng)
    y = eng.get_state()[0].astype(np.float64)
    assert steps == K
    trn = _trainable(model).numpy()
    pmax = np.float32(max(np.abs(x[trn]).max(), np.abs(y[trn]).max()))
    ulp = float(np.nextafter(pmax, np.float32(np.inf)) - pmax)
    bound = K * ulp / (K * eta)
    got = (x - y) / (K * eta)
    want = mean.cpu().numpy().astype(np.float64) + s.cpu().numpy().astype(np.float64)
    err = float(np.abs(got - want)[trn].max())
    print(f"\n[drift] {model} SCAFFOLD identity: max |(x - y)/(K eta) - (mean g + s)| {err:.3e}, bound {bound:.3e}")
    assert float(np.abs(want[trn]).max()) > 100 * bound and err <= bound


# 8 ------------------------------------------------------------------------------------------------------------------------
def test_refusals(lines):
    model = "Resnet18"
    eng, net = lines.get(model)
    _backward(net, None, 360)
    eng.adamw_step(*_aw(ADAMW))                     # non-zero moments, step count 1
    lib, h = eng.lib, eng.h
    buf = torch.zeros(eng.nf, device="cuda")
    ptr = buf.data_ptr()
    def refused(fn, *args, text):
        before = _snap(eng)
        active = drift_active(eng)
        rc = fn(h, *args)
        msg = lib.fm_last_error().decode()
        assert rc == -1 and text in msg, (rc, msg)              # FM_ERR_ARG
        with pytest.raises(_lib.FmError):
            _lib.check(rc)
        eng.sync()
        _same_snap(_snap(eng), before)
        assert drift_active(eng) == active

    refused(lib.fm_drift_end, None, None, text="no correction is installed")
    for mu in (-0.1, float("nan"), float("inf")):
        refused(lib.fm_drift_begin, C.c_float(mu), None, 1, text="mu must be finite and >= 0")
    refused(lib.fm_drift_begin, C.c_float(0.0), None, 0, text="nothing to install")
    assert not drift_active(eng)
    drift_begin(eng, mu=MU)
    refused(lib.fm_drift_begin, C.c_float(MU), None, 0, text="already installed")
    refused(lib.fm_drift_last, C.c_void_p(ptr), text="no optimizer step since fm_drift_begin")
    # the optimizer resets leave the install alone
    eng.adam_reset(1e-3)
    assert drift_active(eng)
    mean, K = drift_end(eng)
    assert K == 0 and not mean.any()
    with pytest.raises(ValueError):
        drift_begin(eng, mu=MU, shift=torch.zeros(eng.nf - 4, device="cuda"))
    assert not drift_active(eng)
