"""Kernel-level parity of the FedLSR / FedIRM loss heads (csrc/heads.hip: k_loss_fedlsr, k_loss_fedirm_sup, k_loss_fedirm_rel) through
Engine.loss_fedlsr / loss_fedirm_sup / loss_fedirm_rel, against the float64 restatement tests/irm_lsr_ref.py (pinned to the
reference's own functions by tests/test_irm_lsr_cpu.py).

Bound.  tests/test_head_kernels_gpu.py propagates (value, error) pairs operation by operation with u = 2^-24 and expf / logf /
log1pf ASSUMED within 2 ulp.  For these heads that propagation is impractical: FedLSR's log(p / (1 - p)) chain and FedIRM's kd
gradient, which reaches every selected logit through a C x C matrix of sigmoids of quotients of sums.  So the yardstick is
MEASURED, per tensor and per case, on the same inputs: d = max |torch-CPU fp32 autograd - float64 restatement| (the same torch
code in the two dtypes), and the kernel is allowed 4 d: a different operation order, plus the device libm's assumed 2 ulp
against the host's.  One floor from the number format: no fp32 result can be expected nearer than u max|tensor| (half an ulp
of its largest element), so d is taken as at least that; it matters where torch's single scalar loss happens to round well.
The inputs are checked first to keep the fp32 reference itself finite and every discrete decision (0.7 / 0.3 / 0.5 / 2.0 / the
1e-6 clamp) away from its threshold by more than fp32 rounding, so that both dtypes and the kernel decide alike.  Measured
distances and worst ratios go to irm_lsr_parity.json.

Logits: the smooth band of tests/test_head_kernels_gpu.py (|z| <= 8).  Saturated band (|z| in [20, 80], FedLSR): torch's fp32 chain
is NaN there (tests/test_irm_lsr_cpu.py shows it on the CPU); the kernel's stated deviation is that loss and every dz are finite."""
import numpy as np
import pytest
import torch

from tests import irm_lsr_ref as R
from tests.test_local_training_gpu import _dump

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
REPORT = {}
SHAPES = [(B, C) for B in (1, 3, 64, 67) for C in (5, 8, 14)]     # one-row sums; 67: past a wave, a multiple of nothing
_ENG = {}


@pytest.fixture(scope="module")
def engines():
    """a handle per class count (the heads take C from the handle); it owns the stream the launches run on, nothing else"""
    from fedmlp_amd import spec
    from fedmlp_amd.engine import Engine

    def get(C):
        if C not in _ENG:
            e = Engine("Resnet18", C, 32, 32, 4)
            e.set_state(*spec.init_state("Resnet18", C, 3))
            _ENG[C] = e
        return _ENG[C]
    yield get
    for e in _ENG.values():
        e.close()
    _ENG.clear()


def _f32(a):
    return np.asarray(a, np.float32).astype(np.float64)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def _labels(rs, B, C):
    y = (rs.rand(B, C) < 0.4).astype(np.float64)
    y[:, 1] = 0.0                                 # an all-zero class column: the + 1e-8 denominator
    return y


def _pw(rs, C):
    pw = rs.choice([1.0, 0.05, 37.5], C)
    pw[:3] = [1.0, 0.05, 37.5]
    return _f32(pw)


def _smooth(rs, shape):
    """|z| <= 8, fp32 numbers, every element at least 1e-3 in z from the logits of 0.7 / 0.3 / 0.5 and from the 1e-6 clamp of
    sigmoid(3 z) (z = -4.605); an element that lands nearer is moved by 4e-3"""
    z = rs.uniform(-8, 8, shape)
    for t in (0.0, np.log(0.7 / 0.3), -np.log(0.7 / 0.3), np.log(1e-6 / (1 - 1e-6)) / 3):
        z = np.where(np.abs(z - t) < 2e-3, t + 4e-3, z)
    return _f32(z)


def _within(name, got, want, f32):
    """the module docstring's bound; records d and the ratio"""
    got, want, f32 = (np.asarray(a, np.float64) for a in (got, want, f32))
    assert got.shape == want.shape == f32.shape, (name, got.shape, want.shape)
    assert np.isfinite(f32).all(), f"{name}: the fp32 reference is not finite on these inputs"
    assert np.isfinite(got).all(), f"{name}: not finite (an element was not written?)"
    d = max(float(np.abs(f32 - want).max()), U * float(np.abs(want).max()))
    err = float(np.abs(got - want).max())
    ratio = err / (4 * d) if d > 0 else (0.0 if err == 0 else np.inf)
    key = name.split(" ")[0] + "/" + name.split(" ")[-1]
    r = REPORT.setdefault(key, {"torch_fp32_distance": 0.0, "max_abs_err": 0.0, "worst_err_over_bound": 0.0})
    r["torch_fp32_distance"] = max(r["torch_fp32_distance"], d)
    r["max_abs_err"] = max(r["max_abs_err"], err)
    r["worst_err_over_bound"] = max(r["worst_err_over_bound"], ratio)
    _dump(REPORT, "irm_lsr_parity.json")
    print(f"{name}: torch fp32 distance {d:.3e}, max|err| {err:.3e}, err / (4 d) {ratio:.3f}")
    assert err <= 4 * d, f"{name}: max|err| {err:.3e} beyond 4 x {d:.3e}"


def _bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("bc", SHAPES, ids=str)
def test_loss_fedlsr(engines, bc):
    B, C = bc
    eng = engines(C)
    rs = np.random.RandomState(1000 + 17 * B + C)
    z, y, pw = _smooth(rs, (2 * B, C)), _labels(rs, B, C), _pw(rs, C)
    for mix1, beta in ((float(np.float32(rs.beta(1, 1))), 0.4), (0.25, 0.125)):
        want = R.loss_fedlsr(z, y, pw, mix1, beta)
        f32 = R.loss_fedlsr(z, y, pw, mix1, beta, dtype=torch.float32)
        dz, loss = eng.loss_fedlsr(_dev(z), _dev(y), pw, mix1, beta)
        dz2, loss2 = eng.loss_fedlsr(_dev(z), _dev(y), pw, mix1, beta)
        assert np.array_equal(_bits(dz), _bits(dz2)) and np.array_equal(_bits(loss), _bits(loss2))     # run to run
        _within(f"fedlsr {bc} loss", loss.cpu().numpy()[0], want[0], f32[0])
        _within(f"fedlsr {bc} dz", dz.cpu().numpy(), want[1], f32[1])


@pytest.mark.parametrize("bc", SHAPES, ids=str)
def test_loss_fedlsr_saturated_is_finite(engines, bc):
    """|z| in [20, 80]: p rounds to 1 (or 1 - p does); the stated deviation from torch's NaN"""
    B, C = bc
    eng = engines(C)
    rs = np.random.RandomState(2000 + 17 * B + C)
    z = _f32(rs.uniform(20, 80, (2 * B, C)) * rs.choice([-1.0, 1.0], (2 * B, C)))
    z[0, 0], z[B, 0] = 25.0, 30.0                 # both views saturated high in one element, whatever the draw
    y, pw = _labels(rs, B, C), _pw(rs, C)
    dz, loss = eng.loss_fedlsr(_dev(z), _dev(y), pw, 0.3, 0.4)
    assert torch.isfinite(loss).all() and torch.isfinite(dz).all()
    assert abs(float(dz[0, 0])) < 1e-12 and abs(float(dz[B, 0])) < 1e-12      # the derivative tends to 0 there


def _active(C):
    return [float(c % 2) for c in range(C)]


@pytest.mark.parametrize("bc", SHAPES, ids=str)
def test_loss_fedirm_sup(engines, bc):
    B, C = bc
    eng = engines(C)
    rs = np.random.RandomState(3000 + 17 * B + C)
    z, y, pw, act = _smooth(rs, (2 * B, C)), _labels(rs, B, C), _pw(rs, C), _active(C)
    ann, bs = int(sum(act)), 32
    want = R.loss_fedirm_sup(z, y, pw, act, ann, bs)
    f32 = R.loss_fedirm_sup(z, y, pw, act, ann, bs, dtype=torch.float32)
    rel = torch.zeros((C, C), device="cuda")
    dz, loss = eng.loss_fedirm_sup(_dev(z), _dev(y), pw, act, ann, bs, rel)
    dz2, loss2 = eng.loss_fedirm_sup(_dev(z), _dev(y), pw, act, ann, bs)          # no accumulator: the same loss and gradient
    assert np.array_equal(_bits(dz), _bits(dz2)) and np.array_equal(_bits(loss), _bits(loss2))
    _within(f"fedirm_sup {bc} loss", loss.cpu().numpy()[0], want[0], f32[0])
    _within(f"fedirm_sup {bc} dz", dz.cpu().numpy(), want[1], f32[1])
    _within(f"fedirm_sup {bc} rel", rel.cpu().numpy(), want[2], f32[2])
    assert (rel.cpu().numpy()[1] == 0.5).all()                 # the class without positives: 0 / 1e-8
    # accumulation: a call on a used buffer adds what the same call leaves in a zeroed one, to the bit
    first = rel.clone()
    z_b = _smooth(rs, (2 * B, C))
    one = torch.zeros((C, C), device="cuda")
    eng.loss_fedirm_sup(_dev(z_b), _dev(y), pw, act, ann, bs, one)
    eng.loss_fedirm_sup(_dev(z_b), _dev(y), pw, act, ann, bs, rel)
    assert np.array_equal(_bits(rel), _bits(first + one))


def _rel_case(rs, B, C, kind):
    """view-1 logits per case: `mixed` the smooth band as drawn; `all`: magnitudes in [4, 8], so that every probability is beyond
    0.7 / 0.3 and C H(sigmoid 4) < 2 up to C = 14; `none`: logits near 0"""
    z = _smooth(rs, (2 * B, C))
    if kind == "all":
        z[:B] = _f32(np.where(z[:B] >= 0, 1.0, -1.0) * rs.uniform(4, 8, (B, C)))
    elif kind == "none":
        z[:B] = _f32(rs.uniform(0.05, 0.5, (B, C)) * rs.choice([-1.0, 1.0], (B, C)))
    return z


@pytest.mark.parametrize("kind", ["mixed", "all", "none"])
@pytest.mark.parametrize("bc", SHAPES, ids=str)
def test_loss_fedirm_rel(engines, bc, kind):
    B, C = bc
    eng = engines(C)
    rs = np.random.RandomState(4000 + 17 * B + C + {"mixed": 0, "all": 500, "none": 700}[kind])
    z = _rel_case(rs, B, C, kind)
    zt, y, pw, act = _smooth(rs, (B, C)), _labels(rs, B, C), _pw(rs, C), _active(C)
    target = _f32(1.0 / (1.0 + np.exp(-rs.standard_normal((C, C)))))
    ann, bs, cw = int(sum(act)), 32, float(np.float32(0.6))
    el, un = R.selection_margin(z[:B])
    assert el > 1e-4 and un > 1e-3, ("an input sits on a selection threshold", el, un)
    want = R.loss_fedirm_rel(z, zt, y, pw, act, ann, bs, cw, target)
    f32 = R.loss_fedirm_rel(z, zt, y, pw, act, ann, bs, cw, target, dtype=torch.float32)
    assert want[3] == f32[3] and {"all": want[3] == B, "none": want[3] == 0, "mixed": True}[kind], (kind, want[3], B)
    rel = torch.zeros((C, C), device="cuda")
    args = (_dev(z), _dev(zt), _dev(y), pw, act, ann, bs, cw, _dev(target))
    dz, loss = eng.loss_fedirm_rel(*args, rel)
    dz2, loss2 = eng.loss_fedirm_rel(*args)
    assert np.array_equal(_bits(dz), _bits(dz2)) and np.array_equal(_bits(loss), _bits(loss2))     # run to run
    name = f"fedirm_rel_{kind}"
    _within(f"{name} {bc} n_sel={want[3]} loss", loss.cpu().numpy()[0], want[0], f32[0])
    _within(f"{name} {bc} n_sel={want[3]} dz", dz.cpu().numpy(), want[1], f32[1])
    _within(f"{name} {bc} n_sel={want[3]} rel", rel.cpu().numpy(), want[2], f32[2])
    single = rel.clone()
    eng.loss_fedirm_rel(*args, rel)                            # accumulates: twice the single call, to the bit
    assert np.array_equal(_bits(rel), _bits(single + single))
