"""fedmlp_amd.optim's SGD / AdamW / Adam steps, gradient clipping and optimizer state on a real MI355X (fm_sgd_step,
fm_adamw_step, fm_grad_norm, fm_clip_grad_norm, fm_clip_grad_value, fm_optim_get_state / fm_optim_set_state) over the engines'
full arenas (ResNet-18 11.2 M floats, EfficientNet-B0 4 M) at the smallest input the models allow.

Every line of training here is an engine of its own with a ResidentNet on it: the optimizer state belongs to the engine, so
two lines that are compared step by step cannot share the process-wide engine cache.

Reference arithmetic: torch's single-tensor update formulas evaluated in float64 on the CPU from the weights, gradients and
optimizer state read before the step.  The hyper-parameters enter that formula as the C ABI carries them, rounded to fp32
(fm_sgd / fm_adam are float structs; 1 - beta and 1 - dampening are formed from the fp32 values): what is left between the two
sides is fp32 rounding and fma contraction of a handful of operations."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from fedmlp_amd import spec
from fedmlp_amd.engine import Engine
from fedmlp_amd.model import ResidentNet
from fedmlp_amd.optim import SGD, Adam, AdamW, clip_grad_norm_, clip_grad_value_

pytestmark = pytest.mark.gpu

C_, HW, B = 5, 32, 4
MODELS = ["Resnet18", "Efficient_b0"]
# the norm kernel's own constants (csrc/kernels.h): every thread of stage 1 adds GRAD_NORM_F4 = 8 squares per vector component
# in fp32 (k), its block folds the 256 threads in a fixed tree of GRAD_NORM_TREE = 10 fp32 levels (d: 2 over the components, 6
# over the lanes, 2 over the waves); everything after that is double
NORM_K, NORM_D = 8, 10
NORM_RTOL = (NORM_K + NORM_D + 2) * 2.0 ** -24


def _f32(v):
    return float(np.float32(v))


class _Lines:
    """Engines by (model, slot), made on first use with the model's initial state and closed with the module."""

    def __init__(self):
        self.engines = {}

    def get(self, model, slot=0, seed=1037):
        eng = self.engines.get((model, slot))
        if eng is None:
            eng = self.engines[(model, slot)] = Engine(model, C_, HW, HW, B)
            eng.stochastic = False           # EfficientNet-B0: no drop-connect / dropout draws (identity multipliers)
        flat, cnt = spec.init_state(model, C_, seed)
        eng.set_state(flat, cnt)
        eng.zero_grad()
        eng._grad_owner = None
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


_MASKS = {}


def _trainable(model):
    """bool [nf]: the trainable positions of the flat state_dict layout (everything but the BN running statistics)"""
    if model not in _MASKS:
        parts = [np.full(int(np.prod(shape)), spec.is_trainable(key)) for key, shape, dt in spec.entries(model, C_) if dt == "f32"]
        _MASKS[model] = torch.from_numpy(np.concatenate(parts))
    return _MASKS[model]


def _batch(seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((B, 3, HW, HW), generator=g)
    y = (torch.rand((B, C_), generator=g) < 0.4).float()
    return x.cuda(), y.cuda()


def _backward(net, opt, seed):
    """a fresh forward and backward of one batch into the (emptied) accumulator"""
    x, y = _batch(seed)
    opt.zero_grad() if opt is not None else net.zero_grad()
    f, z = net(x)
    (F.binary_cross_entropy_with_logits(z, y) + 1e-3 * f.pow(2).mean()).backward()


def _weights(net):
    """(flat fp32 [nf] in state_dict order, counters) from net.state_dict()"""
    sd = net.state_dict()
    fl = torch.cat([v.reshape(-1) for k, v in sd.items() if v.dtype == torch.float32])
    cn = torch.stack([v.reshape(()) for k, v in sd.items() if v.dtype == torch.int64])
    return fl, cn


def _grads(net):
    """net.grads() scattered into the flat [nf] layout (zeros at the running statistics), on the device"""
    g = torch.cat([v.reshape(-1) for v in net.grads().values()])
    m = _trainable(net.model).cuda()
    out = torch.zeros(m.numel(), device="cuda")
    out[m] = g
    return out


def _ulp(x64):
    """ulp_fp32(|x|) of float64 values, as float64"""
    a = x64.abs().float()
    return (torch.nextafter(a, torch.full_like(a, float("inf"))) - a).double()


def _excess(got, want, old):
    """max of |got - want| / (4 ulp_fp32(|want|) + 1e-5 |want - old|): the issue's bound holds when this is <= 1.  Where the
    bound is zero (want == old == 0) the two sides must be equal."""
    err = (got.double() - want).abs()
    bound = 4.0 * _ulp(want) + 1e-5 * (want - old).abs()
    return float((err / bound).max())


def _sgd_ref(p, g, buf, step, hp):
    lr, mom, damp, wd = _f32(hp["lr"]), _f32(hp["momentum"]), _f32(hp["dampening"]), _f32(hp["weight_decay"])
    g = g + wd * p
    if mom != 0:
        buf = g.clone() if step == 0 else mom * buf + (1.0 - damp) * g
        g = g + mom * buf if hp["nesterov"] else buf
    return p - lr * g, buf


def _adamw_ref(p, g, m, v, step, hp):
    lr, b1, b2 = _f32(hp["lr"]), _f32(hp["betas"][0]), _f32(hp["betas"][1])
    eps, wd, t = _f32(hp["eps"]), _f32(hp["weight_decay"]), step + 1
    p = p * (1.0 - lr * wd)
    m = b1 * m + (1.0 - b1) * g
    v = b2 * v + (1.0 - b2) * g * g
    bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
    return p - (lr / bc1) * m / (v.sqrt() / bc2 ** 0.5 + eps), m, v


SGD_CASES = {
    "sgd_plain": dict(lr=1e-2),
    "sgd_momentum_dampening": dict(lr=1e-2, momentum=0.9, dampening=0.1),
    "sgd_nesterov_wd": dict(lr=1e-2, momentum=0.9, nesterov=True, weight_decay=5e-4),
}


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("case", list(SGD_CASES) + ["adamw"])
def test_step_arithmetic(lines, model, case):
    """Three single steps, each checked against torch's formula in float64 from what was read before it: weights within
    4 ulp_fp32(|p|) + 1e-5 |dp|, the new optimizer state within the same bound on its own magnitude; BN running statistics and
    counters untouched by a step.
    Observed maxima of error / bound on an MI355X (1 = the bound), the same for ResNet-18 and EfficientNet-B0 to the digits shown:
      SGD, all three forms: p 0.125, momentum_buffer 0.125 (half an fp32 ulp against 4: the kernel rounds each stored value once)
      AdamW: p 0.182, exp_avg 0.125, exp_avg_sq 0.249
    A pure fp32 chain (torch's own arithmetic) misses the bound: SGD with momentum p 2.13, AdamW p 2.47 on ResNet-18, where the
    two terms of the buffer / exp_avg update cancel under a small p; the kernels form those sums in double."""
    eng, net = lines.get(model)
    tr = _trainable(model)
    if case == "adamw":
        opt = AdamW(net, lr=1e-3, weight_decay=1e-2)
    else:
        opt = SGD(net, **SGD_CASES[case])
    worst = {}
    for it in range(3):
        _backward(net, opt, 100 + it)
        p0, c0 = _weights(net)
        g = _grads(net).cpu().double()
        osd = opt.state_dict()["state"]
        hp = opt.param_groups[0]
        assert osd["step"] == it
        opt.step()
        p1, c1 = _weights(net)
        nsd = opt.state_dict()["state"]
        assert nsd["step"] == it + 1
        assert torch.equal(p1[~tr], p0[~tr]) and torch.equal(c1, c0), "a step moved BN running statistics / counters"
        p64 = p0.double()
        if case == "adamw":
            m0, v0 = osd["exp_avg"].cpu().double(), osd["exp_avg_sq"].cpu().double()
            want_p, want_m, want_v = _adamw_ref(p64, g, m0, v0, it, hp)
            state = {"exp_avg": (nsd["exp_avg"].cpu(), want_m, m0), "exp_avg_sq": (nsd["exp_avg_sq"].cpu(), want_v, v0)}
        else:
            b0 = osd["momentum_buffer"].cpu().double()
            want_p, want_b = _sgd_ref(p64, g, b0, it, hp)
            state = {"momentum_buffer": (nsd["momentum_buffer"].cpu(), want_b, b0)}
            if not hp["momentum"]:
                assert torch.equal(nsd["momentum_buffer"].cpu(), osd["momentum_buffer"].cpu()), "momentum 0 wrote the buffer"
        assert float((p1[tr].double() - p64[tr]).abs().max()) > 0, "the step changed nothing"
        worst["p"] = max(worst.get("p", 0.0), _excess(p1[tr], want_p[tr], p64[tr]))
        for k, (got, want, old) in state.items():
            assert torch.equal(got[~tr], torch.zeros_like(got[~tr])), f"{k}: non-zero at the BN running statistics"
            sel = tr & ((want != 0) | (old != 0) | (got != 0))
            if bool(sel.any()):
                worst[k] = max(worst.get(k, 0.0), _excess(got[sel], want[sel], old[sel]))
    print(f"\n[optim] {model} {case}: max error / bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert all(v <= 1.0 for v in worst.values()), worst


@pytest.mark.parametrize("model", MODELS)
def test_first_step_buffer_is_the_decayed_gradient(lines, model):
    """momentum 0.9, dampening 0.5: after ONE step the buffer is g + wd p, not (1 - dampening) of it (torch clones the gradient
    on the first step).  The kernel forms g + wd p in double and rounds it once, so the buffer is the correctly rounded fp32
    value of the sum: at most half an fp32 ulp from the float64 value (whose own rounding, 2^-53, is the slack term)."""
    eng, net = lines.get(model)
    opt = SGD(net, lr=1e-2, momentum=0.9, dampening=0.5, weight_decay=5e-4)
    _backward(net, opt, 7)
    p0, _ = _weights(net)
    g = _grads(net).cpu().double()
    opt.step()
    buf = opt.state_dict()["state"]["momentum_buffer"].cpu()
    want = g + _f32(5e-4) * p0.double()                  # the product of two fp32 values is exact in float64
    r = want.float()                                     # round to nearest even
    err = (buf.double() - want).abs()
    half = 0.5 * torch.maximum(_ulp(want), _ulp(r.double())) + 2.0 ** -52 * want.abs()
    tr = _trainable(model)
    assert bool((err <= half)[tr].all()), f"{int((err > half)[tr].sum())} buffer entries are not the rounded decayed gradient"
    assert float(buf[tr].abs().max()) > 0 and torch.equal(buf[~tr], torch.zeros_like(buf[~tr]))


@pytest.mark.parametrize("model", MODELS)
def test_grad_norm(lines, model):
    """clip_grad_norm_(net, 1e30) and Engine.grad_norm() against sqrt(sum g^2) of net.grads() in float64: relative error at
    most (k + d + 2) 2^-24 with the kernel's k = 8, d = 10; the same gradients give the same bits; a clip that does not bite
    leaves the gradients as they were.  EfficientNet-B0: the engine's channel padding does not enter.
    Observed relative error on an MI355X: ResNet-18 2.98e-8, EfficientNet-B0 9.6e-9 (bound 1.19e-6)."""
    eng, net = lines.get(model)
    _backward(net, None, 11)
    g0 = _grads(net)
    want = float(g0.double().cpu().pow(2).sum().sqrt())
    n1 = clip_grad_norm_(net, 1e30)
    n2 = eng.grad_norm()
    n3 = eng.grad_norm()
    assert n1.is_cuda and n1.dim() == 0 and n2.dim() == 0
    rel = abs(float(n1) - want) / want
    print(f"\n[optim] {model} grad norm {float(n1):.9g}, float64 {want:.9g}, relative error {rel:.3e} (bound {NORM_RTOL:.3e})")
    assert want > 0 and rel <= NORM_RTOL
    assert torch.equal(n1, n2) and torch.equal(n2, n3)
    assert torch.equal(_grads(net), g0)


@pytest.mark.parametrize("model", MODELS)
def test_clipping(lines, model):
    eng, net = lines.get(model)
    opt = SGD(net, lr=1e-2)
    _backward(net, opt, 13)
    g0 = _grads(net)
    norm = eng.grad_norm()
    n32 = np.float32(float(norm))
    # a clip that bites: one fp32 multiply by the coefficient formed in fp32
    max_norm = 0.5 * float(n32)
    ret = clip_grad_norm_(net, max_norm)
    coef = np.float32(max_norm) / (n32 + np.float32(1e-6))
    assert torch.equal(ret, norm), "the returned value is the norm before clipping"
    g1 = _grads(net)
    assert coef < 1 and torch.equal(g1.cpu(), g0.cpu() * float(coef))      # the product on the CPU: IEEE, denormals kept
    # one that does not: bitwise unchanged (the norm is now coef times what it was)
    ret = clip_grad_norm_(net, 2.0 * float(n32))
    assert torch.equal(_grads(net), g1) and abs(float(ret) - float(coef) * float(n32)) <= 1e-5 * float(n32)
    # by value: clamp
    v = float(g1.abs().max()) / 64.0
    clip_grad_value_(net, v)
    g2 = _grads(net)
    v32 = float(np.float32(v))
    assert torch.equal(g2, g1.clamp(-v32, v32)) and int((g2 != g1).sum()) > 0
    # an empty accumulator: norm 0, and a following step changes nothing
    opt.zero_grad()
    assert float(clip_grad_norm_(net, 1.0)) == 0.0 and float(eng.grad_norm()) == 0.0
    clip_grad_value_(net, 1.0)
    p0, c0 = _weights(net)
    opt.step()
    p1, c1 = _weights(net)
    assert torch.equal(p0, p1) and torch.equal(c0, c1)


def _load(line, net_sd, opt, opt_sd):
    eng, net = line
    net.load_state_dict(net_sd)
    opt.load_state_dict(opt_sd)


def _same_state(a, b):
    assert a["step"] == b["step"]
    for k in a:
        if k != "step":
            assert torch.equal(a[k], b[k]), f"{k} differs at {int((a[k] != b[k]).sum())} positions"


def test_padding_stays_zero(lines):
    """EfficientNet-B0 (channels padded to multiples of 16 inside the engine): three SGD steps with weight decay, three AdamW
    steps, then weights and moments through state_dict() into a FRESH engine, whose padding is zero by construction; one more
    identical step on both must give the same bits."""
    model = "Efficient_b0"
    eng, net = lines.get(model)
    opt = SGD(net, lr=1e-2, momentum=0.9, weight_decay=5e-4)
    for it in range(3):
        _backward(net, opt, 200 + it)
        opt.step()
    opt = AdamW(net, lr=1e-3, weight_decay=1e-2)
    for it in range(3):
        _backward(net, opt, 210 + it)
        opt.step()
    eng2 = Engine(model, C_, HW, HW, B)
    try:
        eng2.stochastic = False
        net2 = ResidentNet(eng2).train()
        opt2 = AdamW(net2, lr=1e-3, weight_decay=1e-2)
        _load((eng2, net2), net.state_dict(), opt2, opt.state_dict())
        for n_, o_ in ((net, opt), (net2, opt2)):
            _backward(n_, o_, 220)
            o_.step()
        pa, ca = _weights(net)
        pb, cb = _weights(net2)
        assert torch.equal(pa, pb), f"weights differ at {int((pa != pb).sum())} positions"
        assert torch.equal(ca, cb)
        _same_state(opt.state_dict()["state"], opt2.state_dict()["state"])
    finally:
        eng2.close()


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_optimizer_state_round_trip(lines, model, kind):
    def make(net):
        return Adam(net, lr=1e-3, weight_decay=5e-4) if kind == "adam" else SGD(net, lr=1e-2, momentum=0.9, dampening=0.1)

    line_a, line_b = lines.get(model, 0), lines.get(model, 1, seed=7)
    net, net2 = line_a[1], line_b[1]
    opt = make(net)
    for it in range(2):
        _backward(net, opt, 300 + it)
        opt.step()
    net_sd, opt_sd = net.state_dict(), opt.state_dict()
    assert opt_sd["state"]["step"] == 2
    opt2 = make(net2)
    _load(line_b, net_sd, opt2, opt_sd)
    _same_state(opt_sd["state"], opt2.state_dict()["state"])
    for n_, o_ in ((net, opt), (net2, opt2)):
        _backward(n_, o_, 302)
        o_.step()
    pa, ca = _weights(net)
    pb, cb = _weights(net2)
    assert torch.equal(pa, pb), f"weights differ at {int((pa != pb).sum())} positions"
    assert torch.equal(ca, cb)
    sa, sb = opt.state_dict()["state"], opt2.state_dict()["state"]
    assert sa["step"] == 3
    _same_state(sa, sb)
    # a tensor of the wrong length
    key = "exp_avg" if kind == "adam" else "momentum_buffer"
    bad = {"state": dict(opt_sd["state"]), "param_groups": opt_sd["param_groups"]}
    bad["state"][key] = bad["state"][key][:-4]
    with pytest.raises(ValueError):
        opt2.load_state_dict(bad)
    with pytest.raises(ValueError):
        line_b[0].set_optim_state(1, torch.zeros(line_b[0].nf - 4, device="cuda"))
