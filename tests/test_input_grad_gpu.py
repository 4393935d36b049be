"""d loss / d x of a train-mode net(x) on a real MI355X: the two stem data-gradient kernels (csrc/stem_dgrad.hip) against
torch's fp32 and float64 convolutions through fm_debug_conv, x.grad through autograd for ResNet-18 and EfficientNet-B0
(fp32 and bf16 storage) against the CPU oracles, accumulation, the recompute path, and that nothing else moved."""
import copy
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from fedmlp_amd import spec
from fedmlp_amd.model import HipNet
from tests.helpers import oracle_net, relu_masks_from_engine

pytestmark = pytest.mark.gpu

C_, HW, MAXI = 5, 64, 16
MODELS = [("Resnet18", "fp32"), ("Efficient_b0", "fp32"), ("Efficient_b0", "bf16")]
RECORD = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r08", "parity_input_grad.json")


def _net(model="Resnet18", precision="fp32", seed=1037, maxi=MAXI):
    flat, cnt = spec.init_state(model, C_, seed)
    net = HipNet(model, C_, flat, cnt)
    net.default_max_images, net.precision = maxi, precision
    return net.train()


def _x(B, seed, hw=HW):
    return torch.randn((B, 3, hw, hw), generator=torch.Generator().manual_seed(seed))


def _labels(B, seed):
    return (torch.rand((B, C_), generator=torch.Generator().manual_seed(seed)) < 0.4).float()


def _loss(f, z, y, act=(1, 3), lam=0.5):
    """masked BCE plus a feature term"""
    bce = F.binary_cross_entropy_with_logits(z, y.to(z.device).to(z.dtype), reduction="none")[:, list(act)].sum()
    return bce / (z.shape[0] * len(act)) + lam * f.pow(2).sum() / f.numel()


def _np(grads):
    return {k: v.cpu().numpy().copy() for k, v in grads.items()}


def _record(key, value):
    """profiles/r08/parity_input_grad.json: measured figures of the last run (best effort: a read-only tree is not a failure)"""
    try:
        rec = {}
        if os.path.isfile(RECORD):
            with open(RECORD) as f:
                rec = json.load(f)
        rec[key] = value
        os.makedirs(os.path.dirname(RECORD), exist_ok=True)
        with open(RECORD, "w") as f:
            json.dump(rec, f, indent=1, sort_keys=True)
    except OSError:
        pass


class _fixed_draws:
    """EfficientNet-B0: the engine's own draws off, the given drop-connect / dropout multipliers installed"""

    def __init__(self, net, B, seed=5):
        self.net, self.B, self.seed = net, B, seed

    def __enter__(self):
        self.eng = self.net.bind(HW, HW, MAXI)
        self.dc = self.dr = None
        if self.net.model == "Efficient_b0":
            from oracle.efficientnet_ref import draw_stochastic
            self.prev = self.eng.stochastic
            self.eng.stochastic = False
            self.dc, self.dr = draw_stochastic(self.B, torch.Generator().manual_seed(self.seed))
            self.eng.set_stochastic(self.dc.cuda(), self.dr.cuda())
        return self

    def __exit__(self, *exc):
        if self.net.model == "Efficient_b0":
            self.eng.stochastic = self.prev
            self.eng.set_stochastic(None, None)
        return False


# ---- 1. x.grad exists ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,precision", MODELS)
@pytest.mark.parametrize("where", ["cpu", "cuda"])
def test_x_grad_is_populated(model, precision, where):
    B = 4
    net = _net(model, precision)
    y = _labels(B, 2)
    x = _x(B, 1).to(where).requires_grad_(True)
    f, z = net(x)
    _loss(f, z, y).backward()
    assert x.grad is not None, "x.grad is None: the train-mode call did not differentiate with respect to its input"
    assert x.grad.shape == x.shape and x.grad.dtype == x.dtype and x.grad.device == x.device
    assert torch.isfinite(x.grad).all() and x.grad.abs().max() > 0
    # an x that does not require grad gets none
    x2 = _x(B, 1).to(where)
    f, z = net(x2)
    _loss(f, z, y).backward()
    assert x2.grad is None


@pytest.mark.parametrize("model,precision", MODELS)
def test_second_backward_adds_to_x_grad(model, precision):
    B = 4
    net = _net(model, precision)
    y = _labels(B, 4)
    with _fixed_draws(net, B):
        x = _x(B, 3).cuda().requires_grad_(True)
        f, z = net(x)
        _loss(f, z, y).backward()
        g1 = x.grad.clone()
        f, z = net(x)
        _loss(f, z, y, act=(0, 2), lam=0.1).backward()
        g12 = x.grad.clone()
        x.grad = None
        f, z = net(x)
        _loss(f, z, y, act=(0, 2), lam=0.1).backward()
        g2 = x.grad.clone()
    assert torch.equal(g12, g1 + g2)


def test_eval_mode_call_records_no_graph():
    net = _net().eval()
    x = _x(2, 5).cuda().requires_grad_(True)
    f, z = net(x)
    assert f.grad_fn is None and z.grad_fn is None


# ---- 2. the kernels against torch -------------------------------------------------------------------------------------
def _stem_dgrad_case(model, hw, imgs, seed):
    from fedmlp_amd.engine import Engine
    e = Engine(model, C_, hw, hw, max(imgs, 2))
    try:
        flat, cnt = spec.init_state(model, C_, 1037)
        e.set_state(flat, cnt)
        sd = spec.flat_to_state_dict(model, C_, flat, cnt)
        info = e.debug_conv_info(0)
        assert info["cin"] == 3
        res = model == "Resnet18"
        w = torch.from_numpy(np.asarray(sd["conv1.weight" if res else "_conv_stem.weight"]))
        g = torch.Generator().manual_seed(seed)
        dy = torch.randn((imgs, info["cout"], info["hout"], info["wout"]), generator=g)

        def conv(x, wt):
            if res:
                return F.conv2d(x, wt, None, 2, 3)
            return F.conv2d(F.pad(x, (0, 1, 0, 1)), wt, None, 2, 0)          # TF-"same" at even sizes: 0 top / left, 1 bottom / right

        def want_dx(dtype):
            x = torch.zeros((imgs, 3, hw, hw), dtype=dtype, requires_grad=True)
            conv(x, w.to(dtype)).backward(dy.to(dtype))
            return x.grad
        want32, want64 = want_dx(torch.float32), want_dx(torch.float64)
        dy_d = dy.permute(0, 2, 3, 1).contiguous()
        if info["cout_p"] > info["cout"]:
            dy_d = F.pad(dy_d, (0, info["cout_p"] - info["cout"]))
        dx = torch.full((imgs, hw, hw, 3), float("nan"), device=e.device)
        e.debug_conv(1, 0, None, dy_d.contiguous().to(e.device), dx, imgs)
        got = dx.cpu().permute(0, 3, 1, 2)
    finally:
        e.close()
    assert torch.isfinite(got).all(), f"{int((~torch.isfinite(got)).sum())} elements of dx were not written"
    l2 = float(torch.linalg.vector_norm(got.double() - want64) / torch.linalg.vector_norm(want64))
    print(f"stem dgrad {model} {hw}x{hw} imgs {imgs}: rel L2 vs float64 {l2:.3e}, "
          f"max abs vs fp32 {float((got - want32).abs().max()):.3e} of {float(want32.abs().max()):.3e}")
    scale = want32.abs().max().item()
    np.testing.assert_allclose(got.numpy(), want32.numpy(), rtol=1e-4, atol=2e-5 * scale)
    assert l2 < 2e-6, l2


@pytest.mark.parametrize("model", ["Resnet18", "Efficient_b0"])
@pytest.mark.parametrize("hw,imgs", [(64, 6), (64, 1), (224, 3)])
def test_stem_dgrad_kernel_against_torch(model, hw, imgs):
    """fm_debug_conv(op=1, conv=0) = the stem's input-gradient kernel with its NHWC store, dx pre-filled with NaN: against
    torch's fp32 conv backward at _check_conv's data-gradient bound and against the float64 one at 2e-6 relative L2."""
    _stem_dgrad_case(model, hw, imgs, 700 + hw + imgs)


# ---- 3. whole net against the oracle ----------------------------------------------------------------------------------
def _cmp_param_grads(got, ref, rtol=5e-5):
    bad = []
    for k, p in ref.named_parameters():
        want = p.grad.numpy() if p.grad is not None else np.zeros_like(got[k])
        err = float(np.abs(got[k] - want).max() / (np.abs(want).max() + 1e-12))
        if not err < rtol:
            bad.append(f"{k}: {err:.3e}")
    assert not bad, "grad rel-to-max errors: " + "; ".join(bad[-14:])


@pytest.mark.parametrize("hw,B", [(64, 6), (224, 2)])
def test_resnet_x_grad_against_oracle(hw, B):
    """x.grad of masked BCE + a feature term against the CPU oracle under the engine's discrete decisions (every ReLU mask,
    the stem's included, and the max-pool choices: one flipped stem decision moves a 7x7 patch of dx by percents of its max,
    which is a statement about the choice, not about the arithmetic).  Bound: the engine within max(5e-5, 3 * e_ref) of the
    float64 oracle's dx, e_ref = the fp32 oracle's own distance from it (max abs over max abs)."""
    net = _net(maxi=max(MAXI if hw == 64 else 4, B))
    eng = net.bind(hw, hw, net.default_max_images)
    ref = oracle_net(C_, 1037).train()
    y = _labels(B, 12)
    x = _x(B, 11, hw).requires_grad_(True)
    net.zero_grad()
    f, z = net(x)
    rm = relu_masks_from_engine(eng, 1, B, stem=True)
    _loss(f, z, y).backward()
    got_p, got_x = _np(net.grads()), x.grad.double().numpy()

    def oracle(dtype):
        r = copy.deepcopy(ref).to(dtype)
        xr = x.detach().to(dtype).requires_grad_(True)
        rm.calls = rm.flips = rm.pool_calls = rm.pool_flips = 0
        with rm:
            fr, zr = r(xr)
            _loss(fr, zr, y).backward()
        return r, xr.grad.double().numpy(), int(rm.flips)
    r32, dx32, flips = oracle(torch.float32)
    _, dx64, _ = oracle(torch.float64)
    top = np.abs(dx64).max()
    e_ref = float(np.abs(dx32 - dx64).max() / top)
    e_eng = float(np.abs(got_x - dx64).max() / top)
    bound = max(5e-5, 3 * e_ref)
    print(f"x.grad {hw}x{hw} B {B}: engine vs float64 {e_eng:.3e}, fp32 oracle vs float64 {e_ref:.3e}, bound {bound:.3e}, "
          f"flips {flips}")
    _record(f"resnet18_{hw}_B{B}", {"engine_vs_f64": e_eng, "oracle_f32_vs_f64": e_ref, "bound": bound, "mask_flips": flips,
                                    "pool_flips": int(rm.pool_flips)})
    assert flips <= 16, flips
    _cmp_param_grads(got_p, r32)
    assert e_eng <= bound, (e_eng, e_ref)


def _eff_x_grad(precision, x, y, dc, dr):
    net = _net("Efficient_b0", precision)
    eng = net.bind(HW, HW, MAXI)
    prev, eng.stochastic = eng.stochastic, False
    try:
        eng.set_stochastic(dc.cuda(), dr.cuda())
        xg = x.clone().cuda().requires_grad_(True)
        net.zero_grad()
        f, z = net(xg)
        _loss(f, z, y).backward()
        return xg.grad.cpu().double().numpy(), _np(net.grads())
    finally:
        eng.stochastic = prev
        eng.set_stochastic(None, None)


def test_effnet_x_grad_against_oracle():
    """EfficientNet-B0 fp32 with installed draws against oracle/efficientnet_ref.py: dx at 5e-4 of its max, the gradient
    bound of tests/test_effnet_gpu.py::_cmp_grads; bf16 storage against the fp32 ENGINE's dx at the per-tensor bounds
    tests/test_effnet_bf16_gpu.py::test_step_bce_bf16 holds for every gradient tensor (max abs error < 0.3 of the max,
    cosine > 0.95)."""
    from oracle.efficientnet_ref import EfficientNetB0Ref, draw_stochastic
    B = 6
    x, y = _x(B, 61), _labels(B, 62)
    dc, dr = draw_stochastic(B, torch.Generator().manual_seed(5))
    ref = EfficientNetB0Ref(C_)
    flat, cnt = spec.init_state("Efficient_b0", C_, 1037)
    sd = spec.flat_to_state_dict("Efficient_b0", C_, flat, cnt)
    ref.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    ref.train()
    xr = x.clone().requires_grad_(True)
    fr, zr = ref(xr, dc, dr)
    _loss(fr, zr, y).backward()
    want = xr.grad.double().numpy()
    got32, _ = _eff_x_grad("fp32", x, y, dc, dr)
    e32 = float(np.abs(got32 - want).max() / np.abs(want).max())
    got16, _ = _eff_x_grad("bf16", x, y, dc, dr)
    e16 = float(np.abs(got16 - got32).max() / np.abs(got32).max())
    cos = float(np.dot(got16.ravel(), got32.ravel()) / (np.linalg.norm(got16) * np.linalg.norm(got32)))
    print(f"EfficientNet-B0 x.grad: fp32 vs oracle {e32:.3e}; bf16 vs fp32 engine {e16:.3e}, cosine {cos:.5f}")
    _record("efficientnet_b0_64_B6", {"fp32_vs_oracle": e32, "bf16_vs_fp32_engine": e16, "bf16_cosine": cos})
    assert e32 < 5e-4, e32
    assert e16 < 0.3 and cos > 0.95, (e16, cos)


# ---- 4. nothing else moved ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,precision", MODELS)
def test_parameter_grads_are_bit_equal_with_and_without_dx(model, precision):
    B = 6
    net = _net(model, precision)
    y = _labels(B, 72)
    with _fixed_draws(net, B):
        out = []
        for want_dx in (False, True):
            x = _x(B, 71).cuda().requires_grad_(want_dx)
            net.zero_grad()
            f, z = net(x)
            _loss(f, z, y).backward()
            out.append(_np(net.grads()))
    for k in out[0]:
        assert np.array_equal(out[0][k], out[1][k]), k


# ---- 5. two calls, one backward -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,precision", MODELS)
def test_two_calls_one_backward_each_view_gets_its_own_gradient(model, precision):
    B = 4
    net = _net(model, precision)
    y = _labels(B, 83)
    with _fixed_draws(net, B):
        x1 = _x(B, 81).cuda().requires_grad_(True)
        x2 = _x(B, 82).cuda().requires_grad_(True)
        f1, z1 = net(x1)
        f2, z2 = net(x2)
        (_loss(f1, z1, y) + _loss(f2, z2, y, act=(0, 4), lam=0.2)).backward()      # node 2 direct, node 1 through a recompute
        g1, g2 = x1.grad.clone(), x2.grad.clone()
        assert not torch.equal(g1, g2)
        # each view alone, followed by a recompute (another call in between)
        a1 = _x(B, 81).cuda().requires_grad_(True)
        f, z = net(a1)
        net(x2.detach())
        _loss(f, z, y).backward()
        a2 = _x(B, 82).cuda().requires_grad_(True)
        f, z = net(a2)
        net(x1.detach())
        _loss(f, z, y, act=(0, 4), lam=0.2).backward()
    assert torch.equal(g1, a1.grad) and torch.equal(g2, a2.grad)


def test_engine_backward_grads_dx_pair():
    """Engine.backward_grads(dx=(dx1, dx2)) after a two-view forward: each view's gradient, either entry optional; a second
    pointer after a one-view forward is refused."""
    net = _net()
    eng = net.bind(HW, HW, MAXI)
    B = 3
    x1, x2 = _x(B, 91).cuda(), _x(B, 92).cuda()
    D = (0.1 * torch.randn((2 * B, C_), generator=torch.Generator().manual_seed(93))).cuda()
    eng.forward_train(x1, x2)
    d1, d2 = torch.full_like(x1, float("nan")), torch.full_like(x2, float("nan"))
    eng.backward_grads(D, None, dx=(d1, d2))
    assert torch.isfinite(d1).all() and torch.isfinite(d2).all()
    eng.forward_recompute(x1, x2)
    only2 = torch.full_like(x2, float("nan"))
    eng.backward_grads(D, None, dx=(None, only2))
    assert torch.equal(only2, d2)
    eng.forward_train(x1)
    with pytest.raises(Exception):
        eng.backward_grads(D[:B], None, dx=(d1, d2))
    with pytest.raises(ValueError):
        eng.backward_grads(D[:B], None, dx=torch.empty((B, 3, HW, HW)))
