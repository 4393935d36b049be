"""Frozen BatchNorm statistics for the differentiable train-mode net(x) (HipNet.freeze_bn, fm_bn_freeze) on a real MI355X:
nothing moves, the forward is eval-mode arithmetic, no image's gradient depends on another image, gradients against the CPU
oracles with their BatchNorm modules in eval(), the recompute path, the untouched default path, one fine-tuning step.

Every net starts from the PREPARED state: spec.init_state(model, 5, 1037) after three batch-statistics train-mode forwards,
so the running statistics differ from 0 / 1 and from any batch's statistics."""
import copy
import functools
import json
import os

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from fedmlp_amd import spec
from fedmlp_amd.model import HipNet
from fedmlp_amd.optim import Adam
from tests.helpers import relu_masks_from_engine

pytestmark = pytest.mark.gpu

C_, HW, MAXI = 5, 64, 16
LR, WD = 3e-5, 5e-4
MODELS = [("Resnet18", "fp32"), ("Efficient_b0", "fp32"), ("Efficient_b0", "bf16")]
RECORD = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r09", "parity_freeze_bn.json")


def _x(B, seed, hw=HW):
    return torch.randn((B, 3, hw, hw), generator=torch.Generator().manual_seed(seed))


def _labels(B, seed):
    return (torch.rand((B, C_), generator=torch.Generator().manual_seed(seed)) < 0.4).float()


def _loss(f, z, y, act=(1, 3), lam=0.5):
    """masked BCE plus a feature term (tests/test_input_grad_gpu.py's)"""
    bce = F.binary_cross_entropy_with_logits(z, y.to(z.device).to(z.dtype), reduction="none")[:, list(act)].sum()
    return bce / (z.shape[0] * len(act)) + lam * f.pow(2).sum() / f.numel()


def _np(grads):
    return {k: v.cpu().numpy().copy() for k, v in grads.items()}


def _record(key, value):
    """profiles/r09/parity_freeze_bn.json: measured figures of the last run (best effort: a read-only tree is not a failure)"""
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


class _draws:
    """The engine's own EfficientNet-B0 draws off; drop-connect / dropout multipliers of `seed` installed (None: none)"""

    def __init__(self, net, B, seed=5, hw=HW, maxi=MAXI):
        self.net, self.B, self.seed, self.hw, self.maxi = net, B, seed, hw, maxi

    def __enter__(self):
        self.eng = self.net.bind(self.hw, self.hw, self.maxi)
        self.dc = self.dr = None
        if self.net.model == "Efficient_b0":
            self.prev = self.eng.stochastic
            self.eng.stochastic = False
            if self.seed is not None:
                from oracle.efficientnet_ref import draw_stochastic
                self.dc, self.dr = draw_stochastic(self.B, torch.Generator().manual_seed(self.seed))
                self.eng.set_stochastic(self.dc.cuda(), self.dr.cuda())
            else:
                self.eng.set_stochastic(None, None)
        return self

    def __exit__(self, *exc):
        if self.net.model == "Efficient_b0":
            self.eng.stochastic = self.prev
            self.eng.set_stochastic(None, None)
        return False


def _hipnet(model, precision, flat, cnt, maxi=MAXI):
    net = HipNet(model, C_, flat.copy(), cnt.copy())
    net.default_max_images, net.precision = maxi, precision
    return net.train()


@functools.lru_cache(maxsize=None)
def _prepared(model, precision):
    """(flat, counters) of the prepared state, computed once per model and storage precision and never written to"""
    flat, cnt = spec.init_state(model, C_, 1037)
    net = _hipnet(model, precision, flat, cnt)
    with _draws(net, 6, seed=None), torch.no_grad():
        for i in range(3):
            net(_x(6, 901 + i))
    sd = net.state_dict()
    flat, cnt = spec.state_dict_to_flat(model, C_, sd)
    flat.setflags(write=False)
    cnt.setflags(write=False)
    return flat, cnt


def _net(model="Resnet18", precision="fp32", maxi=MAXI, state_of=None):
    """a fresh train-mode HipNet on the prepared state (state_of: the storage precision whose prepared state is taken)"""
    return _hipnet(model, precision, *_prepared(model, state_of or precision), maxi=maxi)


def _oracle(model, precision="fp32", frozen=True):
    """the CPU oracle on the prepared state: train mode, its BatchNorm modules in eval() (frozen) -- torch's idiom"""
    flat, cnt = _prepared(model, precision)
    sd = spec.flat_to_state_dict(model, C_, flat, cnt)
    if model == "Resnet18":
        from oracle.resnet18_ref import ResNet18Ref
        ref = ResNet18Ref(C_)
    else:
        from oracle.efficientnet_ref import EfficientNetB0Ref
        ref = EfficientNetB0Ref(C_)
    ref.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()})
    ref.train()
    if frozen:
        for m in ref.modules():
            if isinstance(m, nn.BatchNorm2d):
                m.eval()
    return ref


def _engine_stats(eng, model):
    """running statistics and counters as they are on the DEVICE now (a frozen call marks nothing dirty, so state_dict()
    would hand back the host copy)"""
    flat, cnt = eng.get_state()
    sd = spec.flat_to_state_dict(model, C_, flat, cnt)
    return {k: np.array(v) for k, v in sd.items() if "running_" in k or "num_batches" in k}


# ---- 1. nothing moves ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,precision", MODELS)
def test_running_statistics_and_counters_do_not_move(model, precision):
    B = 4
    net = _net(model, precision).freeze_bn()
    y = _labels(B, 2)
    with _draws(net, B) as d:
        eng = d.eng
        assert not eng.bn_frozen
        before = _engine_stats(eng, model)
        assert any(v.any() for k, v in before.items() if k.endswith("running_mean"))
        x = _x(B, 1).cuda().requires_grad_(True)
        f, z = net(x)
        assert f.grad_fn is not None and z.grad_fn is not None
        _loss(f, z, y).backward()
        assert x.grad is not None and torch.isfinite(x.grad).all() and x.grad.abs().max() > 0
        f1, z1 = net(x)                                          # ... and a second frozen forward whose backward recomputes
        with torch.no_grad():
            net(_x(B, 3))
        _loss(f1, z1, y).backward()
        after = _engine_stats(eng, model)
        assert not eng.bn_frozen                                 # the handle's flag is handed back as it was
        for k in before:
            assert np.array_equal(before[k], after[k]), k
        net.freeze_bn(False)                                     # a batch-statistics call on the same net still moves them
        with torch.no_grad():
            net(x.detach())
        moved = _engine_stats(eng, model)
    for k in before:
        if "num_batches" in k:
            assert int(moved[k]) == int(before[k]) + 1, k
        else:
            assert not np.array_equal(moved[k], before[k]), k


# ---- 2. the forward is eval arithmetic -----------------------------------------------------------------------------------
def _rel(got, want):
    return float(np.abs(got - want).max() / (np.abs(want).max() + 1e-12))


@pytest.mark.parametrize("model,precision", MODELS)
def test_frozen_forward_is_eval_arithmetic(model, precision):
    """frozen train-mode feat / logits with no draws installed against the CPU oracle in eval mode, at the bound the eval-forward
    test of that model and precision holds fm_forward_eval to (tests/test_engine_gpu.py, test_effnet_gpu.py: assert_allclose;
    test_effnet_bf16_gpu.py: 1e-2 of the max); fm_forward_eval itself against the same oracle next to it."""
    B = 5
    net = _net(model, precision).freeze_bn()
    ref = _oracle(model, precision).eval()
    x = _x(B, 21)
    with torch.no_grad():
        fr, zr = ref(x)
    with _draws(net, B, seed=None), torch.no_grad():
        ff, zf = net(x)
        fe, ze = net.eval()(x)
    ff, zf, fe, ze, fr, zr = [t.cpu().numpy() for t in (ff, zf, fe, ze, fr, zr)]
    fig = {"frozen_feat": _rel(ff, fr), "frozen_logits": _rel(zf, zr), "eval_feat": _rel(fe, fr), "eval_logits": _rel(ze, zr)}
    print(f"{model} {precision}: rel-to-max distance from the eval-mode oracle: {fig}")
    _record(f"forward_{model}_{precision}", fig)
    for got_f, got_z in ((ff, zf), (fe, ze)):
        if precision == "bf16":
            assert _rel(got_f, fr) < 1e-2 and _rel(got_z, zr) < 1e-2, fig
        else:
            rtol, atol = (1e-4, 1e-5) if model == "Resnet18" else (2e-4, 2e-5)
            np.testing.assert_allclose(got_f, fr, rtol=rtol, atol=atol)
            np.testing.assert_allclose(got_z, zr, rtol=rtol, atol=atol)


# ---- 3. images are independent ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,precision", MODELS)
def test_gradient_of_one_image_does_not_reach_the_others(model, precision):
    """the loss is taken on image 0 alone: with frozen statistics the other images' x.grad is exactly zero everywhere (no kernel
    of the backward graph applies a batch-coupled cb / cc); with batch statistics it is not."""
    B = 4
    y = _labels(B, 32)
    out = {}
    for frozen in (True, False):
        net = _net(model, precision).freeze_bn(frozen)
        with _draws(net, B):                      # EfficientNet-B0: drop-connect and dropout draws installed
            x = _x(B, 31).cuda().requires_grad_(True)
            f, z = net(x)
            _loss(f[:1], z[:1], y[:1]).backward()
            out[frozen] = x.grad.cpu()
    assert out[True][0].abs().max() > 0
    nz = int(torch.count_nonzero(out[True][1:]))
    assert nz == 0, f"{nz} elements of x.grad[1:] are not zero, max {float(out[True][1:].abs().max()):.3e}"
    assert out[False][1:].abs().max() > 0


def test_fp32_operand_resnet_images_are_independent():
    """ResNet-18's fp32-operand kernels (products=0, no planes) take the same frozen finalizes: engine level, d loss / d logits
    of image 0 only"""
    from fedmlp_amd.engine import Engine
    B = 4
    e = Engine("Resnet18", C_, HW, HW, 8, products=0)
    try:
        assert not e.planes
        e.set_state(*_prepared("Resnet18", "fp32"))
        x = _x(B, 33).cuda()
        D = torch.zeros((B, C_), device="cuda")
        D[0] = torch.tensor([0.3, -0.2, 0.1, 0.4, -0.5])
        dxs = {}
        for frozen in (True, False):
            e.bn_freeze(frozen)
            assert e.bn_frozen is frozen
            e.forward_train(x)
            e.bn_freeze(not frozen)               # the backward runs in the pending forward's mode, whatever the flag is by then
            dx = torch.full_like(x, float("nan"))
            e.backward_grads(D, None, dx=dx)
            dxs[frozen] = dx.cpu()
    finally:
        e.close()
    assert torch.isfinite(dxs[True]).all() and dxs[True][0].abs().max() > 0
    assert int(torch.count_nonzero(dxs[True][1:])) == 0
    assert dxs[False][1:].abs().max() > 0


# ---- 4. gradients against the oracle ---------------------------------------------------------------------------------------
def _cmp_param_grads(got, ref, rtol=5e-5):
    """tests/test_input_grad_gpu.py::_cmp_param_grads: every parameter, the BatchNorm weights and biases included"""
    bad = []
    for k, p in ref.named_parameters():
        want = p.grad.numpy() if p.grad is not None else np.zeros_like(got[k])
        err = float(np.abs(got[k] - want).max() / (np.abs(want).max() + 1e-12))
        if not err < rtol:
            bad.append(f"{k}: {err:.3e}")
    assert not bad, "grad rel-to-max errors: " + "; ".join(bad[-14:])


@pytest.mark.parametrize("hw,B", [(64, 6), (224, 2)])
def test_resnet_frozen_grads_against_oracle(hw, B):
    """tests/test_input_grad_gpu.py::test_resnet_x_grad_against_oracle with frozen statistics on both sides: the oracle under
    the engine's discrete decisions (every ReLU mask, the stem's, the max-pool choices), x.grad within max(5e-5, 3 e_ref) of the
    float64 oracle, every parameter gradient (bn*.weight / bias too) at 5e-5 of its max, mask flips <= 16."""
    maxi = max(MAXI if hw == 64 else 4, B)
    net = _net(maxi=maxi).freeze_bn()
    eng = net.bind(hw, hw, maxi)
    ref = _oracle("Resnet18")
    y = _labels(B, 12)
    x = _x(B, 11, hw).requires_grad_(True)
    net.zero_grad()
    f, z = net(x)
    rm = relu_masks_from_engine(eng, 1, B, stem=True)
    _loss(f, z, y).backward()
    got_p, got_x = _np(net.grads()), x.grad.double().numpy()

    def oracle(dtype):
        r = copy.deepcopy(ref).to(dtype)
        assert not r.bn1.training and r.training
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
    print(f"frozen x.grad {hw}x{hw} B {B}: engine vs float64 {e_eng:.3e}, fp32 oracle vs float64 {e_ref:.3e}, bound {bound:.3e}, "
          f"flips {flips}")
    _record(f"resnet18_{hw}_B{B}", {"engine_vs_f64": e_eng, "oracle_f32_vs_f64": e_ref, "bound": bound, "mask_flips": flips,
                                    "pool_flips": int(rm.pool_flips)})
    assert flips <= 16, flips
    _cmp_param_grads(got_p, r32)
    assert e_eng <= bound, (e_eng, e_ref)


def _cmp_eff_grads(got, net, rtol=5e-4):
    """tests/test_effnet_gpu.py::_cmp_grads on a dict of gradients"""
    bad, worst = [], ("", 0.0)
    typ = float(np.median([p.grad.abs().max().item() for _, p in net.named_parameters()]))
    floor = 1e-4 * typ
    for k, p in net.named_parameters():
        want = p.grad.numpy()
        if k.endswith("._bn2.bias") and np.abs(want).max() < floor and np.abs(got[k]).max() < floor:
            continue
        err = float(np.abs(got[k] - want).max() / max(np.abs(want).max(), floor))
        if err > worst[1]:
            worst = (k, err)
        if not err < rtol:
            bad.append(f"{k}: {err:.3e} (|want| {np.abs(want).max():.2e} |got| {np.abs(got[k]).max():.2e} floor {floor:.1e})")
    assert not bad, f"{len(bad)} tensors off; " + "; ".join(bad[-12:])
    return worst


def test_effnet_frozen_grads_against_oracle():
    """tests/test_input_grad_gpu.py::test_effnet_x_grad_against_oracle with frozen statistics: fp32 x.grad at 5e-4 of its max and
    the parameter gradients at test_effnet_gpu.py's bound against the oracle (BatchNorm in eval, drop-connect / dropout draws
    installed); bf16 storage against the fp32 ENGINE on the same state (< 0.3 of the max, cosine > 0.95)."""
    B = 6
    x, y = _x(B, 61), _labels(B, 62)
    ref = _oracle("Efficient_b0")

    def engine(precision):
        net = _net("Efficient_b0", precision, state_of="fp32").freeze_bn()
        with _draws(net, B) as d:
            xg = x.clone().cuda().requires_grad_(True)
            net.zero_grad()
            f, z = net(xg)
            _loss(f, z, y).backward()
            return xg.grad.cpu().double().numpy(), _np(net.grads()), d.dc, d.dr
    got32, p32, dc, dr = engine("fp32")
    xr = x.clone().requires_grad_(True)
    fr, zr = ref(xr, dc, dr)
    _loss(fr, zr, y).backward()
    want = xr.grad.double().numpy()
    e32 = float(np.abs(got32 - want).max() / np.abs(want).max())
    got16, _, _, _ = engine("bf16")
    e16 = float(np.abs(got16 - got32).max() / np.abs(got32).max())
    cos = float(np.dot(got16.ravel(), got32.ravel()) / (np.linalg.norm(got16) * np.linalg.norm(got32)))
    print(f"frozen EfficientNet-B0 x.grad: fp32 vs oracle {e32:.3e}; bf16 vs fp32 engine {e16:.3e}, cosine {cos:.5f}")
    worst = _cmp_eff_grads(p32, ref)
    _record("efficientnet_b0_64_B6", {"fp32_vs_oracle": e32, "bf16_vs_fp32_engine": e16, "bf16_cosine": cos,
                                      "fp32_worst_param_grad": list(worst)})
    assert e32 < 5e-4, e32
    assert e16 < 0.3 and cos > 0.95, (e16, cos)


# ---- 5. recompute and accumulation -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,precision", MODELS)
def test_two_frozen_calls_one_backward(model, precision):
    B = 4
    net = _net(model, precision).freeze_bn()
    y = _labels(B, 83)
    with _draws(net, B):
        x1 = _x(B, 81).cuda().requires_grad_(True)
        x2 = _x(B, 82).cuda().requires_grad_(True)
        net.zero_grad()
        f1, z1 = net(x1)
        f2, z2 = net(x2)
        (_loss(f1, z1, y) + _loss(f2, z2, y, act=(0, 4), lam=0.2)).backward()      # node 2 direct, node 1 through a recompute
        g12 = _np(net.grads())
        # each call alone
        a1 = _x(B, 81).cuda().requires_grad_(True)
        net.zero_grad()
        f, z = net(a1)
        _loss(f, z, y).backward()
        g1 = _np(net.grads())
        a2 = _x(B, 82).cuda().requires_grad_(True)
        net.zero_grad()
        f, z = net(a2)
        _loss(f, z, y, act=(0, 4), lam=0.2).backward()
        g2 = _np(net.grads())
    assert not torch.equal(x1.grad, x2.grad)
    assert torch.equal(x1.grad, a1.grad) and torch.equal(x2.grad, a2.grad)
    for k in g12:
        assert np.array_equal(g12[k], g2[k] + g1[k]), k


@pytest.mark.parametrize("model,precision", MODELS)
def test_frozen_and_batch_nodes_share_one_backward(model, precision):
    """a batch-statistics node and a frozen node of the same net in one backward: each runs in its own mode (the frozen one
    straight from its pending forward, the batch one through a recompute that re-installs its mode)."""
    B = 4
    y = _labels(B, 93)

    def run(batch_grad, frozen_grad):
        net = _net(model, precision)
        with _draws(net, B):
            xb = _x(B, 91).cuda().requires_grad_(batch_grad)
            xf = _x(B, 92).cuda().requires_grad_(frozen_grad)
            with torch.set_grad_enabled(batch_grad):
                fb, zb = net(xb)                       # moves the running statistics the frozen call then applies
            net.freeze_bn()
            with torch.set_grad_enabled(frozen_grad):
                ff, zf = net(xf)
            loss = 0
            if batch_grad:
                loss = loss + _loss(fb, zb, y)
            if frozen_grad:
                loss = loss + _loss(ff, zf, y, act=(0, 4), lam=0.2)
            loss.backward()
        return xb.grad, xf.grad
    gb, gf = run(True, True)
    gb1, _ = run(True, False)
    _, gf1 = run(False, True)
    assert torch.equal(gb, gb1), "the batch-statistics node did not run in its own mode"
    assert torch.equal(gf, gf1), "the frozen node did not run in its own mode"
    assert not torch.equal(gb, gf)


# ---- 6. the flag leaves the default path alone -----------------------------------------------------------------------------
@pytest.mark.parametrize("model,precision", MODELS)
def test_batch_statistics_call_is_bit_equal_after_a_frozen_one(model, precision):
    B = 4
    net = _net(model, precision)
    y = _labels(B, 72)
    with _draws(net, B):
        out = []
        for k in range(2):
            x = _x(B, 71).cuda().requires_grad_(True)
            net.zero_grad()
            f, z = net(x)
            _loss(f, z, y).backward()
            out.append((_np(net.grads()), x.grad.clone()))
            if k == 0:
                net.freeze_bn(True)
                xf = _x(B, 73).cuda().requires_grad_(True)
                f, z = net(xf)
                _loss(f, z, y).backward()
                net.freeze_bn(False)
    assert torch.equal(out[0][1], out[1][1])
    for k in out[0][0]:
        assert np.array_equal(out[0][0][k], out[1][0][k]), k


@pytest.mark.parametrize("model,precision", MODELS)
def test_fused_step_ignores_the_flag(model, precision):
    from fedmlp_amd.engine import Engine
    B = 4
    x, y = _x(B, 75).cuda(), _labels(B, 76).cuda()
    flat, cnt = _prepared(model, precision)
    res = []
    for flag in (True, False):
        e = Engine(model, C_, HW, HW, 8, precision=precision)
        try:
            e.stochastic = False
            e.set_state(flat, cnt)
            e.adam_reset(LR)
            if flag:
                e.bn_freeze(True)
                assert e.bn_frozen
            lo = torch.zeros(1, device="cuda")
            e.step_bce(x, y, [3.0, 1.5, 4.0, 2.0, 2.5], 8, lo)
            res.append((lo.item(),) + e.get_state())
        finally:
            e.close()
    assert res[0][0] == res[1][0]
    assert np.array_equal(res[0][1], res[1][1]) and np.array_equal(res[0][2], res[1][2])
    assert not np.array_equal(res[0][1], flat) and int(res[0][2][0]) == int(cnt[0]) + 1     # batch statistics: they moved


# ---- 7. one frozen fine-tuning step ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,precision", MODELS)
def test_one_frozen_fine_tuning_step(model, precision):
    """net.train().freeze_bn(); Adam(net); loss.backward(); opt.step() against torch Adam on the oracle (BatchNorm in eval) at
    the post-Adam bound of tests/test_autograd_gpu.py (_cmp_state: rtol 1e-4, atol 2.5 lr on the weights); the running
    statistics and counters keep their bits."""
    B = 6
    net = _net(model, precision).freeze_bn()
    ref = _oracle(model, precision)
    x, y = _x(B, 41), _labels(B, 42)
    with _draws(net, B) as d:
        eng = d.eng
        before = _engine_stats(eng, model)
        opt = Adam(net, lr=LR, betas=(0.9, 0.999), weight_decay=WD)
        ropt = torch.optim.Adam(ref.parameters(), lr=LR, betas=(0.9, 0.999), weight_decay=WD)
        f, z = net(x)
        rm = relu_masks_from_engine(eng, 1, B, stem=True) if model == "Resnet18" else None
        opt.zero_grad()
        _loss(f, z, y).backward()
        opt.step()
        after = _engine_stats(eng, model)
        ropt.zero_grad()
        if rm is not None:
            with rm:
                fr, zr = ref(x)
                _loss(fr, zr, y).backward()
        else:
            fr, zr = ref(x, d.dc, d.dr)
            _loss(fr, zr, y).backward()
        ropt.step()
    for k in before:
        assert np.array_equal(before[k], after[k]), k
    sd = net.state_dict()
    sd0 = spec.flat_to_state_dict(model, C_, *_prepared(model, precision))
    changed = trainable = 0
    for k, v in ref.state_dict().items():
        want, got = v.numpy(), sd[k].numpy()
        if "num_batches" in k:
            assert int(got) == int(want), k
            continue
        if "running" in k:
            assert np.array_equal(got, want), k              # neither side updated them
            continue
        np.testing.assert_allclose(got, want, rtol=1e-4, atol=2.5 * LR, err_msg=k)
        trainable += 1
        changed += int(not np.array_equal(got, np.asarray(sd0[k])))
    assert changed == trainable, (changed, trainable)        # ... and the step did step: every tensor moved
