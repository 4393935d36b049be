"""Train-mode net(x) as an autograd graph on a real MI355X: HipNet's node runs the engine's backward into the gradient
accumulator (fm_backward_grads), fedmlp_amd.optim.Adam steps from it (fm_adam_step).  Bit-identity with the fused split
step, the feature gradient and the two-call pattern against the CPU oracle, accumulation, a FedIRM-shaped loop."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from fedmlp_amd import spec
from fedmlp_amd.model import HipNet
from fedmlp_amd.optim import Adam
from tests.helpers import oracle_net, relu_masks_from_engine

pytestmark = pytest.mark.gpu

C_, HW = 5, 64
LR, WD = 3e-5, 5e-4
MAXI = 16          # engine workspace (images per forward) of every net here


def _net(model="Resnet18", precision="fp32", seed=1037):
    flat, cnt = spec.init_state(model, C_, seed)
    net = HipNet(model, C_, flat, cnt)
    net.default_max_images, net.precision = MAXI, precision
    return net.train()


def _x(B, seed):
    return torch.randn((B, 3, HW, HW), generator=torch.Generator().manual_seed(seed))


def _labels(B, seed):
    return (torch.rand((B, C_), generator=torch.Generator().manual_seed(seed)) < 0.4).float()


def _np(grads):
    return {k: v.cpu().numpy().copy() for k, v in grads.items()}


def _cmp_grads(got, ref, rtol=5e-5):
    """max |g_hip - g_oracle| / max |g_oracle| per parameter tensor (test_engine_gpu.py's bound); a parameter outside the
    oracle's graph must have an exactly zero gradient."""
    bad = []
    for k, p in ref.named_parameters():
        want = p.grad.numpy() if p.grad is not None else np.zeros_like(got[k])
        err = float(np.abs(got[k] - want).max() / (np.abs(want).max() + 1e-12))
        if not err < rtol:
            bad.append(f"{k}: {err:.3e}")
    assert not bad, "grad rel-to-max errors: " + "; ".join(bad[-14:])


def _cmp_state(net, ref, atol_w):
    """test_engine_gpu.py's _cmp_state on a HipNet's state_dict."""
    sd = net.state_dict()
    for k, v in ref.state_dict().items():
        want, got = v.numpy(), sd[k].numpy()
        if "num_batches" in k:
            assert int(got) == int(want), k
            continue
        tol = atol_w if ("running" not in k) else 1e-5 * (np.abs(want).max() + 1.0)
        np.testing.assert_allclose(got, want, rtol=1e-4, atol=tol, err_msg=k)


def test_train_mode_call_returns_autograd_outputs():
    net = _net()
    f, z = net(_x(4, 1))
    assert f.is_cuda and z.is_cuda and f.grad_fn is not None and z.grad_fn is not None
    assert tuple(f.shape) == (4, 512) and tuple(z.shape) == (4, C_)


@pytest.mark.parametrize("model,precision", [("Resnet18", "fp32"), ("Efficient_b0", "fp32"), ("Efficient_b0", "bf16")])
def test_bitwise_equal_to_fused_split_step(model, precision):
    """Path B (z = net(x); z.backward(D); grads(); Adam.step()) against path A (forward_train; backward_step; the fused
    path's gradients and post-step state) from the same state, x, D and installed draws: every bit equal."""
    B = 6
    net = _net(model, precision)
    x = _x(B, 2).cuda()
    D = (0.1 * torch.randn((B, C_), generator=torch.Generator().manual_seed(3))).cuda()
    flat0, cnt0 = net.flat.copy(), net.counters.copy()
    eng = net.bind(HW, HW, MAXI)
    stochastic = eng.stochastic
    eng.stochastic = False
    try:
        if model == "Efficient_b0":
            from oracle.efficientnet_ref import draw_stochastic
            dc, dr = draw_stochastic(B, torch.Generator().manual_seed(5))
            eng.set_stochastic(dc.cuda(), dr.cuda())
        opt = Adam(net, lr=LR, weight_decay=WD)
        fb, zb = net(x)
        zb.backward(D)
        gb = net.grads()
        gb = torch.cat([v.reshape(-1) for v in gb.values()]).cpu().numpy()
        opt.step()
        sb, cb = eng.get_state()

        eng.set_state(flat0, cnt0)
        eng.adam_reset(LR, weight_decay=WD)
        fa, za = eng.forward_train(x)
        eng.backward_step(D)
        ga_sd = spec.flat_to_state_dict(model, C_, eng.debug_get_grads(), np.zeros(eng.ni, np.int64))
        ga = np.concatenate([np.asarray(ga_sd[k]).reshape(-1) for k, _, dt in spec.entries(model, C_)
                             if dt == "f32" and spec.is_trainable(k)])
        sa, ca = eng.get_state()
    finally:
        eng.stochastic = stochastic
        if model == "Efficient_b0":
            eng.set_stochastic(None, None)
    assert torch.equal(fa, fb.detach()) and torch.equal(za, zb.detach())
    assert np.array_equal(ga, gb), f"gradients differ at {np.count_nonzero(ga != gb)} of {ga.size}"
    assert np.array_equal(sa, sb), f"post-step state differs at {np.count_nonzero(sa != sb)} of {sa.size}"
    assert np.array_equal(ca, cb)


def test_feature_gradient_against_oracle():
    """d loss / d feature enters the head backward: masked BCE + lambda * ||f||^2 / n, and a loss of f alone (dlogits None)."""
    B, lam, act = 6, 0.5, [1, 3]
    net = _net()
    eng = net.bind(HW, HW, MAXI)
    ref = oracle_net(C_, 1037).train()
    x, y = _x(B, 11), _labels(B, 12)

    def bce_feat(f, z):
        bce = F.binary_cross_entropy_with_logits(z, y.to(z.device), reduction="none")[:, act].sum() / (B * len(act))
        return bce + lam * f.pow(2).sum() / f.numel()

    def feat_only(f, z):
        return lam * f.pow(2).sum() / f.numel()

    for loss_fn in (bce_feat, feat_only):
        net.zero_grad()
        f, z = net(x)
        rm = relu_masks_from_engine(eng, 1, B)       # the engine's masks of this forward (reads do not enqueue)
        loss_fn(f, z).backward()
        got = _np(net.grads())
        ref.zero_grad()
        with rm:
            fr, zr = ref(x)
            loss_fn(fr, zr).backward()
        assert rm.flips <= 16, rm.flips
        _cmp_grads(got, ref)


def _fedirm_loss(z1, z2, y, pw, act, bs, ann):
    """utils/local_training.py:370-376: BCEWithLogits(pos_weight, reduction='none') over both views, active classes,
    / (batch_size * annotation_num)."""
    crit = torch.nn.BCEWithLogitsLoss(pos_weight=torch.tensor(pw, device=z1.device), reduction="none")
    y = y.to(z1.device)
    return (crit(z1, y) + crit(z2, y))[:, act].sum() / (bs * ann)


def test_two_calls_one_backward():
    B, act, pw = 6, [0, 2], [2.0, 1.5, 3.0, 1.0, 2.5]
    net = _net()
    eng = net.bind(HW, HW, MAXI)
    ref = oracle_net(C_, 1037).train()
    x1, x2, y = _x(B, 21), _x(B, 22), _labels(B, 23)
    cnt0 = net.counters.copy()
    f1, z1 = net(x1)
    rm = relu_masks_from_engine(eng, 1, B)
    f2, z2 = net(x2)
    rm.masks += relu_masks_from_engine(eng, 1, B).masks    # the oracle's ReLU calls: view 1's, then view 2's
    loss = _fedirm_loss(z1, z2, y, pw, act, 8, 2) + 0.1 * f1.pow(2).mean()
    loss.backward()                              # node 2 straight after its forward, node 1 through a recompute
    got = _np(net.grads())
    with rm:
        fr1, zr1 = ref(x1)
        fr2, zr2 = ref(x2)
        (_fedirm_loss(zr1, zr2, y, pw, act, 8, 2) + 0.1 * fr1.pow(2).mean()).backward()
    assert rm.flips <= 32, rm.flips
    _cmp_grads(got, ref)
    # two train-mode calls: running statistics and num_batches_tracked move exactly twice (the recompute moved nothing)
    assert np.array_equal(net.state_dict()["bn1.num_batches_tracked"].numpy(), np.int64(cnt0[0] + 2))
    _cmp_state(net, ref, atol_w=0.0)

    # the recomputed node's gradients are those it produces straight after its own forward, bit for bit
    def view1_loss(f, z):
        return F.binary_cross_entropy_with_logits(z, y.cuda(), reduction="sum") / 8 + 0.1 * f.pow(2).mean()
    net.zero_grad()
    f1, z1 = net(x1)
    net(x2)
    view1_loss(f1, z1).backward()                # recompute, then backward
    recomputed = _np(net.grads())
    net.zero_grad()
    f1, z1 = net(x1)
    view1_loss(f1, z1).backward()                # straight after the forward
    direct = _np(net.grads())
    for k in direct:
        assert np.array_equal(recomputed[k], direct[k]), k


def test_accumulation_is_the_fp32_sum():
    B = 5
    net = _net()
    x1, x2 = _x(B, 31), _x(B, 32)
    D1 = (0.1 * torch.randn((B, C_), generator=torch.Generator().manual_seed(33))).cuda()
    D2 = (0.1 * torch.randn((B, C_), generator=torch.Generator().manual_seed(34))).cuda()
    net(x1)[1].backward(D1)
    g1 = _np(net.grads())
    net.zero_grad()
    net(x2)[1].backward(D2)
    g2 = _np(net.grads())
    net.zero_grad()
    net(x1)[1].backward(D1)
    net(x2)[1].backward(D2)
    g12 = _np(net.grads())
    for k in g1:
        assert np.array_equal(g12[k], g1[k] + g2[k]), k
    net.zero_grad()
    assert all(not v.any() for v in _np(net.grads()).values())


def test_fedirm_phase1_loop_against_oracle():
    """Three steps of train_FedIRM's supervised phase (utils/local_training.py:370-379) with fedmlp_amd.optim.Adam against
    the oracle with torch.optim.Adam."""
    B, act, pw, ann = 6, [1], [2.0, 3.0, 1.5, 1.0, 2.5], 1
    net = _net()
    eng = net.bind(HW, HW, MAXI)
    ref = oracle_net(C_, 1037).train()
    opt = Adam(net, lr=LR, betas=(0.9, 0.999), weight_decay=WD)
    ropt = torch.optim.Adam(ref.parameters(), lr=LR, betas=(0.9, 0.999), weight_decay=WD)
    for step in range(3):
        x1, x2, y = _x(B, 40 + 3 * step), _x(B, 41 + 3 * step), _labels(B, 42 + 3 * step)
        _, l1 = net(x1)
        rm = relu_masks_from_engine(eng, 1, B)
        _, l2 = net(x2)
        rm.masks += relu_masks_from_engine(eng, 1, B).masks
        loss = _fedirm_loss(l1, l2, y, pw, act, 8, ann)
        opt.zero_grad()
        loss.backward()
        opt.step()
        with rm:
            _, r1 = ref(x1)
            _, r2 = ref(x2)
            rloss = _fedirm_loss(r1, r2, y, pw, act, 8, ann)
            ropt.zero_grad()
            rloss.backward()
        ropt.step()
        assert rm.flips <= 32, rm.flips
        assert abs(loss.item() - rloss.item()) < 1e-4 * abs(rloss.item()) + 1e-6, (step, loss.item(), rloss.item())
    _cmp_state(net, ref, atol_w=2.5 * LR)


def test_backward_after_step_raises():
    net = _net()
    opt = Adam(net, lr=LR)
    _, z1 = net(_x(4, 51))
    _, z2 = net(_x(4, 52))
    z2.sum().backward()
    opt.step()
    with pytest.raises(RuntimeError, match="weights changed"):
        z1.sum().backward()
