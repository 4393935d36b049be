"""EfficientNet-B0 path (BASELINE configs 4-5) on a real MI355X through the C ABI: eval forward
and one training step of each variant against the CPU oracle (oracle/efficientnet_ref.py) on the
same seeded inputs and the same drop-connect / dropout draws."""
import copy

import numpy as np
import pytest
import torch

from fedmlp_amd import spec
from oracle import steps_ref as R
from oracle.efficientnet_ref import EfficientNetB0Ref, draw_stochastic

pytestmark = pytest.mark.gpu

M = "Efficient_b0"
C_, HW = 5, 64
LR = 3e-5


@pytest.fixture(scope="module")
def eng():
    from fedmlp_amd.engine import Engine
    e = Engine(M, C_, HW, HW, 16)
    e.stochastic = False          # the tests install the oracle's draws themselves
    yield e
    e.close()


def _oracle(seed, perturb=True):
    net = EfficientNetB0Ref(C_)
    flat, cnt = spec.init_state(M, C_, seed)
    sd = spec.flat_to_state_dict(M, C_, flat, cnt)
    g = torch.Generator().manual_seed(seed + 1)
    out = {}
    for k, v in sd.items():
        t = torch.from_numpy(np.asarray(v))
        if perturb and t.dtype == torch.float32:
            # non-trivial BN affine / running stats and SE biases, so that nothing is tested at 0/1
            if k.endswith("running_var"):
                t = t * (0.5 + torch.rand(t.shape, generator=g))
            elif k.endswith("running_mean") or k.endswith(".bias"):
                t = t + 0.1 * torch.randn(t.shape, generator=g)
            elif t.dim() == 1:
                t = t * (1.0 + 0.1 * torch.randn(t.shape, generator=g))
        out[k] = t
    net.load_state_dict(out)
    return net


def _load(e, seed=1037):
    net = _oracle(seed)
    flat, cnt = spec.state_dict_to_flat(M, C_, net.state_dict())
    e.set_state(flat, cnt)
    e.adam_reset(LR)
    return net


def _data(B, seed, views=1):
    g = torch.Generator().manual_seed(seed)
    xs = [torch.randn((B, 3, HW, HW), generator=g) for _ in range(views)]
    y = (torch.rand((B, C_), generator=g) < 0.3).float()
    return xs, y


def _cmp_grads(e, net, rtol=5e-4):
    flat = e.debug_get_grads()
    gsd = spec.flat_to_state_dict(M, C_, flat, np.zeros(e.ni, np.int64))
    bad, worst = [], ("", 0.0)
    # Without drop-connect `_bn2.bias` of every block has an analytically ZERO gradient (a per-channel
    # constant added before a conv that is followed by BatchNorm is removed by that BatchNorm): both
    # sides hold rounding noise there (~1e-9 against typical gradients of ~4e-3).  Such tensors pass
    # when both sides are zero to 1e-4 of the typical per-tensor gradient magnitude.
    typ = float(np.median([p.grad.abs().max().item() for _, p in net.named_parameters()]))
    floor = 1e-4 * typ
    for k, p in net.named_parameters():
        want = p.grad.numpy()
        got = gsd[k]
        if k.endswith("._bn2.bias") and np.abs(want).max() < floor and np.abs(got).max() < floor:
            continue
        err = float(np.abs(got - want).max() / max(np.abs(want).max(), floor))
        if err > worst[1]:
            worst = (k, err)
        if not err < rtol:
            bad.append(f"{k}: {err:.3e} (|want| {np.abs(want).max():.2e} |got| {np.abs(got).max():.2e} floor {floor:.1e})")
    assert not bad, f"{len(bad)} tensors off; " + "; ".join(bad[-12:])
    return worst


def _cmp_state(e, net, atol_w):
    flat, cnt = e.get_state()
    sd = spec.flat_to_state_dict(M, C_, flat, cnt)
    for k, v in net.state_dict().items():
        want = v.numpy()
        if "num_batches" in k:
            assert int(sd[k]) == int(want), k
            continue
        tol = atol_w if ("running" not in k) else 1e-5 * (np.abs(want).max() + 1.0)
        np.testing.assert_allclose(sd[k], want, rtol=1e-4, atol=tol, err_msg=k)


def test_state_roundtrip(eng):
    net = _load(eng)
    flat, cnt = eng.get_state()
    want, _ = spec.state_dict_to_flat(M, C_, net.state_dict())
    np.testing.assert_array_equal(flat, want)


def test_forward_eval(eng):
    net = _load(eng)
    (x,), _ = _data(5, 1)
    net.eval()
    with torch.no_grad():
        f, z = net(x)
    fe, ze = eng.forward_eval(x.cuda())
    np.testing.assert_allclose(fe.cpu().numpy(), f.numpy(), rtol=2e-4, atol=2e-5)
    np.testing.assert_allclose(ze.cpu().numpy(), z.numpy(), rtol=2e-4, atol=2e-5)


def test_forward_eval_224():
    from fedmlp_amd.engine import Engine
    e = Engine(M, C_, 224, 224, 4)
    try:
        net = _oracle(7)
        flat, cnt = spec.state_dict_to_flat(M, C_, net.state_dict())
        e.set_state(flat, cnt)
        g = torch.Generator().manual_seed(3)
        x = torch.randn((3, 3, 224, 224), generator=g)
        net.eval()
        with torch.no_grad():
            f, z = net(x)
        fe, ze = e.forward_eval(x.cuda())
        np.testing.assert_allclose(fe.cpu().numpy(), f.numpy(), rtol=2e-4, atol=2e-5)
        np.testing.assert_allclose(ze.cpu().numpy(), z.numpy(), rtol=2e-4, atol=2e-5)
    finally:
        e.close()


@pytest.mark.parametrize("stochastic", [False, True])
def test_step_bce(eng, stochastic):
    net = _load(eng)
    (x,), y = _data(6, 2)
    pw = [3.0, 1.5, 4.0, 2.0, 2.5]
    dc = dr = None
    if stochastic:
        dc, dr = draw_stochastic(6, torch.Generator().manual_seed(5))
    eng.set_stochastic(None if dc is None else dc.cuda(), None if dr is None else dr.cuda())
    net.train()
    opt = torch.optim.Adam(net.parameters(), lr=LR, betas=(0.9, 0.999), weight_decay=5e-4)
    _, z = net(x, dc, dr)
    loss = R.loss_train(z, y, pw, 8, C_)
    opt.zero_grad(); loss.backward(); opt.step()
    lo = torch.zeros(1, device="cuda")
    eng.step_bce(x.cuda(), y.cuda(), pw, 8, lo)
    eng.set_stochastic(None, None)
    assert abs(lo.item() - loss.item()) < 2e-5 * abs(loss.item()) + 1e-7
    _cmp_grads(eng, net)
    _cmp_state(eng, net, atol_w=2.5 * LR)


def test_step_stage1(eng):
    net = _load(eng)
    (x1, x2), y = _data(6, 3, views=2)
    act, neg = [1], [0, 2, 3, 4]
    glob = copy.deepcopy(net).eval()
    eng.teacher_snapshot()
    gen = torch.Generator().manual_seed(9)
    dc1, dr1 = draw_stochastic(6, gen)
    dc2, dr2 = draw_stochastic(6, gen)
    net.train()
    opt = torch.optim.Adam(net.parameters(), lr=LR, betas=(0.9, 0.999), weight_decay=5e-4)
    _, z1 = net(x1, dc1, dr1)
    _, z2 = net(x2, dc2, dr2)
    with torch.no_grad():
        _, g1 = glob(x1)
        _, g2 = glob(x2)
    loss, _, _ = R.loss_stage1(z1, z2, g1, g2, y, act, neg, 8, 1)
    opt.zero_grad(); loss.backward(); opt.step()
    mask = [1.0 if c in act else 0.0 for c in range(C_)]
    lo = torch.zeros(1, device="cuda")
    eng.set_stochastic(torch.cat([dc1, dc2], 1).cuda(), torch.cat([dr1, dr2], 0).cuda())
    try:
        eng.step_stage1(x1.cuda(), x2.cuda(), y.cuda(), mask, 1, 8, lo)
    finally:
        eng.set_stochastic(None, None)
    assert abs(lo.item() - loss.item()) < 2e-5 * abs(loss.item()) + 1e-7
    _cmp_grads(eng, net)
    _cmp_state(eng, net, atol_w=2.5 * LR)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_step_stage1_chestxray14_shape(monkeypatch, precision):
    """BASELINE configs[4]'s head shape: 14 labels on the 1280-wide feature, three annotated classes, one stage-1 step
    against the oracle.  fp32: the bounds of test_step_stage1; bf16: loss within 5e-3 (measured 1.6e-3), the classifier's
    gradient within 0.1 of its max elementwise (measured 5.8e-2) and cosine > 0.998 (measured 0.9994)."""
    import sys
    from fedmlp_amd.engine import Engine
    monkeypatch.setattr(sys.modules[__name__], "C_", 14)
    e = Engine(M, 14, HW, HW, 16, precision=precision)
    e.stochastic = False
    try:
        net = _load(e)
        g = torch.Generator().manual_seed(21)
        x1 = torch.randn((6, 3, HW, HW), generator=g); x2 = torch.randn((6, 3, HW, HW), generator=g)
        y = (torch.rand((6, 14), generator=g) < 0.3).float()
        act = [2, 7, 11]
        neg = [c for c in range(14) if c not in act]
        glob = copy.deepcopy(net).eval()
        e.teacher_snapshot()
        net.train()
        opt = torch.optim.Adam(net.parameters(), lr=LR, betas=(0.9, 0.999), weight_decay=5e-4)
        _, z1 = net(x1); _, z2 = net(x2)
        with torch.no_grad():
            _, g1 = glob(x1); _, g2 = glob(x2)
        loss, _, _ = R.loss_stage1(z1, z2, g1, g2, y, act, neg, 8, 3)
        opt.zero_grad(); loss.backward(); opt.step()
        mask = [1.0 if c in act else 0.0 for c in range(14)]
        lo = torch.zeros(1, device="cuda")
        e.set_stochastic(None, None)
        e.step_stage1(x1.cuda(), x2.cuda(), y.cuda(), mask, 3, 8, lo)
        rel = abs(lo.item() - loss.item()) / abs(loss.item())
        if precision == "fp32":
            assert rel < 2e-5, rel
            _cmp_grads(e, net)
            _cmp_state(e, net, atol_w=2.5 * LR)
        else:
            assert rel < 5e-3, rel
            gsd = spec.flat_to_state_dict(M, 14, e.debug_get_grads(), np.zeros(e.ni, np.int64))
            for k in ("_fc.weight", "_fc.bias"):
                want, got = dict(net.named_parameters())[k].grad.numpy().ravel(), gsd[k].ravel()
                dev = np.abs(got - want).max() / np.abs(want).max()
                cos = np.dot(got, want) / (np.linalg.norm(got) * np.linalg.norm(want))
                print(f"bf16 C=14 {k}: deviation {dev:.3e} of max, cosine {cos:.5f}, loss rel {rel:.2e}")
                assert dev < 0.1 and cos > 0.998, (k, dev, cos)
    finally:
        e.close()


def test_multi_step_loss_track(eng):
    """5 consecutive BCE steps: per-step loss follows the oracle's."""
    net = _load(eng, seed=11)
    pw = [2.0] * C_
    net.train()
    opt = torch.optim.Adam(net.parameters(), lr=1e-3, betas=(0.9, 0.999), weight_decay=5e-4)
    eng.adam_reset(1e-3)
    lo = torch.zeros(1, device="cuda")
    for it in range(5):
        (x,), y = _data(8, 100 + it)
        _, z = net(x)
        loss = R.loss_train(z, y, pw, 8, C_)
        opt.zero_grad(); loss.backward(); opt.step()
        eng.step_bce(x.cuda(), y.cuda(), pw, 8, lo)
        assert abs(lo.item() - loss.item()) < 2e-3 * abs(loss.item()), (it, lo.item(), loss.item())


def test_localupdate_surface_efficient_b0():
    """build_model(args.model='Efficient_b0') + LocalUpdate.train + stage-1/2 of train_FedMLP run
    through the same drop-in surface as ResNet-18; with the stochastic draws off, one epoch of
    LocalUpdate.train follows the oracle's RefClient.train on the same batch order."""
    import types
    from fedmlp_amd.model import build_model
    from tests.helpers import replay_local_update
    LocalUpdate = replay_local_update()      # LocalUpdate + recorded batch orders / tagging log (tests/helpers.py)
    from tests.helpers import make_args, data_dict
    from tests.test_local_training_gpu import SynthDataset
    from tests.synth import class_lists
    C, N, hw = 5, 24, 64
    args = make_args(n_classes=C, n_clients=1, seed=5, model=M, batch_size=8, feature_dim=1280)
    ds = SynthDataset(N, C, hw, 77, False)
    pos, neg = class_lists(ds.targets, C)
    net = build_model(args)
    loc = LocalUpdate(args, 0, ds, list(range(N)), pos, neg, active_class_list=[0])
    order = torch.randperm(N, generator=torch.Generator().manual_seed(1)).tolist()
    loc.order_queue.append(order)
    eng = loc._bind(net, "image")
    eng.stochastic = False
    ref_net = EfficientNetB0Ref(C)
    ref_net.load_state_dict({k: torch.as_tensor(np.asarray(v)) for k, v in net.state_dict().items()})
    sd, loss, _, _, negl, actl = loc.train(0, net, None)
    eng.stochastic = True
    rc = R.RefClient(args, 0, data_dict(N, C, hw, 77, False), list(range(N)), neg, [0])
    _, want_loss, _ = rc.train(ref_net, order)
    assert abs(loss - want_loss) < 2e-3 * abs(want_loss), (loss, want_loss)
    for k, v in ref_net.state_dict().items():
        if "num_batches" in k:
            assert int(sd[k]) == int(v)
        elif "running" in k:
            np.testing.assert_allclose(np.asarray(sd[k]), v.numpy(), rtol=1e-3, atol=1e-5, err_msg=k)
    # with the draws on (the product default) the step still runs and the loss stays finite
    loc.order_queue.append(order)
    _, loss2, _, _, _, _ = loc.train(1, net, None)
    assert np.isfinite(loss2)


def test_step_stage2(eng):
    net = _load(eng)
    (x,), y = _data(7, 4)
    g = torch.Generator().manual_seed(44)
    dist = (torch.rand((7, C_), generator=g) < 0.4).float()
    dc, dr = draw_stochastic(7, torch.Generator().manual_seed(6))
    net.train()
    opt = torch.optim.Adam(net.parameters(), lr=LR, betas=(0.9, 0.999), weight_decay=5e-4)
    _, z = net(x, dc, dr)
    loss = R.loss_stage2(z, y, dist)
    opt.zero_grad(); loss.backward(); opt.step()
    lo = torch.zeros(1, device="cuda")
    eng.set_stochastic(dc.cuda(), dr.cuda())
    try:
        eng.step_stage2(x.cuda(), y.cuda(), dist.cuda(), lo)
    finally:
        eng.set_stochastic(None, None)
    assert abs(lo.item() - loss.item()) < 2e-5 * abs(loss.item()) + 1e-7
    _cmp_grads(eng, net)
    _cmp_state(eng, net, atol_w=2.5 * LR)


def test_step_fixmatch(eng):
    net = _load(eng)
    with torch.no_grad():
        net._fc.weight.mul_(40.0)              # saturate some probabilities -> confident rows
    flat, cnt = spec.state_dict_to_flat(M, C_, net.state_dict())
    eng.set_state(flat, cnt)
    eng.adam_reset(LR)
    (xw, xs), y = _data(8, 5, views=2)
    act, neg = [0], [1, 2, 3, 4]
    pw, pwu = [3.0, 1.5, 4.0, 2.0, 2.5], [3.3, 1, 1, 1, 1]
    net.train()
    opt = torch.optim.Adam(net.parameters(), lr=LR, betas=(0.9, 0.999), weight_decay=5e-4)
    _, zw = net(xw); _, zs = net(xs)
    assert len(R.fixmatch_mask(zw, neg, 8)) > 0, "test needs at least one confident row"
    loss = R.loss_fixmatch(zw, zs, y, pw, pwu, act, neg, 8, 1, C_)
    opt.zero_grad(); loss.backward(); opt.step()
    lo = torch.zeros(1, device="cuda")
    mask = [1.0 if c in act else 0.0 for c in range(C_)]
    eng.step_fixmatch(xw.cuda(), xs.cuda(), y.cuda(), pw, pwu, mask, 1, 8, lo)
    assert abs(lo.item() - loss.item()) < 1e-4 * abs(loss.item()) + 1e-7
    _cmp_grads(eng, net, rtol=2e-3)


def test_prototype_pass_and_tagging_1280(eng):
    """Prototype accumulation / cosine tagging run at the model's feature width (1280)."""
    _load(eng)
    (x,), y = _data(8, 21)
    y[:, 0] = torch.tensor([0, 1, 0, 1, 1, 0, 0, 1.0])
    fe, ze = eng.forward_eval(x.cuda())
    assert fe.shape == (8, 1280)
    act, negm = [1.0, 0, 0, 0, 0], [0.0, 1, 1, 1, 1]
    eng.proto_reset()
    eng.proto_accumulate(fe, ze, y.cuda(), act, negm, 0.3, 0.7)
    t, proto = eng.proto_finalize(False, 8, act)
    want_t, want_proto = R.prototype_pass([(fe.cpu(), ze.cpu(), y)], C_, [0], [1, 2, 3, 4], 0.3, 0.7, 8, False)
    np.testing.assert_allclose(proto[:2], want_proto[:2].numpy(), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(t, want_t, rtol=0, atol=1e-12)
    sim = eng.cos_tag(fe, torch.from_numpy(proto).cuda(), [0])
    want = R.cosine_diff(fe.cpu(), want_proto[0], want_proto[1])
    np.testing.assert_allclose(sim[0].cpu().numpy(), np.asarray(want), rtol=1e-4, atol=1e-5)


def test_step_bce_tail_batch_of_one(eng):
    """A tail batch of one image through the EfficientNet-B0 train step."""
    net = _load(eng)
    (x,), y = _data(1, 78)
    pw = [2.0] * C_
    net.train()
    opt = torch.optim.Adam(net.parameters(), lr=LR, betas=(0.9, 0.999), weight_decay=5e-4)
    _, z = net(x)
    loss = R.loss_train(z, y, pw, 32, C_)
    opt.zero_grad(); loss.backward(); opt.step()
    lo = torch.zeros(1, device="cuda")
    eng.step_bce(x.cuda(), y.cuda(), pw, 32, lo)
    assert abs(lo.item() - loss.item()) < 1e-4 * abs(loss.item()) + 1e-7
    flat, _ = eng.get_state()
    assert np.isfinite(flat).all()


def test_step_bce_generic_depthwise_kernels(eng, monkeypatch):
    """The register-blocked depthwise kernels cover TF-"same" padding of even inputs; any other padding
    takes the generic per-pixel kernels.  FM_DW_GENERIC=1 forces those, and the step must still match."""
    monkeypatch.setenv("FM_DW_GENERIC", "1")
    net = _load(eng)
    (x,), y = _data(5, 9)
    pw = [3.0, 1.5, 4.0, 2.0, 2.5]
    net.train()
    opt = torch.optim.Adam(net.parameters(), lr=LR, betas=(0.9, 0.999), weight_decay=5e-4)
    _, z = net(x)
    loss = R.loss_train(z, y, pw, 8, C_)
    opt.zero_grad(); loss.backward(); opt.step()
    lo = torch.zeros(1, device="cuda")
    eng.step_bce(x.cuda(), y.cuda(), pw, 8, lo)
    assert abs(lo.item() - loss.item()) < 2e-5 * abs(loss.item()) + 1e-7
    _cmp_grads(eng, net)


@pytest.mark.parametrize("hw,views", [(224, 1), (160, 1), (96, 2)])
def test_step_odd_spatial_sizes(hw, views):
    """The benchmark's spatial sizes are 112 / 56 / 28 / 14 / 7; the 64 x 64 tests above only see powers of two.  At
    224 x 224 the blocks run at exactly those sizes (odd rows and 7 % 4 = 3 partial column blocks in the row-uniform
    depthwise kernels, their fused BN statistics and per-image pooling records); 160 x 160 gives 80 / 40 / 20 / 10 / 5 and
    96 x 96 gives 48 / 24 / 12 / 6 / 3 with two statistics groups (a stage-1 step).  fp32, oracle bounds."""
    from fedmlp_amd.engine import Engine
    e = Engine(M, C_, hw, hw, 8)
    try:
        e.stochastic = False
        net = _load(e)
        g = torch.Generator().manual_seed(100 + hw)
        B = 2 if hw > 200 else 3
        xs = [torch.randn((B, 3, hw, hw), generator=g) for _ in range(views)]
        y = (torch.rand((B, C_), generator=g) < 0.3).float()
        net.train()
        opt = torch.optim.Adam(net.parameters(), lr=LR, betas=(0.9, 0.999), weight_decay=5e-4)
        lo = torch.zeros(1, device="cuda")
        if views == 1:
            pw = [3.0, 1.5, 4.0, 2.0, 2.5]
            _, z = net(xs[0])
            loss = R.loss_train(z, y, pw, 4, C_)
            opt.zero_grad(); loss.backward(); opt.step()
            e.step_bce(xs[0].cuda(), y.cuda(), pw, 4, lo)
        else:
            import copy
            glob = copy.deepcopy(net).eval()
            e.teacher_snapshot()
            act, neg = [1], [0, 2, 3, 4]
            _, z1 = net(xs[0]); _, z2 = net(xs[1])
            with torch.no_grad():
                _, g1 = glob(xs[0]); _, g2 = glob(xs[1])
            loss, _, _ = R.loss_stage1(z1, z2, g1, g2, y, act, neg, 4, 1)
            opt.zero_grad(); loss.backward(); opt.step()
            mask = [1.0 if c in act else 0.0 for c in range(C_)]
            e.step_stage1(xs[0].cuda(), xs[1].cuda(), y.cuda(), mask, 1, 4, lo)
        assert abs(lo.item() - loss.item()) < 5e-5 * abs(loss.item()) + 1e-7
        _cmp_grads(e, net)
        _cmp_state(e, net, atol_w=2.5 * LR)
    finally:
        e.close()


def test_stage1_step_mid_size_224(tmp_path):
    """A stage-1 step at 224 x 224 with 16 images per view (32 train-mode + 32 teacher images): large enough that the
    depthwise kernels' fused BN statistics run with many row groups per statistics group, several reducer splits and
    multi-block squeeze-excite / pointwise launches -- the shapes of the benchmark, not of the 3-image tests.  fp32 engine
    vs the fp32 oracle at the step bounds."""
    from fedmlp_amd.engine import Engine
    B, hw = 16, 224
    e = Engine(M, C_, hw, hw, 4 * B)
    try:
        e.stochastic = False
        net = _load(e)
        g = torch.Generator().manual_seed(4242)
        x1 = torch.randn((B, 3, hw, hw), generator=g); x2 = torch.randn((B, 3, hw, hw), generator=g)
        y = (torch.rand((B, C_), generator=g) < 0.3).float()
        glob = copy.deepcopy(net).eval()
        e.teacher_snapshot()
        act, neg = [1], [0, 2, 3, 4]
        net.train()
        opt = torch.optim.Adam(net.parameters(), lr=LR, betas=(0.9, 0.999), weight_decay=5e-4)
        _, z1 = net(x1); _, z2 = net(x2)
        with torch.no_grad():
            _, g1 = glob(x1); _, g2 = glob(x2)
        loss, _, _ = R.loss_stage1(z1, z2, g1, g2, y, act, neg, B, 1)
        opt.zero_grad(); loss.backward(); opt.step()
        mask = [1.0 if c in act else 0.0 for c in range(C_)]
        lo = torch.zeros(1, device="cuda")
        e.step_stage1(x1.cuda(), x2.cuda(), y.cuda(), mask, 1, B, lo)
        assert abs(lo.item() - loss.item()) < 5e-5 * abs(loss.item()) + 1e-7
        _cmp_grads(e, net)
        _cmp_state(e, net, atol_w=2.5 * LR)
    finally:
        e.close()


def test_step_is_run_to_run_deterministic(eng):
    (x,), y = _data(6, 42)
    outs = []
    for _ in range(2):
        _load(eng)
        lo = torch.zeros(1, device="cuda")
        for _ in range(3):
            eng.step_bce(x.cuda(), y.cuda(), [2.0] * C_, 8, lo)
        flat, _ = eng.get_state()
        outs.append((flat.copy(), lo.item()))
    assert outs[0][1] == outs[1][1]
    np.testing.assert_array_equal(outs[0][0], outs[1][0])


@pytest.mark.parametrize("hw,B", [(64, 6), (224, 16)])
def test_stage1_two_stream_step_is_deterministic_and_equals_one_stream(monkeypatch, hw, B):
    """Stage-1 steps enqueue the frozen teacher's forward on a side stream with its own buffers next to the student's
    train forward, and the backward's weight gradients on the side stream next to the data-gradient chain (gradient
    tensors double-buffered by block parity).  Three steps twice from the same state must agree bit for bit (no race
    between the streams), and with the teacher-only / one-stream orders (Engine(streams=2 / 1)) as well."""
    from fedmlp_amd.engine import Engine
    g = torch.Generator().manual_seed(43)
    x1 = torch.randn((B, 3, hw, hw), generator=g); x2 = torch.randn((B, 3, hw, hw), generator=g)
    y = (torch.rand((B, C_), generator=g) < 0.3).float()
    mask = [0.0, 1.0, 0.0, 0.0, 0.0]
    outs = []
    for streams in (0, 0, 2, 1):        # 0 teacher + weight gradients on the side stream, 2 teacher only, 1 one stream
        e = Engine(M, C_, hw, hw, 4 * B, streams=streams)
        try:
            e.stochastic = False
            _load(e)
            e.teacher_snapshot()
            lo = torch.zeros(3, device="cuda")
            for s_ in range(3):
                e.step_stage1(x1.cuda(), x2.cuda(), y.cuda(), mask, 1, B, lo[s_:s_ + 1])
            flat, _ = e.get_state()
            outs.append((flat.copy(), lo.cpu().numpy().copy()))
        finally:
            e.close()
    for k in (1, 2, 3):
        np.testing.assert_array_equal(outs[0][1], outs[k][1])
        np.testing.assert_array_equal(outs[0][0], outs[k][0])


def test_autograd_path_equals_across_stream_modes():
    """The split path -- forward_train, backward_grads with d loss / d feature and both views' input gradients,
    forward_recompute, a second backward_grads, adam_step -- with frozen and with batch statistics, in every stream mode:
    the orders differ only in which stream a launch goes to, so gradients, input gradients, outputs, the state after Adam
    and the counters are the same bits as with side stream for teacher and weight gradients (streams=0)."""
    from fedmlp_amd.engine import Engine
    hw, B = 64, 6
    g = torch.Generator().manual_seed(50)
    x1 = torch.randn((B, 3, hw, hw), generator=g).cuda(); x2 = torch.randn((B, 3, hw, hw), generator=g).cuda()
    dlogits = torch.randn((2 * B, C_), generator=g).cuda()
    dfeat = torch.randn((2 * B, 1280), generator=g).cuda()
    for freeze in (False, True):
        outs = []
        for streams in (0, 1, 2):
            e = Engine(M, C_, hw, hw, 4 * B, streams=streams)
            try:
                e.stochastic = False
                _load(e)
                e.teacher_snapshot()
                e.bn_freeze(freeze)
                feat, logits = e.forward_train(x1, x2)
                dx1, dx2 = torch.empty_like(x1), torch.empty_like(x2)
                e.backward_grads(dlogits, dfeat, dx=(dx1, dx2))
                e.forward_recompute(x1, x2)
                e.backward_grads(dlogits)
                grads = e.grads().cpu().numpy()
                e.adam_step(LR)
                flat, _ = e.get_state()
                outs.append([grads, dx1.cpu().numpy(), dx2.cpu().numpy(), feat.cpu().numpy(), logits.cpu().numpy(), flat.copy(),
                             np.asarray(e.counters()).copy()])
            finally:
                e.close()
        assert np.isfinite(outs[0][0]).all() and np.abs(outs[0][1]).max() > 0
        for k in (1, 2):
            for want, got in zip(outs[0], outs[k]):
                np.testing.assert_array_equal(want, got)


def test_build_model_call_surface():
    """net = build_model(args); net.eval(); feature, logits = net(x) -- the eval-mode call of
    utils/evaluations.py:25 -- for --model Efficient_b0 (feature width 1280)."""
    from fedmlp_amd.model import build_model
    from tests.helpers import make_args
    args = make_args(n_classes=C_, model=M, seed=4, feature_dim=1280)
    net = build_model(args)
    ref = EfficientNetB0Ref(C_)
    ref.load_state_dict({k: torch.as_tensor(np.asarray(v)) for k, v in net.state_dict().items()})
    ref.eval(); net.eval()
    x = torch.randn((3, 3, HW, HW), generator=torch.Generator().manual_seed(8))
    with torch.no_grad():
        f, z = ref(x)
    fe, ze = net(x.cuda())
    assert fe.shape == (3, 1280) and ze.shape == (3, C_)
    np.testing.assert_allclose(fe.cpu().numpy(), f.numpy(), rtol=2e-4, atol=2e-5)
    np.testing.assert_allclose(ze.cpu().numpy(), z.numpy(), rtol=2e-4, atol=2e-5)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_row_blocked_bn_act_passes_are_bit_identical(monkeypatch, precision):
    """FM_EW_ROWS / FM_EW_ROWS_F32: BN + activation apply (bit 0) and backward-apply (bit 1) with four pixels per thread
    and the per-channel parameters loaded once.  Pure re-tiling of an elementwise pass: the same bits after two
    stage-1 steps with both passes row-blocked (3) as with the one-piece-per-thread kernels (0)."""
    from fedmlp_amd.engine import Engine
    e = Engine(M, C_, 96, 96, 16, precision=precision)
    e.stochastic = False
    g = torch.Generator().manual_seed(5)
    x1 = torch.randn((6, 3, 96, 96), generator=g).cuda(); x2 = torch.randn((6, 3, 96, 96), generator=g).cuda()
    y = (torch.rand((6, C_), generator=g) < 0.3).float().cuda()
    outs = []
    try:
        for mode in ("3", "0"):
            monkeypatch.setenv("FM_EW_ROWS" if precision == "bf16" else "FM_EW_ROWS_F32", mode)
            _load(e)
            e.set_stochastic(None, None)
            e.teacher_snapshot()
            lo = torch.zeros(2, device="cuda")
            for s_ in range(2):
                e.step_stage1(x1, x2, y, [0.0, 1.0, 0.0, 0.0, 0.0], 1, 8, lo[s_:s_ + 1])
            flat, _ = e.get_state()
            outs.append((flat.copy(), lo.cpu().numpy().copy(), e.debug_get_grads().copy()))
    finally:
        e.close()
    np.testing.assert_array_equal(outs[0][1], outs[1][1])
    np.testing.assert_array_equal(outs[0][2], outs[1][2])
    np.testing.assert_array_equal(outs[0][0], outs[1][0])


@pytest.mark.parametrize("shape", [(32, 16), (96, 32), (144, 32), (144, 48)])
def test_fused_project_backward_fp32_kernel(shape):
    """pw_proj_bwd_f32_kernel (fp32 storage, blocks 0-3; the 12 x 12 map of the last shape ends with a ragged 16-pixel tile): d a_s = d y_p W formed on the fp32 matrix pipe in both phases;
    phase 0 = the five per-image sums of (d a_s, y_d) + the project conv's weight gradient with a_s = swish(bn1(y_d)) * gate,
    phase 1 = the BN1-backward apply.  Against the same arithmetic in float64 torch (fp32 summation order and the hardware
    exp / rcp of the fp32 build are the only differences)."""
    from fedmlp_amd.engine import Engine
    e = Engine(M, C_, 96, 96, 8)
    try:
        e.stochastic = False
        _load(e)
        L, S = shape
        ci, info = None, None
        for c in range(e.debug_num_convs()):
            i = e.debug_conv_info(c)
            if i["k"] == 1 and i["cin_p"] == L and i["cout_p"] == S and i["cin"] > i["cout"]:
                ci, info = c, i
                break
        assert ci is not None
        flat, cnt = e.get_state()
        sd = spec.flat_to_state_dict(M, C_, flat, cnt)
        ckeys = [k for k, shp, _ in spec.entries(M, C_) if len(shp) == 4 and "_depthwise" not in k and "_se_" not in k]
        W = torch.zeros((S, L), dtype=torch.float64)
        W[:info["cout"], :info["cin"]] = torch.from_numpy(sd[ckeys[ci]].reshape(info["cout"], info["cin"])).double()
        HWo = info["hout"] * info["wout"]
        imgs, groups = 6, 2
        npix = imgs * HWo
        g = torch.Generator().manual_seed(23 + L)
        dyp = torch.randn((npix, S), generator=g) * 0.5
        dyp[:, info["cout"]:] = 0
        yd = torch.randn((npix, L), generator=g)
        bn = torch.empty((7, groups, L))
        bn[0] = torch.rand((groups, L), generator=g) + 0.5
        bn[1] = torch.randn((groups, L), generator=g) * 0.3
        bn[2] = torch.randn((groups, L), generator=g) * 0.2
        bn[3] = torch.rand((groups, L), generator=g) + 0.5
        bn[4] = torch.rand((groups, L), generator=g) + 0.5
        bn[5] = torch.randn((groups, L), generator=g) * 0.1
        bn[6] = torch.randn((groups, L), generator=g) * 0.1
        gate = torch.rand((imgs, L), generator=g)
        ds = torch.randn((imgs, L), generator=g)
        d = (dyp.double() @ W).view(imgs, HWo, L)
        y = yd.double().view(imgs, HWo, L)
        per_img = lambda t: t.double().repeat_interleave(imgs // groups, dim=0)[:, None, :]
        v = y * per_img(bn[0]) + per_img(bn[1])
        sgm = torch.sigmoid(v)
        ad, sg = v * sgm, sgm * (1 + v * (1 - sgm))
        xh = (y - per_img(bn[2])) * per_img(bn[3])
        want5 = torch.stack([(d * ad).sum(1), (d * sg).sum(1), (d * sg * xh).sum(1), sg.sum(1), (sg * xh).sum(1)], dim=1)
        want_dw = dyp.double().t() @ (ad * gate.double()[:, None, :]).view(npix, L)
        want_dy = per_img(bn[4]) * ((d * gate.double()[:, None, :] + ds.double()[:, None, :] / HWo) * sg) + per_img(bn[5]) * y \
            + per_img(bn[6])
        dev = e.device
        dw = torch.empty((S, L), device=dev)
        pool5 = torch.empty((imgs, 5, L), device=dev)
        e.debug_proj_bwd(ci, 0, dyp.to(dev), yd.to(dev), bn.to(dev), gate.to(dev), None, imgs, groups, dw, pool5)
        dy = torch.empty((npix, L), device=dev)
        e.debug_proj_bwd(ci, 1, dyp.to(dev), yd.to(dev), bn.to(dev), gate.to(dev), ds.to(dev), imgs, groups, dy)
        torch.cuda.synchronize()
        e5 = [float((pool5[:, t].cpu().double() - want5[:, t]).abs().max() / want5[:, t].abs().max()) for t in range(5)]
        edw = float((dw.cpu().double() - want_dw).abs().max() / want_dw.abs().max())
        edy = float((dy.cpu().double().view(imgs, HWo, L) - want_dy).abs().max() / want_dy.abs().max())
        assert max(e5) < 2e-5, e5                # fp32 sums of 576-2304 terms, fast exp / rcp (~2 ulp)
        assert edw < 2e-5, edw
        assert edy < 5e-6, edy
    finally:
        e.close()


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("shape", [(96, 16), (144, 32)])
def test_fused_expand_backward_kernel(shape, precision):
    """pw_exp_bwd_f32_kernel / pw_exp_bwd_kernel (blocks 1-3): BN0-backward apply + the expand conv's weight gradient + its data
    gradient (+ skip gradient) from one read of (d a_e, y_e).  Against the same arithmetic in float64 torch on the operands as
    stored (bf16: d y_e is rounded to bf16 before the two products, as the unfused passes store it)."""
    from fedmlp_amd.engine import Engine
    e = Engine(M, C_, 64, 64, 8, precision=precision)
    try:
        e.stochastic = False
        _load(e)
        L, S = shape
        bf = precision == "bf16"
        ci, info = None, None
        for c in range(e.debug_num_convs()):
            i = e.debug_conv_info(c)
            if i["k"] == 1 and i["cout_p"] == L and i["cin_p"] == S and i["cout"] > i["cin"]:
                ci, info = c, i
                break
        assert ci is not None
        flat, cnt = e.get_state()
        sd = spec.flat_to_state_dict(M, C_, flat, cnt)
        ckeys = [k for k, shp, _ in spec.entries(M, C_) if len(shp) == 4 and "_depthwise" not in k and "_se_" not in k]
        W = torch.zeros((L, S), dtype=torch.float64)
        W[:info["cout"], :info["cin"]] = torch.from_numpy(sd[ckeys[ci]].reshape(info["cout"], info["cin"])).double()
        if bf:
            W = W.float().to(torch.bfloat16).double()
        HWi = info["hout"] * info["wout"]
        imgs, groups = 4, 2
        npix = imgs * HWi
        st = torch.bfloat16 if bf else torch.float32
        g = torch.Generator().manual_seed(5 + L)
        da = (torch.randn((npix, L), generator=g) * 0.5).to(st)
        ye = torch.randn((npix, L), generator=g).to(st)
        x = torch.randn((npix, S), generator=g).to(st)
        x[:, info["cin"]:] = 0
        res = (torch.randn((npix, S), generator=g) * 0.3).to(st)
        bn = torch.empty((5, groups, L))
        bn[0] = torch.rand((groups, L), generator=g) + 0.5          # ca
        bn[1] = torch.randn((groups, L), generator=g) * 0.1         # cb
        bn[2] = torch.randn((groups, L), generator=g) * 0.1         # cc
        bn[3] = torch.rand((groups, L), generator=g) + 0.5          # scale
        bn[4] = torch.randn((groups, L), generator=g) * 0.3         # shift
        per_pix = lambda t: t.double().repeat_interleave(npix // groups, dim=0)
        y = ye.double()
        u = y * per_pix(bn[3]) + per_pix(bn[4])
        sg = torch.sigmoid(u)
        dy = per_pix(bn[0]) * (da.double() * (sg * (1 + u * (1 - sg)))) + per_pix(bn[1]) * y + per_pix(bn[2])
        if bf:
            dy = dy.float().to(torch.bfloat16).double()
        want_dw = dy.t() @ x.double()
        want_dx = dy @ W + res.double()
        dev = e.device
        dx = torch.empty((npix, S), dtype=st, device=dev)
        dw = torch.empty((L, S), device=dev)
        e.debug_exp_bwd(ci, da.to(dev), ye.to(dev), x.to(dev), res.to(dev), bn.to(dev), imgs, groups, dx, dw)
        torch.cuda.synchronize()
        edw = float((dw.cpu().double() - want_dw).abs().max() / want_dw.abs().max())
        edx = float((dx.cpu().double() - want_dx).abs().max() / want_dx.abs().max())
        # bf16: d y_e may round the other way after the fast exp / rcp (one 2^-9 step in a 96-144-term sum), dX is stored in bf16
        assert edw < (3e-3 if bf else 2e-5), edw
        assert edx < (1e-2 if bf else 2e-5), edx
    finally:
        e.close()
