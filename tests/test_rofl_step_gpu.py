"""RoFL above the head, on a real MI355X: step_rofl against the split sequence forward_train -> loss_rofl -> backward_step (bits:
loss, state, centroids and label table after each of three steps, both models, both stream modes), its refusal under a
requires_grad mask, and train_RoFL against tests/rofl_ref.py driving the autograd path (net(x), the torch head, loss.backward(),
optim.Adam) in the same batch order, at the tolerance of tests/test_irm_lsr_step_gpu.py's autograd comparison: loss 1e-4
relative, weights rtol 1e-4 and 2.5 lr per Adam step, running statistics 1e-5, counters equal."""
import types

import numpy as np
import pytest
import torch

from fedmlp_amd import spec
from tests import rofl_ref as R
from tests.helpers import make_args
from tests.synth import class_lists

pytestmark = pytest.mark.gpu

HW, B, C_ = 32, 8, 5
LR, WD = 3e-5, 5e-4
PW = [2.0, 5.0, 3.0, 5.0, 2.5]
MODELS = ["Resnet18", "Efficient_b0"]
STEPS = 3
NT = 13                                           # rows of the label table


def _data(seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((B, 3, HW, HW), generator=g)
    y = (torch.rand((B, C_), generator=g) < 0.4).float()
    item = torch.randperm(NT, generator=g)[:B].to(torch.int32)
    return x.cuda(), y.cuda(), item.cuda()


def _engine(model, streams):
    from fedmlp_amd.engine import Engine
    e = Engine(model, C_, HW, HW, 2 * B, streams=streams)
    e.stochastic = False                       # EfficientNet-B0: no drop-connect / dropout draws, the same graph on both sides
    e.set_state(*spec.init_state(model, C_, 1037))
    e.adam_reset(LR, (0.9, 0.999), 1e-8, WD)
    return e


def _client_state(e, seed):
    g = torch.Generator().manual_seed(seed)
    f_k = torch.randn((2 * C_, e.feature_dim), generator=g).cuda()
    pseudo = (torch.rand((NT, C_), generator=g) < 0.5).to(torch.uint8).cuda()
    return f_k, pseudo


def _same_state(a, b, what):
    (sa, ca), (sb, cb) = a, b
    assert np.array_equal(sa.view(np.uint32), sb.view(np.uint32)), f"{what}: {np.count_nonzero(sa != sb)} of {sa.size} state floats differ"
    assert np.array_equal(ca, cb), what


@pytest.mark.parametrize("streams", [0, 1])
@pytest.mark.parametrize("model", MODELS)
def test_step_rofl_is_the_split_step(model, streams):
    a, b = _engine(model, streams), _engine(model, streams)
    try:
        (fa, pa), (fb, pb) = _client_state(a, 5), _client_state(b, 5)
        f0, p0 = fa.clone(), pa.clone()
        la = torch.zeros(STEPS, device="cuda")
        n = R.n_keep(0.2, B)
        for step in range(STEPS):
            x, y, item = _data(70 + step)
            wl, lam = step < 2, 0.25 * step
            a.step_rofl(x, y, item, n, PW, lam, 0.8, wl, fa, pa, la[step:step + 1])
            f, z = b.forward_train(x)
            dz, loss = b.loss_rofl(z, f, y, item, n, PW, lam, 0.8, wl, fb, pb)
            b.backward_step(dz)
            assert torch.equal(la[step:step + 1], loss) and bool(torch.isfinite(loss).all()), (step, la, loss)
            assert int((dz != 0).any(1).sum()) == n
            _same_state(a.get_state(), b.get_state(), f"after step {step}")
            assert np.array_equal(fa.cpu().numpy().view(np.uint32), fb.cpu().numpy().view(np.uint32)), step
            assert torch.equal(pa, pb), step
        assert not torch.equal(fa, f0) and not torch.equal(pa, p0) and bool(torch.isfinite(fa).all())
    finally:
        a.close()
        b.close()


def test_step_rofl_refuses_a_requires_grad_mask():
    from fedmlp_amd._lib import FmError
    e = _engine("Resnet18", 1)
    try:
        flags = np.ones(len(spec.entries("Resnet18", C_)), np.int32)
        flags[0] = 0                               # conv1.weight frozen
        e.set_trainable(flags)
        x, y, item = _data(60)
        f_k, pseudo = _client_state(e, 6)
        f0, p0 = f_k.clone(), pseudo.clone()
        lo = torch.zeros(1, device="cuda")
        before = e.get_state()
        with pytest.raises(FmError, match="requires_grad mask"):
            e.step_rofl(x, y, item, 6, PW, 1.0, 0.8, True, f_k, pseudo, lo)
        _same_state(e.get_state(), before, "a refused step")         # the BatchNorm counters with it
        assert torch.equal(f_k, f0) and torch.equal(pseudo, p0)
        e.set_trainable(np.ones(len(flags), np.int32))
        with pytest.raises(FmError, match="n_keep < 1"):
            e.step_rofl(x, y, item, 0, PW, 1.0, 0.8, True, f_k, pseudo, lo)
        _same_state(e.get_state(), before, "a refused step")
    finally:
        e.close()


# ---- the trainer -------------------------------------------------------------------------------------------------------------
N, BSZ = 20, 8                                    # two full batches and a tail of 4
T_PL = 3


def _args(seed):
    return make_args(n_classes=C_, n_clients=1, batch_size=BSZ, seed=seed, base_lr=LR, forget_rate=0.2, T_pl=T_PL,
                     lambda_cen=1.0, lambda_e=0.8)


def _client(seed, n=N):
    from fedmlp_amd.local_training import LocalUpdate
    from fedmlp_amd.model import build_model
    from tests.test_local_training_gpu import SynthDataset

    class InOrder(LocalUpdate):
        def _order(self, n):                      # the loader's order, fixed: the reference side walks the same batches
            return list(range(n))
    ds = SynthDataset(n, C_, HW, seed, False)
    assert (ds.targets.sum(0) > 0).all()
    pos, neg = class_lists(ds.targets, C_)
    neg = [p[::2] for p in neg]                   # every other positive of a missing class is masked: the others stay 1
    loc = InOrder(_args(seed), 0, ds, list(range(n)), pos, neg, active_class_list=[2])
    return loc, build_model(make_args(n_classes=C_, n_clients=1, seed=seed))


class _HostSide:
    """the autograd path behind a net that takes and returns CPU tensors (rofl_ref works on the host)"""

    def __init__(self, net):
        self.net = net

    def eval(self):
        self.net.eval()

    def train(self):
        self.net.train()

    def __call__(self, x):
        f, z = self.net(x.cuda())
        return f.cpu(), z.cpu()


def _cmp_state(got, want, atol_w):
    for k, w in want.items():
        g, w = np.asarray(got[k]), np.asarray(w)
        if "num_batches" in k:
            assert int(g) == int(w), k
            continue
        tol = atol_w if ("running" not in k) else 1e-5 * (np.abs(w).max() + 1.0)
        np.testing.assert_allclose(g, w, rtol=1e-4, atol=tol, err_msg=k)


def _reference_round(seed, epoch, f_G):
    """-> (losses, f_k, tables, margins, state_dict, loss_w) of rofl_ref.train_round on the autograd path"""
    from fedmlp_amd.optim import Adam
    loc, net = _client(seed)
    net.train()
    opt = Adam(net, lr=LR, betas=(0.9, 0.999), weight_decay=WD)
    x = loc.dataset.x1
    y = torch.from_numpy(loc._y_masked)
    batches = [(x[i:i + BSZ], y[i:i + BSZ], torch.arange(i, min(i + BSZ, N))) for i in range(0, N, BSZ)]
    a = types.SimpleNamespace(n_classes=C_, local_ep=1, forget_rate=0.2, T_pl=T_PL, lambda_cen=1.0, lambda_e=0.8)
    loss_w = list(loc.loss_w)
    out = R.train_round(_HostSide(net), opt, batches, f_G, epoch, loss_w, [2], a)
    return out + ({k: v.clone() for k, v in net.state_dict().items()}, loss_w)


@pytest.mark.parametrize("epoch", [0, T_PL + 1], ids=["epoch0", "past_T_pl"])
def test_train_rofl_against_the_reference_on_the_autograd_path(epoch):
    """20 samples at batch 8 (tail 4), one local epoch.  The data seed is the first of four whose float64 margins hold (votes
    and keep boundaries 1e-4 from a tie on the reference side's features and logits); with none the test fails."""
    f_G = torch.randn((2 * C_, 512), generator=torch.Generator().manual_seed(3))
    for seed in (81, 82, 83, 84):
        losses, f_k, tables, margin, want_sd, want_w = _reference_round(seed, epoch, f_G)
        print(f"seed {seed}: margins {margin}")
        if min(m[0] for m in margin) >= 1e-4 and min(m[1] for m in margin) >= 1e-4:
            break
    else:
        pytest.fail(f"no seed keeps the decisions 1e-4 from a tie: {margin}")
    loc, net = _client(seed)
    w0 = {k: v.clone() for k, v in net.state_dict().items()}
    sd, mean, got_fk = loc.train_RoFL(net, f_G.clone(), epoch)
    assert len(losses) == 3 and loc.iter_num == 3 and loc.epoch == 1
    assert abs(mean - np.mean(losses)) < 1e-4 * abs(np.mean(losses)) + 1e-6, (mean, losses)
    assert loc.loss_w == want_w and [loc.loss_w[c] for c in (0, 1, 3, 4)] == [5.0] * 4
    assert isinstance(got_fk, torch.Tensor) and not got_fk.is_cuda and tuple(got_fk.shape) == (2 * C_, 512)
    np.testing.assert_allclose(got_fk.numpy(), f_k.numpy(), rtol=1e-4, atol=1e-5 * float(f_k.abs().max()))
    _cmp_state(sd, want_sd, atol_w=2.5 * LR * 3)
    assert not torch.equal(got_fk, f_G)
    # 7.5 lr is as wide as three Adam steps move a weight, so the UPDATES are compared too: over the conv / fc weights both sides
    # moved the same way.  An Adam step is lr m / (sqrt(v) + eps), about lr sign(g) in the first steps, so two fp32 evaluations of
    # one gradient differ in an element's direction only where |g| is within their rounding of 0 -- a fraction far below 1 %;
    # 95 % leaves room for that, and weights that were not trained, or trained on another head, agree in about half
    agree = total = 0
    for k, w in want_sd.items():
        if w.dim() < 2:
            continue
        dg, dw = (sd[k] - w0[k]).double(), (w - w0[k]).double()
        moved = dw != 0
        agree += int(((dg * dw) > 0)[moved].sum())
        total += int(moved.sum())
    print(f"update directions: {agree} of {total} agree ({agree / total:.4f})")
    assert total > 1e6 and agree >= 0.95 * total, (agree, total)


def test_train_rofl_label_table_and_steps(monkeypatch):
    """the round's label table after the last step is the reference side's, exactly; the steps got the host's n_keep, the
    ramped lambda_cen and write_labels = epoch < T_pl"""
    epoch = 1
    f_G = torch.randn((2 * C_, 512), generator=torch.Generator().manual_seed(4))
    for seed in (85, 86, 87, 88):
        losses, f_k, tables, margin, _, _ = _reference_round(seed, epoch, f_G)
        if min(m[0] for m in margin) >= 1e-4 and min(m[1] for m in margin) >= 1e-4:
            break
    else:
        pytest.fail(f"no seed keeps the decisions 1e-4 from a tie: {margin}")
    loc, net = _client(seed)
    eng = loc._bind(net, "image")
    calls = []
    real = eng.step_rofl

    def spy(x, y, item, n_keep, pw, lam_cen, lam_e, wl, centroids, pseudo, loss_out):
        real(x, y, item, n_keep, pw, lam_cen, lam_e, wl, centroids, pseudo, loss_out)
        calls.append((x.shape[0], n_keep, lam_cen, lam_e, wl, pseudo.cpu().clone()))
    monkeypatch.setattr(eng, "step_rofl", spy, raising=False)
    loc.train_RoFL(net, f_G, epoch)
    assert [c[:5] for c in calls] == [(8, 6, 1.0 * 1 / T_PL, 0.8, True)] * 2 + [(4, 3, 1.0 * 1 / T_PL, 0.8, True)]
    for step in range(3):
        assert torch.equal(calls[step][5], tables[step]), step


def test_train_rofl_skips_a_tail_of_one():
    """17 samples at batch 8: the tail of 1 keeps int(0.8 * 1) = 0 rows; it is skipped, counted in neither the loss mean nor
    iter_num, and moves no BatchNorm counter"""
    loc, net = _client(91, n=17)
    nbt0 = int(net.state_dict()["bn1.num_batches_tracked"])
    sd, mean, f_k = loc.train_RoFL(net, None, 0)
    assert np.isfinite(mean) and mean > 0 and bool(torch.isfinite(f_k).all())
    assert loc.iter_num == 2
    assert int(sd["bn1.num_batches_tracked"]) == nbt0 + 2
    assert all(bool(torch.isfinite(v).all()) for v in sd.values())
