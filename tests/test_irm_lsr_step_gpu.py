"""FedLSR / FedIRM above the heads, on a real MI355X: the fused FedLSR step against the split step (bits) and against the autograd
path with a torch head (the bounds of tests/test_autograd_gpu.py's state comparison), the parameters-only teacher blend, and the
two trainers of the drop-in surface on tests/synth.py data."""
import numpy as np
import pytest
import torch

from fedmlp_amd import spec
from fedmlp_amd.model import HipNet
from tests.helpers import make_args
from tests.synth import class_lists

pytestmark = pytest.mark.gpu

HW, B, C_ = 32, 4, 5
LR, WD = 3e-5, 5e-4
PW = [2.0, 1.5, 3.0, 1.0, 2.5]
MODELS = ["Resnet18", "Efficient_b0"]


def _data(seed):
    g = torch.Generator().manual_seed(seed)
    x1 = torch.randn((B, 3, HW, HW), generator=g)
    x2 = x1 + 0.1 * torch.randn((B, 3, HW, HW), generator=g)
    y = (torch.rand((B, C_), generator=g) < 0.4).float()
    return x1.cuda(), x2.cuda(), y.cuda()


def _engine(model, streams):
    from fedmlp_amd.engine import Engine
    e = Engine(model, C_, HW, HW, 2 * B, streams=streams)
    e.stochastic = False                       # EfficientNet-B0: no drop-connect / dropout draws, the same graph on both sides
    e.set_state(*spec.init_state(model, C_, 1037))
    e.adam_reset(LR, (0.9, 0.999), 1e-8, WD)
    return e


@pytest.mark.parametrize("streams", [0, 1])
@pytest.mark.parametrize("model", MODELS)
def test_step_fedlsr_is_the_split_step(model, streams):
    """step_fedlsr leaves the bits that forward_train(x1, x2) + loss_fedlsr + backward_step leave on a twin engine, over two steps"""
    a, b = _engine(model, streams), _engine(model, streams)
    try:
        la, lb = torch.zeros(2, device="cuda"), []
        for step, (mix1, beta) in enumerate(((0.3, 0.4), (0.81, 0.1))):
            x1, x2, y = _data(10 + step)
            a.step_fedlsr(x1, x2, y, PW, mix1, beta, la[step:step + 1])
            _, z = b.forward_train(x1, x2)
            dz, loss = b.loss_fedlsr(z, y, PW, mix1, beta)
            b.backward_step(dz)
            lb.append(loss)
        sa, ca = a.get_state()
        sb, cb = b.get_state()
        assert np.array_equal(sa.view(np.uint32), sb.view(np.uint32)), f"{np.count_nonzero(sa != sb)} of {sa.size} state floats differ"
        assert np.array_equal(ca, cb)
        assert torch.equal(la, torch.cat(lb)) and torch.isfinite(la).all()
    finally:
        a.close()
        b.close()


def _torch_head(z1, z2, y, pw, mix1, beta):
    """train_FedLSR's head as the reference writes it (utils/local_training.py:1296-1314), float32 on the device"""
    q1 = torch.clamp(torch.sigmoid(z1 * 3), min=1e-6, max=1.0)
    q2 = torch.clamp(torch.sigmoid(z2 * 3), min=1e-6, max=1.0)
    p = torch.sigmoid(z1) * mix1 + torch.sigmoid(z2) * (1 - mix1)
    pred_mix = torch.sigmoid(torch.log(p / (1 - p)) * 2)
    loss = torch.nn.BCEWithLogitsLoss(pos_weight=torch.tensor(pw, device=z1.device))(pred_mix, y)
    kl = torch.nn.KLDivLoss(reduction="mean")
    lm = ((q1 + q2) / 2).log()
    return loss + (kl(lm, q1) + kl(lm, q2)) / 2 * beta


def _cmp_state(got, want, model, atol_w):
    """tests/test_autograd_gpu.py's _cmp_state on two flat states: weights rtol 1e-4 and atol_w, running statistics
    1e-5 (max + 1), counters equal"""
    gs = spec.flat_to_state_dict(model, C_, *got)
    ws = spec.flat_to_state_dict(model, C_, *want)
    for k, w in ws.items():
        g, w = np.asarray(gs[k]), np.asarray(w)
        if "num_batches" in k:
            assert int(g) == int(w), k
            continue
        tol = atol_w if ("running" not in k) else 1e-5 * (np.abs(w).max() + 1.0)
        np.testing.assert_allclose(g, w, rtol=1e-4, atol=tol, err_msg=k)


@pytest.mark.parametrize("model", MODELS)
def test_step_fedlsr_against_the_autograd_path(model):
    """one step: net(x1), net(x2), the torch head, loss.backward(), optim.Adam -- against step_fedlsr from the same state on the
    same engine; an Adam step moves a weight by at most lr, so 2.5 lr covers a flipped sign of a near-zero gradient"""
    from fedmlp_amd.optim import Adam
    flat, cnt = spec.init_state(model, C_, 1037)
    net = HipNet(model, C_, flat.copy(), cnt.copy())
    net.default_max_images = 2 * B
    net.train()
    eng = net.bind(HW, HW, 2 * B)
    stochastic = eng.stochastic
    eng.stochastic = False
    eng.set_stochastic(None, None)
    try:
        x1, x2, y = _data(20)
        mix1, beta = 0.37, 0.4
        opt = Adam(net, lr=LR, betas=(0.9, 0.999), weight_decay=WD)
        _, z1 = net(x1)
        _, z2 = net(x2)
        loss = _torch_head(z1, z2, y, PW, mix1, beta)
        opt.zero_grad()
        loss.backward()
        opt.step()
        want = eng.get_state()
        eng.set_state(flat, cnt)
        eng.adam_reset(LR, (0.9, 0.999), 1e-8, WD)
        lf = torch.zeros(1, device="cuda")
        eng.step_fedlsr(x1, x2, y, PW, mix1, beta, lf)
        got = eng.get_state()
    finally:
        eng.stochastic = stochastic
    assert abs(float(lf) - float(loss)) < 1e-4 * abs(float(loss)) + 1e-6, (float(lf), float(loss))
    _cmp_state(got, want, model, atol_w=2.5 * LR)


@pytest.mark.parametrize("model", MODELS)
def test_teacher_ema_params(model):
    """parameters: alpha t + (1 - alpha) s to fp32 rounding (two products and a sum: 3 u of the magnitudes); the teacher's
    running statistics and num_batches_tracked: the same bits"""
    e = _engine(model, 0)
    try:
        s_flat, s_cnt = e.get_state()
        t_flat, t_cnt = spec.init_state(model, C_, 7)
        rs = np.random.RandomState(3)
        t_flat = t_flat.copy()
        off = 0
        stats = np.zeros(t_flat.size, bool)
        for key, shape, dt in spec.entries(model, C_):
            if dt != "f32":
                continue
            n = int(np.prod(shape)) if len(shape) else 1
            if not spec.is_trainable(key):
                stats[off:off + n] = True
                t_flat[off:off + n] = rs.uniform(0.5, 1.5, n).astype(np.float32)      # distinct from the student's 0 / 1
            off += n
        assert off == t_flat.size and stats.any() and not stats.all()
        t_cnt = (np.asarray(t_cnt) + 11).astype(np.int64)
        e.teacher_swap()
        e.set_state(t_flat, t_cnt)
        e.teacher_swap()
        alpha = 0.75
        e.teacher_ema_params(alpha)
        e.teacher_swap()
        got, got_cnt = e.get_state()
        e.teacher_swap()
        s_after, _ = e.get_state()
        assert np.array_equal(s_after.view(np.uint32), s_flat.view(np.uint32))           # the student is only read
        assert np.array_equal(got[stats].view(np.uint32), t_flat[stats].view(np.uint32))
        assert np.array_equal(got_cnt, t_cnt)
        a, b = np.float64(np.float32(alpha)), np.float64(np.float32(1 - alpha))
        t64, s64 = t_flat[~stats].astype(np.float64), s_flat[~stats].astype(np.float64)
        want = a * t64 + b * s64
        bound = 3 * 2.0 ** -24 * (np.abs(a * t64) + np.abs(b * s64)) + 2.0 ** -149
        assert (np.abs(got[~stats].astype(np.float64) - want) <= bound).all()
        assert not np.array_equal(got[~stats], t_flat[~stats])
    finally:
        e.close()


# ---- the trainers ------------------------------------------------------------------------------------------------------------
N, BS = 24, 4


def _client(C, seed, **kw):
    from fedmlp_amd.local_training import LocalUpdate
    from fedmlp_amd.model import build_model
    from tests.test_local_training_gpu import SynthDataset
    args = make_args(n_classes=C, n_clients=1, batch_size=BS, seed=seed, t_w=40, rounds_FedIRM_sup=2, consistency=1,
                     consistency_rampup=30, ema_decay=0.99, **kw)
    ds = SynthDataset(N, C, HW, seed, True)
    assert (ds.targets.sum(0) > 0).all()
    pos, neg = class_lists(ds.targets, C)
    teacher = build_model(make_args(n_classes=C, n_clients=1, seed=seed + 1))
    loc = LocalUpdate(args, 0, ds, list(range(N)), pos, neg, active_class_list=[0], teacher_neg=teacher)
    return loc, build_model(make_args(n_classes=C, n_clients=1, seed=seed)), teacher


def test_train_fedlsr_round():
    loc, net, _ = _client(5, 41)
    np.random.seed(5)                                   # mix_1 comes from numpy's global RNG, like the reference's
    nbt0 = int(net.state_dict()["bn1.num_batches_tracked"])
    for rnd in (0, 3):                                  # beta = 0 in round 0, 0.4 * 3 / 40 in round 3
        out = loc.train_FedLSR(rnd, net)
        assert len(out) == 6 and out[2] is None and out[3] is None
        assert np.isfinite(out[1]) and out[1] > 0
        assert out[4] == [1, 2, 3, 4] and out[5] == [0]
    steps = 2 * (N // BS)
    assert int(out[0]["bn1.num_batches_tracked"]) == nbt0 + 2 * steps      # two views per step
    assert loc.iter_num == steps


@pytest.mark.parametrize("C", [8, 5])
def test_train_fedirm_rounds(C):
    """rounds_FedIRM_sup = 2: round 0 supervised (6-tuple), round 1 supervised with the first relation matrix (7-tuple), round 2
    relation matching against the FedAvg_rela of round 1's matrix (7-tuple)"""
    from fedmlp_amd.fedavg import FedAvg_rela
    loc, net, teacher = _client(C, 43)
    steps = N // BS
    outs = []
    target = None
    for rnd in range(3):
        if rnd == 2:
            before = {k: v.clone() for k, v in net.state_dict().items()}
        out = loc.train_FedIRM(rnd, target, None, None, None, net)
        outs.append(out)
        assert np.isfinite(out[1]), (rnd, out[1])
        if rnd >= 1:
            rel = out[6]
            assert rel.is_cuda and tuple(rel.shape) == (C, C)
            assert bool(((rel > 0) & (rel < 1)).all())
            target = FedAvg_rela([rel.detach().cpu()], [N], [[0]] * C)
            assert bool(torch.isfinite(target).all())
    assert [len(o) for o in outs] == [6, 7, 7]
    assert loc.flag is False and loc.iter_num == steps              # iter_num counts relation-phase steps only (:458)
    after = outs[2][0]
    k = "bn1" if "bn1.running_mean" in after else "_bn0"
    # the student forwards two views per step
    assert int(after[k + ".num_batches_tracked"]) == int(before[k + ".num_batches_tracked"]) + 2 * steps
    # the EMA model started the round as a copy of the student (self.flag) and runs in train mode: one forward per step moves its
    # running statistics and counters, while the parameter blend leaves them alone
    tsd = teacher.state_dict()
    assert int(tsd[k + ".num_batches_tracked"]) == int(before[k + ".num_batches_tracked"]) + steps
    assert not torch.equal(tsd[k + ".running_mean"], before[k + ".running_mean"])
    assert not torch.equal(tsd[k + ".running_mean"], after[k + ".running_mean"])
    w = "conv1.weight"
    assert not torch.equal(tsd[w], before[w]) and not torch.equal(tsd[w], after[w])        # blended towards the student
