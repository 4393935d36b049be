"""RSCFed / FedNoRo / CBAFed above the heads, on a real MI355X: each fused step against the split sequence it replaces (bits:
loss, state, and for RSCFed the teacher's state, after each of three consecutive steps, in both stream modes), CBAFed's device
decisions over a round against the per-step host decisions of the split path (exact), and the three trainers of the drop-in
surface on tests/synth.py data with a tail batch."""
import numpy as np
import pytest
import torch

from fedmlp_amd import spec
from tests.helpers import make_args
from tests.synth import class_lists

pytestmark = pytest.mark.gpu

HW, B, C_ = 32, 5, 5
LR, WD = 3e-5, 5e-4
PW = [2.0, 1.5, 3.0, 1.0, 2.5]
ACT = [0.0, 0.0, 1.0, 0.0, 0.0]
NEG = [0, 1, 3, 4]
ANN, BS = 1, 8
MODELS = ["Resnet18", "Efficient_b0"]
STEPS = 3


def _data(seed):
    g = torch.Generator().manual_seed(seed)
    x1 = torch.randn((B, 3, HW, HW), generator=g)
    x2 = x1 + 0.1 * torch.randn((B, 3, HW, HW), generator=g)
    y = (torch.rand((B, C_), generator=g) < 0.4).float()
    return x1.cuda(), x2.cuda(), y.cuda()


def _engine(model, streams, max_images=2 * B, teacher_seed=None):
    from fedmlp_amd.engine import Engine
    e = Engine(model, C_, HW, HW, max_images, streams=streams)
    e.stochastic = False                       # EfficientNet-B0: no drop-connect / dropout draws, the same graph on both sides
    if teacher_seed is not None:               # a teacher of its own in the teacher slot
        e.set_state(*spec.init_state(model, C_, teacher_seed))
        e.teacher_swap()
    e.set_state(*spec.init_state(model, C_, 1037))
    e.adam_reset(LR, (0.9, 0.999), 1e-8, WD)
    return e


def _teacher_state(e):
    e.teacher_swap()
    s = e.get_state()
    e.teacher_swap()
    return s


def _same_state(a, b, what):
    (sa, ca), (sb, cb) = a, b
    assert np.array_equal(sa.view(np.uint32), sb.view(np.uint32)), f"{what}: {np.count_nonzero(sa != sb)} of {sa.size} state floats differ"
    assert np.array_equal(ca, cb), what


@pytest.mark.parametrize("streams,max_images", [(0, 2 * B), (1, 2 * B), (0, B)], ids=["two_lanes", "one_lane", "staging_for_one_view"])
@pytest.mark.parametrize("model", MODELS)
def test_step_rscfed_is_the_split_step(model, streams, max_images):
    """step_rscfed leaves the bits of forward_eval(x2, teacher) + forward_train(x1) + loss_rscfed + backward_step + teacher_axpby
    on a twin engine: loss, student AND teacher after every step -- a teacher forward that read a stale or half-blended teacher,
    or stale weight packs, would show in step 2's loss"""
    a, b = (_engine(model, streams, max_images, teacher_seed=7) for _ in range(2))
    wt, ws = 0.9, 0.1
    try:
        la = torch.zeros(STEPS, device="cuda")
        for step in range(STEPS):
            x1, x2, y = _data(30 + step)
            a.step_rscfed(x1, x2, y, PW, ACT, ANN, BS, wt, ws, la[step:step + 1])
            _, zt = b.forward_eval(x2, teacher=True)
            _, z = b.forward_train(x1)
            dz, loss = b.loss_rscfed(z, zt, y, PW, ACT, ANN, BS)
            b.backward_step(dz)
            b.teacher_axpby(wt, ws)
            assert torch.equal(la[step:step + 1], loss) and bool(torch.isfinite(loss).all()), (step, la, loss)
            _same_state(a.get_state(), b.get_state(), f"student after step {step}")
            _same_state(_teacher_state(a), _teacher_state(b), f"teacher after step {step}")
        t_end, s_end = _teacher_state(a)[0], a.get_state()[0]
        t0 = spec.init_state(model, C_, 7)[0]
        assert not np.array_equal(t_end, t0) and not np.array_equal(t_end, s_end)      # blended, not replaced
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("streams", [0, 1])
@pytest.mark.parametrize("model", MODELS)
def test_step_fednoro_is_the_split_step(model, streams):
    a, b = _engine(model, streams), _engine(model, streams)
    try:
        a.teacher_snapshot()
        b.teacher_snapshot()
        la = torch.zeros(STEPS, device="cuda")
        for step, w_kd in enumerate((0.8 * 0.0067, 0.3, 0.8)):
            x, _, y = _data(40 + step)
            a.step_fednoro(x, y, ACT, w_kd, la[step:step + 1])
            _, zt = b.forward_eval(x, teacher=True)
            _, z = b.forward_train(x)
            dz, loss = b.loss_lakd(z, zt, y, ACT, w_kd)
            b.backward_step(dz)
            assert torch.equal(la[step:step + 1], loss) and bool(torch.isfinite(loss).all()), (step, la, loss)
            _same_state(a.get_state(), b.get_state(), f"student after step {step}")
        _same_state(_teacher_state(a), _teacher_state(b), "the frozen teacher")
        _same_state(_teacher_state(a), spec.init_state(model, C_, 1037), "the frozen teacher is the snapshot")
    finally:
        a.close()
        b.close()


def _tao_for(e, x):
    """thresholds that split this net's probabilities: per class, the midpoint of the 2nd and 3rd largest of the batch (B = 5), so
    that two rows are above tao; rows below 1 - tao come as they fall"""
    _, z = e.forward_eval(x)
    p = torch.sigmoid(z).cpu().numpy().astype(np.float64)
    srt = np.sort(p, axis=0)
    return [float(np.float32(max(0.5 * (srt[-2, c] + srt[-3, c]), 0.5005))) for c in range(C_)]


@pytest.mark.parametrize("streams", [0, 1])
@pytest.mark.parametrize("model", MODELS)
def test_step_cbafed_is_the_split_step(model, streams):
    """warm-up step, then stage-2 steps; over the stage-2 steps the device's counts and loss_w equal the decisions the trainer
    used to make on the host (torch ops on the logits, an int(tensor.sum()) per class and step), exactly"""
    a, b = _engine(model, streams), _engine(model, streams)
    try:
        pa, pb = (torch.tensor(PW, device="cuda") for _ in range(2))
        ca, cb = (torch.zeros(C_ + 1, dtype=torch.int64, device="cuda") for _ in range(2))
        la = torch.zeros(1 + STEPS, device="cuda")
        x, _, y = _data(50)
        a.step_cbafed(x, y, ACT, ANN, BS, None, pa, ca, la[0:1])
        _, z = b.forward_train(x)
        dz, loss = b.loss_cbafed(z, y, ACT, ANN, BS, None, pb, cb)
        b.backward_step(dz)
        assert torch.equal(la[0:1], loss)
        assert torch.equal(pa, torch.tensor(PW, device="cuda")) and int(ca.sum()) == 0      # the warm-up only reads them
        _same_state(a.get_state(), b.get_state(), "after the warm-up step")
        tao = _tao_for(b, _data(51)[0])
        a.forward_eval(_data(51)[0])                                                        # the twin does what its twin did
        host_w = list(PW)
        host_counts = np.zeros(C_ + 1, np.int64)
        margin = 1.0
        for step in range(1, 1 + STEPS):
            x, _, y = _data(50 + step)
            a.step_cbafed(x, y, ACT, ANN, BS, tao, pa, ca, la[step:step + 1])
            _, z = b.forward_train(x)
            prob = torch.sigmoid(z)
            for i in NEG:                                                                   # utils/local_training.py:303-316
                hi, lo = prob[:, i] > tao[i], prob[:, i] < (1 - tao[i])
                noise_num, clean_num = int(hi.sum()), int(lo.sum())
                n_i = int((hi | lo).sum())
                host_counts[i] += n_i
                host_counts[C_] += n_i
                host_w[i] = 1 if noise_num == 0 else (noise_num + clean_num) / noise_num
                p64 = prob[:, i].double().cpu().numpy()
                margin = min(margin, float(np.abs(p64 - tao[i]).min()), float(np.abs(p64 - (1 - tao[i])).min()))
            host_counts[2] += B
            host_counts[C_] += B * ANN
            dz, loss = b.loss_cbafed(z, y, ACT, ANN, BS, tao, pb, cb)
            b.backward_step(dz)
            assert torch.equal(la[step:step + 1], loss) and bool(torch.isfinite(loss).all()), (step, la, loss)
            _same_state(a.get_state(), b.get_state(), f"student after step {step}")
        assert margin > 1e-6, f"an input probability sits within rounding of a threshold ({margin:.2e}): choose other data"
        assert torch.equal(ca, cb) and np.array_equal(_bits(pa), _bits(pb))
        assert np.array_equal(ca.cpu().numpy(), host_counts), (ca.cpu().numpy(), host_counts)
        assert np.array_equal(pa.cpu().numpy(), np.asarray(host_w, np.float32)), (pa.cpu().numpy(), host_w)
        n_pseudo = int(host_counts[NEG].sum())
        assert 0 < n_pseudo < STEPS * B * len(NEG)            # the decisions were not all alike
    finally:
        a.close()
        b.close()


def _bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("which", ["rscfed", "fednoro", "cbafed"])
def test_fused_steps_refuse_a_requires_grad_mask(which):
    from fedmlp_amd._lib import FmError
    e = _engine("Resnet18", 1)
    try:
        flags = np.ones(len(spec.entries("Resnet18", C_)), np.int32)
        flags[0] = 0                               # conv1.weight frozen
        e.set_trainable(flags)
        x1, x2, y = _data(60)
        lo = torch.zeros(1, device="cuda")
        before = e.get_state()
        with pytest.raises(FmError):
            if which == "rscfed":
                e.step_rscfed(x1, x2, y, PW, ACT, ANN, BS, 0.9, 0.1, lo)
            elif which == "fednoro":
                e.step_fednoro(x1, y, ACT, 0.5, lo)
            else:
                e.step_cbafed(x1, y, ACT, ANN, BS, None, torch.tensor(PW, device="cuda"), None, lo)
        _same_state(e.get_state(), before, "a refused step")
    finally:
        e.close()


# ---- the trainers ------------------------------------------------------------------------------------------------------------
N, BSZ = 22, 4                                  # five full batches and a tail batch of 2


def _client(seed, two_view, **kw):
    from fedmlp_amd.local_training import LocalUpdate
    from fedmlp_amd.model import build_model
    from tests.test_local_training_gpu import SynthDataset
    args = make_args(n_classes=C_, n_clients=1, batch_size=BSZ, seed=seed, **kw)
    ds = SynthDataset(N, C_, HW, seed, two_view)
    assert (ds.targets.sum(0) > 0).all()
    pos, neg = class_lists(ds.targets, C_)
    teacher = build_model(make_args(n_classes=C_, n_clients=1, seed=seed + 1))
    loc = LocalUpdate(args, 0, ds, list(range(N)), pos, neg, active_class_list=[2], teacher_neg=teacher)
    return loc, build_model(make_args(n_classes=C_, n_clients=1, seed=seed)), teacher


def _steps():
    return (N + BSZ - 1) // BSZ


def test_train_rscfed_round():
    loc, net, teacher = _client(61, True)
    t0 = {k: v.clone() for k, v in teacher.state_dict().items()}
    nbt0 = int(net.state_dict()["bn1.num_batches_tracked"])
    for rnd in range(2):
        out = loc.train_RSCFed(rnd, net)
        assert len(out) == 6 and out[2] is None and out[3] is None
        assert np.isfinite(out[1]) and out[1] > 0
        assert out[4] == [0, 1, 3, 4] and out[5] == [2]
    assert int(out[0]["bn1.num_batches_tracked"]) == nbt0 + 2 * _steps()      # one train-mode view per step
    assert loc.iter_num == 2 * _steps() and loc.epoch == 2
    tsd = teacher.state_dict()
    w = "conv1.weight"
    assert not torch.equal(tsd[w], t0[w]) and not torch.equal(tsd[w], out[0][w])   # blended towards the student, every step
    # 0.999^12 of the teacher is still there
    assert float((tsd[w] - t0[w]).abs().max()) < 0.05 * float((out[0][w] - t0[w]).abs().max())


def test_train_fednoro_round():
    loc, net, _ = _client(63, False, rounds_FedNoRo_warmup=3)
    out = loc.train_FedNoRo(0, 1, net, None, weight_kd=0.8 * 0.0067)
    assert len(out) == 6 and out[2] is None and out[3] is None
    assert np.isfinite(out[1]) and out[1] > 0
    assert out[4] == [0, 1, 3, 4] and out[5] == [2]
    assert all(loc.class_num_list[c] == 0 for c in out[4]) and loc.class_num_list[2] > 0      # :136-137
    assert loc.iter_num == _steps() and loc.epoch == 1
    with pytest.raises(NotImplementedError):
        loc.train_FedNoRo(0, 3, net, None, weight_kd=0.1)


def test_train_cbafed_rounds():
    loc, net, _ = _client(65, False, rounds_CBAFed_warmup=1)
    w0 = list(loc.loss_w)
    out = loc.train_CBAFed(0, net)                                             # warm-up
    assert len(out) == 8
    cnum, dnum = out[6], out[7]
    assert isinstance(cnum, torch.Tensor) and cnum.dtype == torch.float32 and tuple(cnum.shape) == (C_,) and not cnum.is_cuda
    assert type(dnum) is int and dnum == N                                     # sum of the actual batch lengths, tail included
    assert cnum.tolist() == [0, 0, N, 0, 0]
    assert loc.loss_w == w0                                                    # the warm-up leaves loss_w alone
    # stage 2 with thresholds the untrained net's probabilities straddle
    eng = loc._bind(net, "image")
    x = loc.dataset.device_views(eng.device)["image"]
    z = torch.cat([eng.forward_eval(x[i:i + 2 * BSZ].contiguous())[1] for i in range(0, N, 2 * BSZ)])
    p = torch.sigmoid(z).cpu().numpy()
    tao = [float(max(np.sort(p[:, c])[-N // 3], 0.5005)) for c in range(C_)]
    seen = []
    real = eng.step_cbafed

    def spy(x, y, am, ann, bs, tao_, pw, counts, loss_out):
        if not seen:
            seen.append(pw.cpu().tolist())
        return real(x, y, am, ann, bs, tao_, pw, counts, loss_out)
    eng.step_cbafed = spy
    try:
        out = loc.train_CBAFed(1, net, pt=None, tao=tao)
        cnum, dnum = out[6], out[7]
        assert len(out) == 8 and np.isfinite(out[1])
        assert isinstance(cnum, torch.Tensor) and cnum.dtype == torch.float32 and tuple(cnum.shape) == (C_,) and not cnum.is_cuda
        assert type(dnum) is int
        assert float(cnum[2]) == N and dnum == int(cnum.sum())                # class_num_list[active] += len(batch); data_num is the total
        assert all(0 <= float(cnum[c]) <= N for c in out[4]) and sum(float(cnum[c]) for c in out[4]) > 0
        assert seen[0] == [float(np.float32(v)) for v in w0]                  # the round started from the client's loss_w
        w1 = list(loc.loss_w)
        assert w1[2] == w0[2] and all(w1[c] >= 1 for c in out[4]) and w1 != w0     # the missing classes' weights were rewritten
        seen.clear()
        loc.train_CBAFed(2, net, pt=None, tao=tao)
        assert seen[0] == [float(np.float32(v)) for v in w1]                  # ... and persist into the next round
    finally:
        del eng.step_cbafed
    assert loc.iter_num == 3 * _steps() and loc.epoch == 3
