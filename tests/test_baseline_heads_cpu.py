"""The host side of the RSCFed / FedNoRo / CBAFed clients, without a GPU: the driver's parser, CBAFed's tao and residual-blend
schedule against the reference's lines (main.py:273-316) written out with torch, the rank-independent DMA draw, the float32 pin
of tests/baseline_heads_ref.py to oracle/steps_ref.py, and the new symbols of the built library."""
import random

import numpy as np
import pytest
import torch

from oracle import steps_ref as O
from tests import baseline_heads_ref as R


# ---- the driver's parser ----------------------------------------------------------------------------------------------------------
def test_parser_accepts_the_three_baselines_and_their_flags():
    from fedmlp_amd.driver import args_parser
    for exp in ("RSCFed", "FedNoRo", "CBAFed"):
        assert args_parser(["--exp", exp]).exp == exp
    a = args_parser([])
    assert (a.rounds_FedNoRo_warmup, a.begin, a.end, a.a, a.rounds_CBAFed_warmup) == (500, 10, 499, 0.8, 50)    # utils/options.py:73-79
    a = args_parser(["--exp", "FedNoRo", "--rounds_FedNoRo_warmup", "7", "--rounds_warmup", "7", "--begin", "1", "--end", "5",
                     "--a", "0.25", "--rounds_CBAFed_warmup", "3"])
    assert (a.rounds_FedNoRo_warmup, a.begin, a.end, a.a, a.rounds_CBAFed_warmup) == (7, 1, 5, 0.25, 3)
    assert isinstance(a.begin, int) and isinstance(a.a, float)
    with pytest.raises(SystemExit):
        args_parser(["--exp", "RoFL"])                      # commented out in the reference's main.py


def test_parser_errors(capsys):
    from fedmlp_amd.driver import args_parser
    with pytest.raises(SystemExit):
        args_parser(["--exp", "RSCFed", "--n_clients", "5"])            # groups of 6
    assert "n_clients" in capsys.readouterr().err
    assert args_parser(["--exp", "RSCFed", "--n_clients", "6"]).n_clients == 6
    assert args_parser(["--exp", "FedAVG", "--n_clients", "5"]).n_clients == 5          # the other rows are not concerned
    with pytest.raises(SystemExit):
        args_parser(["--exp", "FedNoRo", "--rounds_warmup", "11", "--rounds_FedNoRo_warmup", "10"])
    assert "rounds_FedNoRo_warmup" in capsys.readouterr().err
    assert args_parser(["--exp", "FedNoRo", "--rounds_warmup", "10", "--rounds_FedNoRo_warmup", "10"]).rounds_warmup == 10
    assert args_parser(["--exp", "CBAFed", "--rounds_warmup", "600"]).rounds_warmup == 600


def test_dma_draw_is_the_same_on_every_rank():
    """main.py:114-120 from one random.Random(seed): two instances (two ranks) draw the same groups, round after round, whatever
    the ranks drew from the global generator in between"""
    from fedmlp_amd.driver import RSCFED_K, RSCFED_M
    assert (RSCFED_M, RSCFED_K) == (10, 6)
    a, b = random.Random(1037), random.Random(1037)
    random.seed(1)
    for rnd in range(4):
        da = [a.sample(range(8), RSCFED_K) for _ in range(RSCFED_M)]
        random.random()                                                  # rank-local draws do not touch it
        db = [b.sample(range(8), RSCFED_K) for _ in range(RSCFED_M)]
        assert da == db
        assert all(len(set(g)) == RSCFED_K and max(g) < 8 for g in da)
    assert da != [random.Random(1038).sample(range(8), RSCFED_K) for _ in range(RSCFED_M)]


# ---- CBAFed's host arithmetic -------------------------------------------------------------------------------------------------
def test_cbafed_tao_is_the_references():
    from fedmlp_amd.fedavg import cbafed_tao
    g = torch.Generator().manual_seed(4)
    for C, n_clients in ((5, 3), (8, 8), (2, 1)):
        class_num_lists = [torch.randint(0, 200, (C,), generator=g).float() for _ in range(n_clients)]
        data_nums = [int(torch.randint(200, 900, (1,), generator=g)) for _ in range(n_clients)]
        # main.py:290-300
        c_num = torch.zeros(C)
        d_num = 0
        for s in range(n_clients):
            c_num += class_num_lists[s]
            d_num += data_nums[s]
        pt = c_num / d_num
        avg_pt = pt.sum() / len(pt)
        std_pt = torch.sqrt((1 / (len(pt) - 1)) * (((pt - avg_pt) ** 2).sum()))
        tao = pt + 0.45 - std_pt
        tao = torch.where(tao > 0.95, 0.95, tao)
        tao = torch.where(tao < 0.55, 0.55, tao)
        got_pt, got_tao = cbafed_tao(class_num_lists, data_nums)
        assert torch.equal(got_pt, pt) and torch.equal(got_tao, tao)
        assert bool(((got_tao >= 0.55) & (got_tao <= 0.95)).all())
        assert torch.allclose(std_pt, pt.std())                          # the unbiased standard deviation
    # both clips bind: std = 0.354, so 0 + 0.45 - std < 0.55 and 1 + 0.45 - std > 0.95
    pt, tao = cbafed_tao([torch.tensor([0.0] + [100.0] * 7)], [100])
    assert float(tao[0]) == pytest.approx(0.55) and float(tao[1]) == pytest.approx(0.95)


def test_cbafed_blend_schedule_is_the_references():
    """rounds 0-12 with a warm-up of 6: main.py:274-288 and :301-316 on one-tensor 'models', against cbafed_blend"""
    from fedmlp_amd.fedavg import cbafed_blend
    W = 6
    g = torch.Generator().manual_seed(9)
    fedavg_out = [torch.randn(7, generator=g) for _ in range(13)]
    # the reference's lines
    want, res_log = [], []
    w_glob_res = None
    for rnd in range(13):
        w_glob_fl = fedavg_out[rnd].clone()
        if rnd < W:
            if rnd % 5 != 0:
                pass
            elif rnd == 0:
                w_glob_res = w_glob_fl.clone()
            else:
                w_glob_fl = 0.2 * w_glob_fl + 0.8 * w_glob_res
                w_glob_res = w_glob_fl.clone()
        if rnd >= W:
            if (rnd - W) % 5 != 0:
                pass
            elif (rnd - W) == 0:
                w_glob_res = w_glob_fl.clone()
            else:
                w_glob_fl = 0.5 * w_glob_fl + 0.5 * w_glob_res
                w_glob_res = w_glob_fl.clone()
        want.append(w_glob_fl)
        res_log.append(w_glob_res.clone())
    # the driver's form
    res = None
    sched = []
    for rnd in range(13):
        w_new, w_res, store = cbafed_blend(rnd, W)
        sched.append((w_new, w_res, store))
        m = fedavg_out[rnd].clone()
        if w_res != 0.0:
            m = m.mul_(w_new).add_(res * w_res)
        if store:
            res = m.clone()
        assert torch.equal(m, want[rnd]), rnd
        assert torch.equal(res, res_log[rnd]), rnd
    plain, keep = (1.0, 0.0, False), (1.0, 0.0, True)
    assert sched == [keep, plain, plain, plain, plain, (0.2, 0.8, True),          # warm-up: res set at 0, 0.2 / 0.8 at 5
                     keep, plain, plain, plain, plain, (0.5, 0.5, True), plain]   # stage 2: res reset at 6, 0.5 / 0.5 at 11
    assert cbafed_blend(10, 50) == (0.2, 0.8, True) and cbafed_blend(50, 50) == keep and cbafed_blend(60, 50) == (0.5, 0.5, True)


# ---- the float64 yardstick's restatement is the oracle's arithmetic ----------------------------------------------------------------
def _oracle(fn, z, *args):
    zz = torch.tensor(z, dtype=torch.float32).requires_grad_(True)
    loss = fn(zz, *args)
    (dz,) = torch.autograd.grad(loss, zz)
    return np.float64(loss.detach().numpy()), dz.numpy().astype(np.float64)


@pytest.mark.parametrize("bc", [(3, 5), (67, 14), (1, 2)], ids=str)
def test_restatement_is_the_oracle_in_float32(bc):
    B, C = bc
    rs = np.random.RandomState(11 * B + C)
    act = [C // 2]
    neg = [c for c in range(C) if c not in act]
    f = lambda a: torch.tensor(a, dtype=torch.float32)                    # noqa: E731
    z = rs.uniform(-8, 8, (B, C)).astype(np.float32)
    zt = rs.uniform(-8, 8, (B, C)).astype(np.float32)
    y = (rs.rand(B, C) < 0.4).astype(np.float32)
    pw = rs.choice([1.0, 0.05, 37.5], C).astype(np.float32)
    tao = rs.uniform(0.55, 0.95, C).astype(np.float32)

    def same(got, want):
        assert got[0] == want[0] and np.array_equal(got[1], want[1])

    same(R.loss_rscfed(z, zt, y, pw, act, neg, 32, 1, dtype=torch.float32),
         _oracle(lambda zz: O.loss_rscfed(zz, f(zt), f(y), pw.tolist(), act, neg, 32, 1), z))
    same(R.loss_la_kd(z, zt, y, act, neg, 0.3, dtype=torch.float32),
         _oracle(lambda zz: O.loss_la_kd(zz, f(zt), f(y), act, neg, 0.3), z))
    same(R.loss_cbafed_stage1(z, y, pw, act, 32, 1, dtype=torch.float32),
         _oracle(lambda zz: O.loss_cbafed_stage1(zz, f(y), pw.tolist(), act, 32, 1), z))
    labels, idx_neg, loss_w, _ = O.cbafed_stage2_targets(torch.sigmoid(f(z)), f(y), neg, tao.tolist(), pw.tolist())
    same(R.loss_cbafed_stage2(z, labels.numpy(), idx_neg, loss_w, act, neg, 32, 1, dtype=torch.float32),
         _oracle(lambda zz: O.loss_cbafed_stage2(zz, labels, idx_neg, loss_w, act, neg, 32, 1), z))


# ---- the library ---------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_exported():
    from fedmlp_amd import _lib
    lib = _lib.load()
    for name in ("fm_loss_rscfed", "fm_loss_lakd", "fm_loss_cbafed", "fm_step_rscfed", "fm_step_fednoro", "fm_step_cbafed"):
        assert name in _lib.SYMBOLS
        assert getattr(lib, name) is not None
