"""RoFL on the CPU: the dtype-generic restatement tests/rofl_ref.py against the reference's own get_small_loss_samples, RFLloss and
train_RoFL (tests/golden/rofl_kat.npz, recorded by tests/golden/make_rofl_golden.py), its dz against finite differences and
autograd, fedavg.rofl_centroids against a float64 evaluation of the server step, and the n_keep arithmetic."""
import os
import types

import numpy as np
import pytest
import torch

from tests import rofl_ref as R

KAT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rofl_kat.npz")
T_PL, LAMBDA_CEN, LAMBDA_E, FORGET, LR = 4, 1.0, 0.8, 0.2, 1e-3         # make_rofl_golden.py's settings
ACTIVE = [2]


@pytest.fixture(scope="module")
def kat():
    return dict(np.load(KAT))


def _t(a, dtype=torch.float64):
    return torch.from_numpy(np.asarray(a)).to(dtype)


def test_small_loss_selection_is_the_reference_s(kat):
    z, y = _t(kat["fn_z"]), _t(kat["fn_y"])
    w = _t(kat["fn_loss_w_out"])
    n = R.n_keep(FORGET, z.shape[0])
    keep = R.kept_rows(R.row_loss(z, y, w), n)
    assert torch.nonzero(keep).flatten().tolist() == kat["fn_kept"].tolist()
    # loss_w[missing] = 5.0, the active class's weight untouched
    want = kat["fn_loss_w_in"].copy()
    want[[c for c in range(5) if c not in ACTIVE]] = 5.0
    assert kat["fn_loss_w_out"].tolist() == want.tolist()


@pytest.mark.parametrize("name", ["ramp", "flat"])
def test_rfl_loss_is_the_reference_s(kat, name):
    """float64 against float64: 1e-12 relative covers the two forms of the entropy (p log p, and softplus(z) - z p) at |z| <= 4"""
    z, y, feat, f_k = (_t(kat[k]) for k in ("fn_z", "fn_y", "fn_feat", "fn_fk"))
    keep = torch.zeros(z.shape[0], dtype=torch.bool)
    keep[_t(kat["fn_kept"], torch.long)] = True
    mask = _t(kat["fn_mask"]) != 0
    lam = R.lambda_cen_eff(LAMBDA_CEN, int(kat["fn_epoch_" + name]), T_PL)
    got = R.rfl_loss(z, y, feat, f_k, mask, keep, _t(kat["fn_new"]), _t(kat["fn_loss_w_out"]), lam, LAMBDA_E)
    want = float(kat["fn_rfl_" + name])
    assert abs(float(got) - want) <= 1e-12 * abs(want), (float(got), want)
    assert float(kat["fn_rfl_ramp"]) != float(kat["fn_rfl_flat"])               # the ramp of lambda_cen is in the fixture


class _Net(torch.nn.Module):
    """the recording's stand-in: 12 inputs -> tanh(Linear) feature of 16 -> Linear logits"""

    def __init__(self, kat, dtype):
        super().__init__()
        self.body = torch.nn.Linear(12, 16)
        self.fc = torch.nn.Linear(16, 5)
        self.load_state_dict({k[len("tr_w0_"):]: torch.from_numpy(v) for k, v in kat.items() if k.startswith("tr_w0_")})
        self.to(dtype)

    def forward(self, x):
        f = torch.tanh(self.body(x))
        return f, self.fc(f)


def _round(kat, name, dtype):
    net = _Net(kat, dtype)
    opt = torch.optim.Adam(net.parameters(), lr=LR, betas=(0.9, 0.999), weight_decay=5e-4)
    x, y = _t(kat["tr_x"], dtype), _t(kat["tr_y"], dtype)
    batches = [(x[i:i + 8], y[i:i + 8], torch.arange(i, min(i + 8, 20))) for i in range(0, 20, 8)]
    a = types.SimpleNamespace(n_classes=5, local_ep=1, forget_rate=FORGET, T_pl=T_PL, lambda_cen=LAMBDA_CEN, lambda_e=LAMBDA_E)
    loss_w = kat["fn_loss_w_in"].tolist()
    out = R.train_round(net, opt, batches, _t(kat["tr_fG"], dtype), int(kat[f"tr_{name}_epoch"]), loss_w, ACTIVE, a)
    return net, loss_w, out


@pytest.mark.parametrize("name", ["e0", "eT"])
def test_train_round_is_the_reference_s(kat, name):
    """One whole train_RoFL call (batches of 8, 8 and a tail of 4) at epoch 0 and at epoch = T_pl with a given f_G.  The
    recording is fp32; the restatement runs in fp32 too.  Label tables: exact (the float64 run asserts that no decision is within
    1e-4 of a tie).  Losses, f_k and weights: 1e-4 relative -- three Adam steps of fp32 chains a few hundred operations long,
    each good to 2^-24, summed in another order than the reference's loops."""
    _, _, (_, _, tables64, margin) = _round(kat, name, torch.float64)
    assert len(margin) == 3 and min(m[0] for m in margin) >= 1e-4 and min(m[1] for m in margin) >= 1e-4, margin
    net, loss_w, (losses, f_k, tables, _) = _round(kat, name, torch.float32)
    want_tables = kat[f"tr_{name}_tables"]
    for step in range(3):
        assert np.array_equal(tables[step].numpy(), want_tables[step]), step
        assert np.array_equal(tables64[step].numpy(), want_tables[step]), step
    np.testing.assert_allclose(losses, kat[f"tr_{name}_losses"], rtol=1e-4)
    np.testing.assert_allclose(f_k.numpy(), kat[f"tr_{name}_fk"], rtol=1e-4, atol=1e-6)
    for k, v in net.state_dict().items():
        np.testing.assert_allclose(v.numpy(), kat[f"tr_{name}_w_{k}"], rtol=1e-4, atol=1e-6, err_msg=k)
    assert loss_w == kat[f"tr_{name}_loss_w"].tolist()
    if name == "e0":        # epoch < T_pl: the kept rows' labels were written into the table
        assert not np.array_equal(want_tables[0], want_tables[2])


def _head_inputs(seed, B=8, C=5, D=16, N=11):
    g = torch.Generator().manual_seed(seed)
    z = 4 * torch.rand((B, C), generator=g, dtype=torch.float64) - 2
    y = (torch.rand((B, C), generator=g) < 0.4).double()
    feat = torch.randn((B, D), generator=g, dtype=torch.float64)
    f_k = torch.randn((2 * C, D), generator=g, dtype=torch.float64)
    item = torch.randperm(N, generator=g)[:B]
    pseudo = (torch.rand((N, C), generator=g) < 0.5).to(torch.uint8)
    w = torch.tensor([2.5, 5.0, 3.0, 5.0, 1.0], dtype=torch.float64)
    return z, feat, y, item, w, f_k, pseudo


@pytest.mark.parametrize("write_labels", [False, True])
def test_dz_is_the_gradient_of_the_loss(write_labels):
    """the stated dz against central differences of the float64 loss (h = 1e-6: truncation ~ h^2 |f'''| ~ 1e-12, rounding
    ~ 2^-53 |loss| / h ~ 1e-10) and against autograd; exact zeros off the kept rows"""
    z, feat, y, item, w, f_k, pseudo = _head_inputs(3)
    n = R.n_keep(FORGET, z.shape[0])
    assert R.margins(z, feat, y, n, w, f_k)[1] > 1e-3           # the kept set is the same at z +- h
    zz = z.clone().requires_grad_(True)
    r = R.head(zz, feat, y, item, n, w, 0.75, LAMBDA_E, write_labels, f_k, pseudo)
    (auto,) = torch.autograd.grad(r["loss"], zz)
    assert float((auto - r["dz"]).abs().max()) < 1e-15
    h = 1e-6
    fd = torch.zeros_like(z)
    for i in range(z.shape[0]):
        for c in range(z.shape[1]):
            zp, zm = z.clone(), z.clone()
            zp[i, c] += h
            zm[i, c] -= h
            lp = R.head(zp, feat, y, item, n, w, 0.75, LAMBDA_E, write_labels, f_k, pseudo)["loss"]
            lm = R.head(zm, feat, y, item, n, w, 0.75, LAMBDA_E, write_labels, f_k, pseudo)["loss"]
            fd[i, c] = (lp - lm) / (2 * h)
    assert float((fd - r["dz"]).abs().max()) < 1e-9, float((fd - r["dz"]).abs().max())
    assert int(r["keep"].sum()) == n and bool((r["dz"][~r["keep"]] == 0).all()) and bool((r["dz"][r["keep"]] != 0).all())


def test_entropy_form_is_finite_and_is_the_entropy():
    z = torch.tensor([-120.0, -30.0, -3.0, 0.0, 2.0, 17.0, 120.0], dtype=torch.float64)
    p = torch.sigmoid(z[1:5])
    plain = -(p * p.log() + (1 - p) * (1 - p).log())
    assert float((R.entropy(z)[1:5] - plain).abs().max()) < 1e-15
    assert bool(torch.isfinite(R.entropy(z)).all()) and bool(torch.isfinite(R.entropy(z.float())).all())
    assert float(R.entropy(z)[0]) < 1e-40 and float(R.entropy(z)[-1]) == 0.0


def test_ties_go_to_the_lower_row_and_nan_sorts_last():
    loss = torch.tensor([3.0, 1.0, float("nan"), 1.0, 2.0, 1.0])
    assert torch.nonzero(R.kept_rows(loss, 2)).flatten().tolist() == [1, 3]
    assert torch.nonzero(R.kept_rows(loss, 5)).flatten().tolist() == [0, 1, 3, 4, 5]


def test_centroid_update_leaves_a_row_without_samples_alone():
    z, feat, y, item, w, f_k, pseudo = _head_inputs(5)
    y[:, 1] = 0.0                                                # no kept row carries label 1 of class 1
    keep = torch.ones(8, dtype=torch.bool)
    new = R.centroid_update(feat, y, keep, f_k)
    assert torch.equal(new[3], f_k[3]) and not torch.equal(new[2], f_k[2])
    # a row of zeros (round 0, a label value the client never saw) has cosine 0 with everything: it stays zero
    f_k[2] = 0
    assert torch.equal(R.centroid_update(feat, y, keep, f_k)[2], f_k[2])
    assert float(R.cosine(f_k[2:3], feat[:1])) == 0.0


def test_round_start_zero_count_row_is_zero():
    g = torch.Generator().manual_seed(1)
    feat, logits = torch.randn((6, 4), generator=g), torch.randn((6, 3), generator=g)
    labels = torch.tensor([[0, 1, 0], [0, 0, 1], [0, 1, 1], [0, 0, 0], [0, 1, 0], [0, 0, 1]], dtype=torch.float32)
    pseudo, f_k = R.round_start(feat, logits, labels)
    assert torch.equal(f_k[1], torch.zeros(4)) and torch.allclose(f_k[0], feat.mean(0))
    assert torch.equal(pseudo, (logits > 0).to(torch.uint8))


def test_rofl_centroids():
    """fedavg.rofl_centroids (fp32) against part C in float64.  Row 0: the clients' cosines are exactly +1 and -1, a zero
    weight sum that divides by 1; row 1: one negative weight in a sum that stays positive.  Bound per element: the cosines
    carry (D + 4) roundings, the fold 2 per client; 2 (D + 6) 2^-24 of sum_i |w_i f_i| / |sum_i w_i|, amplified by
    sum |w| / |sum w| where the weights cancel."""
    from fedmlp_amd.fedavg import rofl_centroids
    g = torch.Generator().manual_seed(9)
    C, D = 3, 16
    f_G = torch.randn((2 * C, D), generator=g)
    locs = [f_G + 0.5 * torch.randn((2 * C, D), generator=g) for _ in range(3)]
    f_G[0] = 0
    f_G[0, 0] = 1.0
    for f, v in zip(locs, (2.0, -2.0, 0.0)):
        f[0] = 0
        f[0, 0] = v                                              # cos = +1, -1, and 0 (a zero row)
    locs[1][1] = -locs[1][1]                                     # cos < 0 for client 1 in row 1
    before = f_G.clone()
    got = rofl_centroids(f_G, locs)
    assert got.dtype == torch.float32 and torch.equal(f_G, before)
    want = R.server_centroids(f_G.double(), [f.double() for f in locs])
    w = torch.stack([R.cosine(f_G.double(), f.double()) for f in locs])           # [clients, rows]
    assert float(w[:, 0].sum()) == 0.0 and float(w[1, 1]) < 0 < float(w[:, 1].sum())
    assert torch.equal(got[0], torch.tensor([4.0] + [0.0] * (D - 1)))               # (1 * 2 + -1 * -2 + 0) / 1
    den = torch.where(w.sum(0) == 0, torch.ones(2 * C, dtype=torch.float64), w.sum(0).abs())
    mag = sum(w[i].abs()[:, None] * locs[i].double().abs() for i in range(3)) / den[:, None]
    bound = 2 * (D + 6) * 2.0 ** -24 * mag * (w.abs().sum(0) / den).clamp(min=1)[:, None]
    err = (got.double() - want).abs()
    assert bool((err <= bound).all()), float((err / bound.clamp(min=1e-300)).max())
    assert torch.equal(rofl_centroids(f_G, [np.asarray(f) for f in locs]), got)    # array-likes are taken too


def test_n_keep_arithmetic():
    """int((1 - forget_rate) * B) in Python double arithmetic: 0.8 * 5 is 4.0 exactly, 0.8 * 128 = 102.4"""
    assert [R.n_keep(0.2, B) for B in (1, 5, 8, 128)] == [0, 4, 6, 102]
    assert [R.n_keep(0.0, B) for B in (1, 5, 8, 128)] == [1, 5, 8, 128]
    assert [R.n_keep(0.5, B) for B in (1, 5, 8, 128)] == [0, 2, 4, 64]


def test_skipping_a_batch_leaves_it_out_of_the_epoch():
    """LocalUpdate._epochs(skip=...): a skipped batch gets no step and no loss slot, so the epoch's mean is over the others"""
    from fedmlp_amd.local_training import LocalUpdate
    lu = LocalUpdate.__new__(LocalUpdate)
    lu.args = types.SimpleNamespace(local_ep=2, batch_size=4)
    lu.idxs = list(range(9))
    lu.epoch = 0
    lu._order = lambda n: list(range(n))
    eng = types.SimpleNamespace(device="cpu")
    epoch_loss, seen = [], []
    for batches in lu._epochs(eng, epoch_loss, skip=lambda pos: len(pos) < 2):
        for pos, slot in batches:
            seen.append(list(pos))
            slot[:] = float(len(seen))
    assert seen == [[0, 1, 2, 3], [4, 5, 6, 7]] * 2 and epoch_loss == [1.5, 3.5] and lu.epoch == 2


def test_driver_rofl_parser():
    """python -m fedmlp_amd.driver_rofl: the driver's flags with exp = RoFL and the reference's defaults (utils/options.py:53-57)"""
    from fedmlp_amd import driver_rofl
    a = driver_rofl.args_parser([])
    assert (a.exp, a.forget_rate, a.T_pl, a.lambda_cen, a.lambda_e) == ("RoFL", 0.2, 100, 1.0, 0.8)
    a = driver_rofl.args_parser(["--forget_rate", "0.1", "--T_pl", "3", "--lambda_cen", "0.5", "--lambda_e", "0.25", "--n_clients", "4"])
    assert (a.forget_rate, a.T_pl, a.lambda_cen, a.lambda_e, a.n_clients) == (0.1, 3, 0.5, 0.25, 4)
    assert isinstance(a.T_pl, int)
    with pytest.raises(SystemExit):
        driver_rofl.args_parser(["--exp", "FedAVG"])
