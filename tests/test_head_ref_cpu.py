"""tests/head_ref.py (the float64 yardstick of tests/test_head_kernels_gpu.py) pinned to torch autograd on CPU tensors and to the
loss heads of oracle/steps_ref.py.

Float64 against float64 (`p32=False`, smooth logits): 1e-12 relative.  The fp32 semantics of the two BCE-on-probabilities heads
(`p32=True`) are pinned to torch's fp32 ops -- which is what the oracle runs -- on saturated logits, |z| in [20, 80], where they
are determined: z >= 20 gives p = 1, a loss element of 100 (1 - y) and a zero gradient; z <= -20 gives p = fp32(e^z) up to the
ulps of the implementation's exp (T32 = 1e-5 relative leaves room for 40 of them).

On smooth logits fp32 torch differs from the yardstick by its own rounding, allowed for as KT u / min(p, 1 - p) per element
(u = 2^-24), KT = 40, from this count.  exp within 2 ulp, the sum and the division: p within 6 u p.  q = 1 - p: 6 u p + u q <= 7 u / q
relative.  The gradient of BCE on probabilities is ((p - y) / max(p q, eps)) q p: p - y is q or p up to sign, within 7 u / min(p, q);
p q within (7 / q + 7) u <= 14 u / min(p, q); the division, and the two products with q and p once more: 3 u + (7 / q + 6) u.  In all
(7 + 14 + 13) u / min(p, q) + 3 u < 40 u / min(p, q), relative to the gradient.  Terms that cancel (p - q_teacher in stage 1, lw p - lw y
under a pos_weight of 37.5) have an ABSOLUTE error of a few u times the head's largest element gradient, `norm`, so an element is
held to KT u / min(p, q) max(|gradient|, norm).  A loss element, -log p or -log q with |log| < 4.1 here, is within (7 / min(p, q) + 2
4.1 + 1) u, again below KT u / min(p, q), times the element's weight (at most norm); the n-term fp32 sum of non-negative elements
adds n u |loss| < T32 |loss| (n = 84): the loss is held to norm sum(KT u / min(p, q)) + T32 |loss|.  In the saturated band the per-element
figure is T32 in both places."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import steps_ref as O
from tests import head_ref as H

TOL = 1e-12
T32 = 1e-5
KT = 40
U = 2.0 ** -24


def _close(name, got, want, tol=TOL):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    scale = max(1.0, float(np.abs(want).max()))
    assert np.abs(got - want).max() <= tol * scale, (name, float(np.abs(got - want).max()))


def _t(a, dtype=torch.float64, grad=False):
    return torch.tensor(np.asarray(a, np.float64), dtype=dtype, requires_grad=grad)


def _sat(rs, shape):
    """|z| in [20, 80], either sign"""
    return rs.uniform(20, 80, shape) * rs.choice([-1.0, 1.0], shape)


def test_head_against_autograd():
    rs = np.random.RandomState(1)
    imgs, HW, D, C = 5, 6, 20, 7
    x = rs.standard_normal((imgs, HW, D))
    W, b, dz = rs.standard_normal((C, D)), rs.standard_normal(C), rs.standard_normal((imgs, C))
    mask = (rs.rand(imgs, D) < 0.7) / 0.7
    dfeat = rs.standard_normal((imgs, D))
    for use_mask in (False, True):
        for use_dfeat in (False, True):
            xt, Wt, bt = _t(x, grad=True), _t(W, grad=True), _t(b, grad=True)
            feature = xt.mean(1)
            h = feature * _t(mask) if use_mask else feature
            logits = h @ Wt.t() + bt
            L = (logits * _t(dz)).sum() + ((feature * _t(dfeat)).sum() if use_dfeat else 0.0)
            L.backward()
            _close("avgpool", H.avgpool(x), feature.detach().numpy())
            hn = h.detach().numpy()
            _close("fc_fwd", H.fc_fwd(hn, W, b), logits.detach().numpy())
            dW, db, dpix = H.fc_bwd(dz, hn, W, HW, mask if use_mask else None, dfeat if use_dfeat else None)
            _close("dW", dW, Wt.grad.numpy())
            _close("db", db, bt.grad.numpy())
            _close("dout", np.broadcast_to(dpix[:, None, :], x.shape), xt.grad.numpy())


@pytest.mark.parametrize("shape", [(1, 5), (7, 14), (52, 32)], ids=str)
def test_loss_elements_against_autograd_float64(shape):
    rs = np.random.RandomState(shape[0])
    z, y = rs.uniform(-8, 8, shape), (rs.rand(*shape) < 0.4).astype(np.float64)
    pw = rs.choice([1.0, 0.05, 37.5], shape[1])
    zt = _t(z, grad=True)
    l = F.binary_cross_entropy_with_logits(zt, _t(y), pos_weight=_t(pw), reduction="none")
    l.sum().backward()
    got = H.bce_logits(z, y, pw[None, :])
    _close("bce_logits", got[0], l.detach().numpy())
    _close("bce_logits dz", got[1], zt.grad.numpy())
    zt = _t(z, grad=True)
    l = F.binary_cross_entropy(torch.sigmoid(zt), _t(y), reduction="none")
    l.sum().backward()
    got = H.bce_prob(z, y, p32=False)
    _close("bce_prob", got[0], l.detach().numpy(), 1e-11)         # 1 - sigmoid(z) loses 3 digits at z = 8 on torch's side
    _close("bce_prob dz", got[1], zt.grad.numpy(), 1e-11)


def test_bce_prob_fp32_semantics_against_torch_fp32():
    """saturated logits: the clamp at -100, p (1 - p) = 0 under the 1e-12 guard and p below 1e-12 are all reached and determined"""
    rs = np.random.RandomState(3)
    z = np.concatenate([_sat(rs, 400), [20.0, -20.0, 80.0, -80.0, 27.0, -27.0, -28.0, -40.0]])
    y = (rs.rand(z.size) < 0.5).astype(np.float64)
    zt = _t(z, torch.float32, grad=True)
    l = F.binary_cross_entropy(torch.sigmoid(zt), _t(y, torch.float32), reduction="none")
    l.sum().backward()
    got_l, got_d = H.bce_prob(z.astype(np.float32), y)
    lt, dt = l.detach().numpy().astype(np.float64), zt.grad.numpy().astype(np.float64)
    up = z >= 20
    assert np.array_equal(got_l[up], 100.0 * (1 - y[up])) and not got_d[up].any()
    assert np.array_equal(lt[up], got_l[up]) and not dt[up].any()
    assert np.abs(got_l - lt).max() <= T32 * 100.0
    assert (np.abs(got_d - dt) <= T32 * np.maximum(np.abs(dt), 1e-30)).all()
    assert (np.abs(got_d[(z < -35) & (y == 1)]) < 1e-3).all() and (np.abs(got_d[(z > -27) & (z < 0) & (y == 1)] + 1) < 1e-6).all()


def _active(kind, C):
    return {"all": np.ones(C), "none": np.zeros(C), "alt": (np.arange(C) % 2).astype(np.float64)}[kind]


@pytest.mark.parametrize("kind", ["all", "none", "alt"])
@pytest.mark.parametrize("band", ["smooth", "saturated"])
def test_loss_heads_against_oracle(band, kind):
    """loss_train, loss_stage1, loss_stage2, loss_fixmatch (with the fixmatch_mask row set) of oracle/steps_ref.py, value and
    autograd gradient, in fp32 as the oracle runs them"""
    rs = np.random.RandomState(11)
    B, C, bs_norm = 7, 6, 9
    gen = (lambda sh: rs.uniform(-4, 4, sh)) if band == "smooth" else (lambda sh: _sat(rs, sh))
    f32 = lambda a: np.asarray(a, np.float32).astype(np.float64)
    z, g, y = f32(gen((2 * B, C))), f32(gen((2 * B, C))), (rs.rand(B, C) < 0.4).astype(np.float64)
    pw, pwu = f32(rs.choice([1.0, 0.05, 37.5], C)), f32(rs.choice([1.0, 0.05, 37.5], C))
    active = _active(kind, C)
    act, neg = [c for c in range(C) if active[c]], [c for c in range(C) if not active[c]]
    ann = max(len(act), 1)

    def tol(zz):
        """per-element allowance for torch's own fp32 rounding (module docstring)"""
        if band == "saturated":
            return np.full(zz.shape, T32)
        p = H.sigmoid(zz)
        return KT * U / np.minimum(p, 1 - p)

    def compare(name, got, want_loss, zt, norm, zz):
        """norm = the largest gradient of an element of this head (weight times normaliser)"""
        t = tol(zz)
        dt = zt.grad.numpy().astype(np.float64)
        scale = np.maximum(np.abs(dt), norm)
        print(f"{name}: worst gradient err / allowance {float((np.abs(got[1] - dt) / (t * scale)).max()):.3f}, "
              f"loss {abs(got[0] - want_loss.item()) / (t.sum() * norm + T32 * abs(want_loss.item())):.3f}")
        assert (np.abs(got[1] - dt) <= t * scale).all(), (name, float((np.abs(got[1] - dt) / (t * scale)).max()))
        assert abs(got[0] - want_loss.item()) <= t.sum() * norm + T32 * abs(want_loss.item()), (name, got[0], want_loss.item())

    # train
    zt = _t(z[:B], torch.float32, grad=True)
    want = O.loss_train(zt, _t(y, torch.float32), pw, bs_norm, C)
    want.backward()
    compare("train", H.loss_bce(z[:B], y, pw, 1.0 / (bs_norm * C)), want, zt, 40.0 / (bs_norm * C), z[:B])
    # stage 1: with every class annotated the oracle's distillation term is 0 / 0, and its supervised term is the whole loss;
    # with none annotated (annotation_num 1) the supervised term is an empty sum
    zt = _t(z, torch.float32, grad=True)
    want = O.loss_stage1(zt[:B], zt[B:], _t(g[:B], torch.float32), _t(g[B:], torch.float32), _t(y, torch.float32), act, neg,
                         bs_norm, ann)
    assert neg or torch.isnan(want[2])
    want = want[0] if neg else want[1]
    want.backward()
    compare("stage1", H.loss_stage1(z, g, y, active, 1.0 / (bs_norm * ann), 1.0 / (bs_norm * len(neg)) if neg else 0.0), want, zt,
            1.0 / bs_norm, z)
    # stage 2
    for frac in (0.0, 0.5):
        distill = (rs.rand(B, C) < frac).astype(np.float64) * rs.choice([1.0, -1.0, 2.0], (B, C))
        zt = _t(z[:B], torch.float32, grad=True)
        want = O.loss_stage2(zt, _t(y, torch.float32), _t(distill, torch.float32))
        want.backward()
        compare("stage2", H.loss_stage2(z[:B], y, distill), want, zt, 1.0 / (B * C), z[:B])
    # fixmatch (bs_norm = B: the oracle seeds its row set with range(bs_norm))
    zt = _t(z, torch.float32, grad=True)
    want = O.loss_fixmatch(zt[:B], zt[B:], _t(y, torch.float32), pw, pwu, act, neg, B, ann, C)
    assert O.fixmatch_mask(zt[:B].detach(), neg, B) == list(np.flatnonzero(H.fixmatch_conf(z[:B], active)))
    if act or (neg and H.fixmatch_conf(z[:B], active).any()):
        want.backward()
        compare("fixmatch", H.loss_fixmatch(z, y, pw, pwu, active, 1.0 / (B * ann), C - ann), want, zt, 40.0 / B, z)


def test_stage2_all_distilled_is_nan():
    z, y = np.zeros((3, 4)), np.ones((3, 4))
    loss, dz = H.loss_stage2(z, y, np.ones((3, 4)))
    assert np.isnan(loss) and np.isnan(dz).all()
    with torch.no_grad():
        assert torch.isnan(O.loss_stage2(_t(z, torch.float32), _t(y, torch.float32), torch.ones(3, 4)))


def test_fixmatch_gate_thresholds_and_arms():
    """weak logits on either side of 0.2 / 0.8 / 0.5 (delta = 2^-6); no confident row, no missing class, every row confident"""
    d, t = 2.0 ** -6, np.log(4.0)                       # logit(0.8) = log 4
    C, active = 4, np.array([1.0, 0.0, 1.0, 0.0])
    rows = [[0.0, t + d, 0.0, -(t + d)], [0.0, t - d, 0.0, -(t + d)], [0.0, t + d, 0.0, -(t - d)], [0.0, d, 0.0, t + d],
            [0.0, -d, 0.0, -(t + d)], [0.0, 30.0, 0.0, -30.0]]
    zw = np.array(rows)
    assert list(H.fixmatch_conf(zw, active)) == [True, False, False, False, False, True]
    assert list(np.flatnonzero(H.fixmatch_conf(zw, active))) == O.fixmatch_mask(_t(zw, torch.float32), [1, 3], 6)
    rs = np.random.RandomState(5)
    z = np.concatenate([zw, rs.standard_normal(zw.shape)], 0)
    y = (rs.rand(6, C) < 0.5).astype(np.float64)
    pw = np.array([1.0, 0.05, 37.5, 1.0])
    loss, dz = H.loss_fixmatch(z, y, pw, pw[::-1], active, 0.25, 2)
    assert not dz[6:][~H.fixmatch_conf(zw, active)].any() and not dz[6:, [0, 2]].any() and dz[6, 1] != 0 and not dz[:6, [1, 3]].any()
    # no confident row: the supervised part alone
    z2 = z.copy(); z2[:6, 1] = 0.5
    assert not H.fixmatch_conf(z2[:6], active).any()
    l2, d2 = H.loss_fixmatch(z2, y, pw, pw, active, 0.25, 2)
    assert not d2[6:].any() and l2 == H.bce_logits(z2[:6], y, pw[None, :])[0][:, [0, 2]].sum() * 0.25
    # no missing class: every row passes the gate, and nothing is unsupervised
    l3, d3 = H.loss_fixmatch(z, y, pw, pw, np.ones(C), 0.25, 0)
    assert H.fixmatch_conf(zw, np.ones(C)).all() and not d3[6:].any() and np.isfinite(l3)
    # every class missing and every row confident
    z4 = z.copy(); z4[:6] = 30.0 * np.sign(rs.standard_normal((6, C)))
    l4, d4 = H.loss_fixmatch(z4, y, pw, pw, np.zeros(C), 0.25, C)
    assert H.fixmatch_conf(z4[:6], np.zeros(C)).all() and d4[6:].all() and not d4[:6].any()
