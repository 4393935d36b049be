"""tests/eff_ref.py (the float64 yardstick of tests/test_eff_kernels_gpu.py) pinned to torch float64 autograd: the depthwise functions
to F.conv2d(groups = C) after F.pad and its .backward, the squeeze-excite functions to the squeeze-excite part of the oracle's
MBConv block (oracle/efficientnet_ref.py) built in float64.  Everything here is float64 on both sides: 1e-12 relative."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import efficientnet_ref as O
from tests import eff_ref as R

TOL = 1e-12


def _close(name, got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    scale = max(1.0, float(np.abs(want).max()))
    assert np.abs(got - want).max() <= TOL * scale, (name, float(np.abs(got - want).max()))


@pytest.mark.parametrize("size", [(7, 7), (5, 10), (8, 12), (1, 3), (16, 12)], ids=str)
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("K", [3, 5])
def test_depthwise_against_conv2d(K, stride, size):
    H, W = size
    N, C = 3, 8
    rs = np.random.RandomState(K * 100 + stride * 10 + H)
    x, w = rs.standard_normal((N, H, W, C)), rs.standard_normal((K * K, C))
    pt, pl = R.same_pad(H, K, stride), R.same_pad(W, K, stride)
    assert (pt, pl) == (O.same_pad(H, K, stride)[0], O.same_pad(W, K, stride)[0])
    Ho, Wo = R.out_size(H, stride), R.out_size(W, stride)
    dy = rs.standard_normal((N, Ho, Wo, C))
    xt = torch.tensor(x).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    wt = torch.tensor(w).reshape(K, K, C).permute(2, 0, 1).reshape(C, 1, K, K).contiguous().requires_grad_(True)
    _, pb = O.same_pad(H, K, stride)
    _, pr = O.same_pad(W, K, stride)
    y = F.conv2d(F.pad(xt, (pl, pr, pt, pb)), wt, None, stride, 0, 1, C)
    assert tuple(y.shape) == (N, C, Ho, Wo)
    y.backward(torch.tensor(dy).permute(0, 3, 1, 2))
    _close("fwd", R.dw_fwd(x, w, K, stride, pt, pl), y.detach().permute(0, 2, 3, 1).numpy())
    _close("dgrad", R.dw_dgrad(dy, w, K, stride, pt, pl, H, W), xt.grad.permute(0, 2, 3, 1).numpy())
    _close("wgrad", R.dw_wgrad(dy, x, K, stride, pt, pl), wt.grad.reshape(C, K * K).t().numpy())


def test_depthwise_other_padding():
    """the generic kernels serve any (pad_t, pad_l) in 0 .. K-1: here not the TF-"same" one"""
    K, s, N, H, W, C = 3, 1, 2, 6, 5, 4
    rs = np.random.RandomState(5)
    x, w, dy = rs.standard_normal((N, H, W, C)), rs.standard_normal((K * K, C)), rs.standard_normal((N, H, W, C))
    xt = torch.tensor(x).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    wt = torch.tensor(w).reshape(K, K, C).permute(2, 0, 1).reshape(C, 1, K, K).contiguous().requires_grad_(True)
    y = F.conv2d(F.pad(xt, (2, 0, 0, 2)), wt, None, s, 0, 1, C)        # pad_l = 2, pad_t = 0, the remainder right / below
    y.backward(torch.tensor(dy).permute(0, 3, 1, 2))
    _close("fwd", R.dw_fwd(x, w, K, s, 0, 2), y.detach().permute(0, 2, 3, 1).numpy())
    _close("dgrad", R.dw_dgrad(dy, w, K, s, 0, 2, H, W), xt.grad.permute(0, 2, 3, 1).numpy())
    _close("wgrad", R.dw_wgrad(dy, x, K, s, 0, 2), wt.grad.reshape(C, K * K).t().numpy())


def test_fused_statistics_against_autograd():
    """bn_stats = the plain sums; bn0_bwd_sums = the sums of the gradient reaching v = ye scale + shift through swish"""
    G, ipg, H, W, C = 2, 3, 5, 4, 8
    rs = np.random.RandomState(9)
    y = rs.standard_normal((G * ipg, H, W, C))
    st = R.bn_stats(y, G)
    _close("sum", st[:, 0], y.reshape(G, -1, C).sum(1))
    _close("sumsq", st[:, 1], (y ** 2).reshape(G, -1, C).sum(1))
    dx, ye = rs.standard_normal(y.shape), rs.standard_normal(y.shape)
    mean, istd, scale, shift = (rs.standard_normal((G, C)) for _ in range(4))
    v = torch.tensor(ye.reshape(G, -1, C) * scale[:, None] + shift[:, None], requires_grad=True)
    (O.swish(v) * torch.tensor(dx.reshape(G, -1, C))).sum().backward()
    got = R.bn0_bwd_sums(dx, ye, mean, istd, scale, shift, G)
    xhat = (ye.reshape(G, -1, C) - mean[:, None]) * istd[:, None]
    _close("S1", got[:, 0], v.grad.numpy().sum(1))
    _close("S2", got[:, 1], (v.grad.numpy() * xhat).sum(1))
    _close("pool", R.pool_sums(y), y.reshape(G * ipg, -1, C).sum(1))


@pytest.mark.parametrize("shape", [(6, 3, 49, 32, 8), (4, 2, 30, 24, 6), (2, 1, 16, 40, 10)], ids=str)
def test_squeeze_excite_against_oracle_block(shape):
    """forward, gating, backward (dgp, drp, ds), the BN1-backward sums and the weight-gradient range against the oracle block's own
    _se_reduce / _se_expand in float64, with y -> swish(y scale + shift) in front as the train path has it"""
    N, ipg, HW, C, Cs = shape
    G = N // ipg
    rs = np.random.RandomState(N + C)
    blk = O.MBConv(3, 1, 1, 4 * Cs, 4 * Cs).double()                     # cs = cin / 4 = Cs; its depthwise width is replaced by C
    blk._se_reduce, blk._se_expand = O.SameConv(C, Cs, 1).double(), O.SameConv(Cs, C, 1).double()
    W1 = blk._se_reduce.weight.detach().numpy().reshape(Cs, C)
    b1 = blk._se_reduce.bias.detach().numpy()
    W2t = np.ascontiguousarray(blk._se_expand.weight.detach().numpy().reshape(C, Cs).T)
    b2 = blk._se_expand.bias.detach().numpy()
    y, dout = rs.standard_normal((N, HW, C)), rs.standard_normal((N, HW, C))
    scale, shift, mean, istd = (rs.standard_normal((G, C)) for _ in range(4))
    # torch side, NCHW with H = HW, W = 1
    yt = torch.tensor(y).permute(0, 2, 1).reshape(N, C, HW, 1)
    v = (yt * torch.tensor(np.repeat(scale, ipg, 0)).reshape(N, C, 1, 1) + torch.tensor(np.repeat(shift, ipg, 0)).reshape(N, C, 1, 1))
    v.requires_grad_(True)
    x = O.swish(v)
    sq_t = F.adaptive_avg_pool2d(x, 1)
    sq_t.retain_grad()
    rp_t = blk._se_reduce(sq_t)
    rp_t.retain_grad()
    gp_t = blk._se_expand(O.swish(rp_t))
    gp_t.retain_grad()
    out = torch.sigmoid(gp_t) * x
    out.backward(torch.tensor(dout).permute(0, 2, 1).reshape(N, C, HW, 1))

    A = R.se_input(y, scale, shift, ipg)
    sq, rpre, gate = R.se_fwd(A, W1, b1, W2t, b2)
    _close("sq", sq, sq_t.detach().reshape(N, C).numpy())
    _close("rpre", rpre, rp_t.detach().reshape(N, Cs).numpy())
    _close("gate", gate, torch.sigmoid(gp_t).detach().reshape(N, C).numpy())
    _close("pooled", R.se_fwd(A, W1, b1, W2t, b2, pooled=R.pool_sums(A))[2], gate)
    _close("scale", R.se_scale(A, gate), out.detach().reshape(N, C, HW).permute(0, 2, 1).numpy())
    pool5, dgp, drp, ds, bn = R.se_bwd_bn1(dout, y, scale, shift, mean, istd, ipg, gate, rpre, W1, W2t)
    _close("dgp", dgp, gp_t.grad.reshape(N, C).numpy())
    _close("drp", drp, rp_t.grad.reshape(N, Cs).numpy())
    _close("ds", ds * (1.0 / HW), sq_t.grad.reshape(N, C).numpy() * (1.0 / HW))          # (d loss / d sq through the gate branch)
    _close("pool5 R", pool5[:, 0], (dout * A).sum(1))
    again = R.se_bwd_bn1(None, y, scale, shift, mean, istd, ipg, gate, rpre, W1, W2t, pool5=pool5)
    for a, b in zip(again, (pool5, dgp, drp, ds, bn)):
        _close("from pool5", a, b)
    gv = v.grad.reshape(N, C, HW).permute(0, 2, 1).numpy()                  # d loss / d v: both branches
    xh = (y - np.repeat(mean, ipg, 0)[:, None]) * np.repeat(istd, ipg, 0)[:, None]
    _close("S1", bn[:, 0], gv.reshape(G, -1, C).sum(1))
    _close("S2", bn[:, 1], (gv * xh).reshape(G, -1, C).sum(1))
    rng = R.se_wgrad(dgp, drp, rpre, sq)
    o_b1, o_w2, o_b2, n = R.se_range_offsets(C, Cs)
    assert rng.shape == (n,) and n == 2 * Cs * C + (Cs + 3) // 4 * 4 + C
    _close("dW1", rng[:o_b1].reshape(Cs, C), blk._se_reduce.weight.grad.reshape(Cs, C).numpy())
    _close("db1", rng[o_b1:o_b1 + Cs], blk._se_reduce.bias.grad.numpy())
    assert not rng[o_b1 + Cs:o_w2].any()
    _close("dW2", rng[o_w2:o_b2].reshape(Cs, C), blk._se_expand.weight.grad.reshape(C, Cs).t().numpy())
    _close("db2", rng[o_b2:], blk._se_expand.bias.grad.numpy())


def test_bf16_helpers():
    x = np.array([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -20, -3.1415926, 0.0, 2.0 ** -100])
    want = torch.tensor(x, dtype=torch.float32).to(torch.bfloat16).to(torch.float64).numpy()
    assert np.array_equal(R.bf16_round(x), want)                            # ties to even both ways, above a tie, sign, zero
    assert np.array_equal(R.bf16_decode(R.bf16_words(want)).astype(np.float64), want)
    assert R.half_ulp_bf16(1.5) == 2.0 ** -8 and R.half_ulp_bf16(-4.0) == 2.0 ** -6


@pytest.mark.parametrize("a", [0, 1, 2])
@pytest.mark.parametrize("gated", [False, True])
@pytest.mark.parametrize("rowscaled", [False, True])
def test_bnact_passes_against_autograd(rowscaled, gated, a):
    """out = act(bn(y)) rowscale + res with train-mode statistics per group, in float64.  Forward: chan_reduce mode 0 gives the
    statistics, bnact_apply the output.  Backward: the upstream gradient of out = act(bn(y)) rowscale is `up`; with gate / dsv the
    loss is sum up (out gate(mean_HW out)) through a small squeeze-excite, gate its forward value and dsv autograd's gradient at the
    squeeze, and d loss / d y comes from differentiating all of it at once; chan_reduce mode 1
    gives (S1, S2), bn_bwd_coefficients the (ca, cb, cc) of BatchNorm's backward, bnact_bwd_apply d loss / d y.  The backward passes
    serve act 0 and 2 only."""
    G, ipg, HW, C, eps = 2, 3, 5, 8, 1e-3
    n = ipg * HW
    rs = np.random.RandomState(40 + a)
    y, res, up = (rs.standard_normal((G, n, C)) for _ in range(3))
    gamma, beta = rs.standard_normal(C), rs.standard_normal(C)
    rowscale = rs.choice([0.0, 1.25], (G, ipg)) if rowscaled else None
    gate = dsv = None
    st = R.chan_reduce(y, 0)
    mean = st[:, 0] / n
    var = st[:, 1] / n - mean ** 2
    yt = torch.tensor(y, requires_grad=True)
    _close("mean", mean, yt.detach().mean(1).numpy())
    _close("var", var, yt.detach().var(1, unbiased=False).numpy())
    istd = 1.0 / np.sqrt(var + eps)
    scale = gamma * istd
    shift = beta - mean * scale
    v = (yt - yt.mean(1, keepdim=True)) / torch.sqrt(yt.var(1, unbiased=False, keepdim=True) + eps) * torch.tensor(gamma) + torch.tensor(beta)
    o = v if a == 0 else (torch.relu(v) if a == 1 else O.swish(v))
    rs_t = torch.tensor(np.repeat(rowscale, HW, 1)[..., None]) if rowscaled else 1.0
    out = o * rs_t + torch.tensor(res)
    _close("apply", R.bnact_apply(y, scale, shift, HW, a, res, rowscale), out.detach().numpy())
    _close("apply plain", R.bnact_apply(y, scale, shift, HW, a), o.detach().numpy())
    if a == 1:
        return
    d = torch.tensor(up)
    if gated:
        # a squeeze-excite forward on out = act(bn(y)) rowscale, differentiated as a whole: gate is its forward value and dsv is
        # autograd's d loss / d squeeze (the gate path alone, out held constant) -- the fold d gate + dsv / HW is nowhere restated
        Cs = 3
        W1, b1, W2t, b2 = (torch.tensor(rs.standard_normal(sh)) for sh in ((Cs, C), (Cs,), (Cs, C), (C,)))
        gate_of = lambda sq: torch.sigmoid(O.swish(sq @ W1.t() + b1) @ W2t + b2)
        o_rs = o * rs_t
        o_img, up_img = o_rs.reshape(G, ipg, HW, C), d.reshape(G, ipg, HW, C)
        loss = (o_img * gate_of(o_img.mean(2))[:, :, None, :] * up_img).sum()
        gy, d = torch.autograd.grad(loss, [yt, o_rs])                        # d: the gradient reaching out, both branches
        sq = o_img.detach().mean(2).requires_grad_(True)
        dsv, = torch.autograd.grad((o_img.detach() * gate_of(sq)[:, :, None, :] * up_img).sum(), sq)
        gate, dsv = gate_of(sq).detach().numpy(), dsv.numpy()
        assert dsv.any() and (gate > 0).all() and (gate < 1).all()
        yt.grad = gy
    else:
        ((o * rs_t) * d).sum().backward()
    kw = dict(scale=scale, shift=shift, rowscale=rowscale, gate=gate, dsv=dsv)
    sums = R.chan_reduce(y, 1, HW, a, d=up, mean=mean, istd=istd, **kw)
    ca, cb, cc = R.bn_bwd_coefficients(sums, np.broadcast_to(gamma, (G, C)), mean, istd, n)
    _close("bwd_apply", R.bnact_bwd_apply(up, y, ca, cb, cc, HW, a, **kw), yt.grad.numpy())
    # the sums themselves: d loss / d beta and d loss / d gamma per group
    vt = v.detach().requires_grad_(True)
    o2 = vt if a == 0 else O.swish(vt)
    ((o2 * rs_t) * d).sum().backward()
    xh = (y - mean[:, None]) * istd[:, None]
    _close("S1", sums[:, 0], vt.grad.numpy().sum(1))
    _close("S2", sums[:, 1], (vt.grad.numpy() * xh).sum(1))
