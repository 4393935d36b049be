"""tests/bn_ref.py -- the float64 yardstick of tests/test_bn_kernels_gpu.py -- against torch float64 autograd: train-mode
F.batch_norm with its running update, F.max_pool2d(F.relu(.), 3, 2, 1) with its argmax, and the backward of their composite, on
random inputs and on inputs full of exact ties and exact zeros.  Also the plane encode / decode and the share of discrete
decisions the GPU tests leave out at their seeds."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import bn_ref as R

EPS = 1e-5


def _nchw(a):
    return torch.from_numpy(np.ascontiguousarray(np.moveaxis(a, -1, 1)))


def _nhwc(t):
    return np.moveaxis(t.detach().numpy(), 1, -1)


def _inputs(kind, seed, N=3, H=8, W=12, C=8):
    rs = np.random.RandomState(seed)
    if kind == "random":
        y = rs.standard_normal((N, H, W, C))
        gamma, beta = rs.standard_normal(C), rs.standard_normal(C)
        dp = rs.standard_normal((N, H // 2, W // 2, C))
    else:       # few distinct values: windows tie all the time, and beta = 0 with symmetric y puts pre-activations exactly on 0
        y = rs.randint(-1, 2, (N, H, W, C)).astype(np.float64)
        y[0, :, :, 0] = 1.0                                    # an all-equal map: every window ties everywhere
        gamma = np.array([1.0, 0.5, -0.5, 0.0, 2.0 ** -6, 1.5, 1.0, 1.0])[:C]
        beta = np.array([0.0, 0.0, 0.5, 1.0, 0.0, -1.0, 0.0, 0.5])[:C]
        dp = rs.randint(-32, 33, (N, H // 2, W // 2, C)) / 8.0
    return y, gamma, beta, dp


@pytest.mark.parametrize("kind", ["random", "ties"])
def test_batch_norm_statistics_and_running_update(kind):
    """two groups = two consecutive train-mode forwards on the same module"""
    y, gamma, beta, _ = _inputs(kind, 1, N=4)
    G, ipg = 2, 2
    C = y.shape[-1]
    yg = y.reshape(G, -1, C)
    count = yg.shape[1]
    rs = np.random.RandomState(2)
    rm0, rv0 = rs.standard_normal(C), rs.uniform(0.5, 2.0, C)
    for tiles in (1, 5):
        got = R.bn_finalize(R.tile_stats(yg, tiles), count, gamma, beta, EPS, 0.1, rm0, rv0)
        rm, rv = torch.from_numpy(rm0.copy()), torch.from_numpy(rv0.copy())
        for g in range(G):
            x = _nchw(y[g * ipg:(g + 1) * ipg])
            want = F.batch_norm(x, rm, rv, torch.from_numpy(gamma), torch.from_numpy(beta), True, 0.1, EPS)
            mine, _, _ = R.bn_apply(yg[g:g + 1], got["scale"][g:g + 1], got["shift"][g:g + 1], relu=False)
            np.testing.assert_allclose(mine.reshape(ipg, *y.shape[1:]), _nhwc(want), rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(got["run_mean"], rm.numpy(), rtol=1e-13, atol=1e-14)
        np.testing.assert_allclose(got["run_var"], rv.numpy(), rtol=1e-13, atol=1e-14)
    kept = R.bn_finalize(R.tile_stats(yg, 3), count, gamma, beta, EPS, 0.1, rm0, rv0, skip=True)
    assert np.array_equal(kept["run_mean"], rm0) and np.array_equal(kept["run_var"], rv0)
    np.testing.assert_allclose(kept["scale"], got["scale"], rtol=1e-13)
    # count = 1: the unbiased factor is skipped (variance 0 stays 0); a negative variance is clamped
    one = R.bn_finalize(np.array([[[[3.0], [9.0]]]]), 1, [1.0], [0.0], EPS, 0.1, [0.0], [1.0])
    assert one["var"][0, 0] == 0.0 and one["run_var"][0] == 0.9 and np.isclose(one["run_mean"][0], 0.3)
    neg = R.bn_finalize(np.array([[[[8.0], [15.9]]]]), 4, [1.0], [0.0], EPS)
    assert neg["var"][0, 0] == 0.0 and neg["istd"][0, 0] == 1.0 / np.sqrt(EPS)
    fz = R.bn_frozen(2, gamma, beta, rm0, rv0, EPS)
    want = F.batch_norm(_nchw(y), torch.from_numpy(rm0.copy()), torch.from_numpy(rv0.copy()), torch.from_numpy(gamma),
                        torch.from_numpy(beta), False, 0.1, EPS)
    mine, _, _ = R.bn_apply(yg, fz["scale"], fz["shift"], relu=False)
    np.testing.assert_allclose(mine.reshape(y.shape), _nhwc(want), rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("kind", ["random", "ties"])
def test_max_pool_choice_rule(kind):
    y, gamma, beta, _ = _inputs(kind, 3)
    N, H, W, C = y.shape
    pre = y * gamma + beta
    pooled, code, margin, _ = R.stem_pool(y, gamma[None], beta[None], ipg=N)
    want, ind = F.max_pool2d(F.relu(_nchw(pre)), 3, 2, 1, return_indices=True)
    assert np.array_equal(pooled, _nhwc(want))
    oh, ow = np.arange(H // 2)[None, :, None, None], np.arange(W // 2)[None, None, :, None]
    flat = (2 * oh - 1 + code // 3) * W + (2 * ow - 1 + code % 3)
    assert np.array_equal(flat, _nhwc(ind))                       # torch's CPU max-pool keeps the first maximum too
    if kind == "ties":
        assert (margin == 0).mean() > 0.5
        assert code[0, 0, 0, 0] == 4 and code[0, 0, 1, 0] == 3 and code[0, 1, 0, 0] == 1 and code[0, 1, 1, 0] == 0
        assert code[..., 3].min() >= 0 and (code[:, 1:, 1:, 3] == 0).all()      # gamma = 0: every window is all-equal
    plain, pcode, _, _ = R.stem_pool(y)
    want, ind = F.max_pool2d(_nchw(y), 3, 2, 1, return_indices=True)
    assert np.array_equal(plain, _nhwc(want))
    assert np.array_equal((2 * oh - 1 + pcode // 3) * W + (2 * ow - 1 + pcode % 3), _nhwc(ind))


@pytest.mark.parametrize("kind", ["random", "ties"])
def test_composite_backward(kind):
    """d/dy, d/dgamma, d/dbeta of sum(dp * maxpool(relu(batch_norm(y)))) per group, groups summed into dgamma / dbeta"""
    y, gamma, beta, dp = _inputs(kind, 5, N=4)
    N, H, W, C = y.shape
    G, ipg = 2, 2
    yg = y.reshape(G, -1, C)
    count = yg.shape[1]
    fin = R.bn_finalize(R.tile_stats(yg, 2), count, gamma, beta, EPS)
    pooled, code, _, _ = R.stem_pool(y, fin["scale"], fin["shift"], ipg=ipg)
    dense = R.pool_route(dp, pooled, code, H, W).reshape(G, -1, C)
    s1, s2, _, _ = R.bn_bwd_sums(dense, yg, fin["mean"], fin["istd"])
    # the fused form's sums: over the pooled positions, xhat of y at each argmax
    gp = np.where(pooled > 0, dp, 0.0).reshape(G, -1, C)
    ya = R.gather_argmax(y, code).reshape(G, -1, C)
    f1, f2, _, _ = R.bn_bwd_sums(gp, ya, fin["mean"], fin["istd"])
    np.testing.assert_allclose(f1, s1, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(f2, s2, rtol=1e-12, atol=1e-12)
    co = R.bn_bwd_coeffs(s1, s2, count, gamma, fin["mean"], fin["istd"])
    dy, _ = R.bn_bwd_apply(dense, yg, co["ca"], co["cb"], co["cc"])

    yt = _nchw(y).requires_grad_(True)
    ga, be = torch.from_numpy(gamma).requires_grad_(True), torch.from_numpy(beta).requires_grad_(True)
    loss = 0
    for g in range(G):
        z = F.batch_norm(yt[g * ipg:(g + 1) * ipg], None, None, ga, be, True, 0.1, EPS)
        loss = loss + (F.max_pool2d(F.relu(z), 3, 2, 1) * _nchw(dp[g * ipg:(g + 1) * ipg])).sum()
    loss.backward()
    np.testing.assert_allclose(dy.reshape(y.shape), _nhwc(yt.grad), rtol=1e-10, atol=1e-10)
    np.testing.assert_allclose(co["dgamma"], ga.grad.numpy(), rtol=1e-10, atol=1e-10)
    np.testing.assert_allclose(co["dbeta"], be.grad.numpy(), rtol=1e-10, atol=1e-10)
    # frozen statistics: eval-mode batch_norm
    fz = R.bn_frozen(G, gamma, beta, fin["mean"][0], fin["var"][0], EPS)
    pooled, code, _, _ = R.stem_pool(y, fz["scale"], fz["shift"], ipg=ipg)
    dense = R.pool_route(dp, pooled, code, H, W).reshape(G, -1, C)
    s1, s2, _, _ = R.bn_bwd_sums(dense, yg, fz["mean"], fz["istd"])
    co = R.bn_bwd_coeffs(s1, s2, count, gamma, fz["mean"], fz["istd"], frozen=True)
    dy, _ = R.bn_bwd_apply(dense, yg, co["ca"], co["cb"], co["cc"])
    yt = _nchw(y).requires_grad_(True)
    ga, be = torch.from_numpy(gamma).requires_grad_(True), torch.from_numpy(beta).requires_grad_(True)
    z = F.batch_norm(yt, torch.from_numpy(fin["mean"][0].copy()), torch.from_numpy(fin["var"][0].copy()), ga, be, False, 0.1, EPS)
    (F.max_pool2d(F.relu(z), 3, 2, 1) * _nchw(dp)).sum().backward()
    np.testing.assert_allclose(dy.reshape(y.shape), _nhwc(yt.grad), rtol=1e-10, atol=1e-10)
    np.testing.assert_allclose(co["dgamma"], ga.grad.numpy(), rtol=1e-10, atol=1e-10)
    np.testing.assert_allclose(co["dbeta"], be.grad.numpy(), rtol=1e-10, atol=1e-10)


def test_plane_layout_round_trip():
    """[C/32][3][P][32]: channel c of pixel p, plane k sits 64 * ((c / 32 * 3 + k) * P + p) + 16 * (c % 16 / 4) + 8 * (c / 16 % 2) +
    2 * (c % 4) bytes in; every word is written exactly once; decode(encode(x)) sums back to x bit for bit"""
    P, C = 7, 64
    x = np.random.RandomState(0).standard_normal((P, C)).astype(np.float32)
    x[0, :6] = np.array([0.0, -0.0, 2.0 ** -126, 1.0, 1.0 + 2.0 ** -10, -3.0], np.float32)
    assert R.plane_word(0, 0, P, 0) == 0 and R.plane_word(1, 0, P, 0) == 1 and R.plane_word(4, 0, P, 0) == 8
    assert R.plane_word(16, 0, P, 0) == 4 and R.plane_word(0, 1, P, 0) == 32 and R.plane_word(0, 0, P, 1) == 32 * P
    assert R.plane_word(32, 0, P, 0) == 3 * 32 * P and R.plane_word(63, P - 1, P, 2) == 3 * P * C - 1
    pp, cc = np.meshgrid(np.arange(P), np.arange(C), indexing="ij")
    idx = np.concatenate([R.plane_word(cc, pp, P, k).ravel() for k in range(3)])
    assert np.array_equal(np.sort(idx), np.arange(3 * P * C))
    w = R.encode_planes(x)
    h, m, l = R.decode_planes(w, P, C)
    assert R.same_floats(R.planes_sum(h, m, l), x)
    assert h.view(np.uint32)[0, 1] == 0x80000000 and R.planes_sum(h, m, l).view(np.uint32)[0, 1] == 0      # -0: sign in h only, reads back +0
    eh, em, el = R.planes_of(x)
    assert np.array_equal(h.view(np.uint32), eh.view(np.uint32)) and np.array_equal(l.view(np.uint32), el.view(np.uint32))
    # the two round-to-nearest-even ties of the split: low 16 bits 0x8000 under an even / odd upper half, and the same in x - h
    t = np.array([0x3F808000, 0x3F818000, 0x3F802020, 0x3F802060], np.uint32).view(np.float32)
    th, tm, tl = R.planes_of(t)
    assert list(th.view(np.uint32) >> 16) == [0x3F80, 0x3F82, 0x3F80, 0x3F80]
    assert list(tm[2:].astype(np.float64)) == [2.0 ** -10, 2.0 ** -10 * (1 + 2 / 128)]
    assert list(tl[2:].astype(np.float64)) == [2.0 ** -18, -2.0 ** -18]


def test_left_out_share_of_the_gpu_tests_seeds():
    """the random family compares a discrete decision only where its float64 margin exceeds the fp32 error bound; at the seeds
    tests/test_bn_kernels_gpu.py uses, that leaves out less than 0.1 % (expected for N(0, 1) operands: below 1e-5)"""
    from tests import test_bn_kernels_gpu as gpu
    for name, share in gpu.left_out_shares().items():
        assert share <= 1e-3, (name, share)
