"""float64 restatements of the EfficientNet-B0 depthwise, squeeze-excite and BN+activation kernels (csrc/effnet.hip) in the kernels' own layouts:
NHWC activations, depthwise weights [K*K][C] (tap kh * K + kw), TF-"same" padding given as (pad_t, pad_l) with the remainder at
the bottom / right, W2 stored transposed [Cs][C], the five per-image sums of k_se_bwd_bn1, the contiguous squeeze-excite gradient
range.  tests/test_eff_ref_cpu.py pins every function to torch float64 autograd; tests/test_eff_kernels_gpu.py holds the kernels
to them.  Every function is linear-algebra on whatever it is given, so calling it on absolute values yields the sum of |terms|
that the rounding bounds of the GPU tests need."""
import numpy as np

U = 2.0 ** -24          # fp32 unit roundoff


def same_pad(size, k, s):
    """top / left padding of TF-"same" for an input of `size` (oracle/efficientnet_ref.py: same_pad()[0])"""
    o = -(-size // s)
    return max((o - 1) * s + k - size, 0) // 2


def out_size(size, s):
    return -(-size // s)


def bf16_round(x):
    """round to nearest even onto bf16, returned as float64 (through fp32: exact for every value the dyadic family forms)"""
    u = np.ascontiguousarray(np.asarray(x, np.float32)).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    return r.astype(np.uint32).view(np.float32).astype(np.float64)


def bf16_words(x):
    """the 16-bit words of bf16-representable values"""
    u = np.ascontiguousarray(np.asarray(x, np.float32)).view(np.uint32)
    assert not (u & 0xFFFF).any(), "not bf16-representable"
    return (u >> 16).astype(np.uint16)


def bf16_decode(w):
    return (np.asarray(w).view(np.uint16).astype(np.uint32) << 16).view(np.float32)


def half_ulp_bf16(x):
    """half a bf16 ulp at |x| (normal range)"""
    a = np.maximum(np.abs(np.asarray(x, np.float64)), 2.0 ** -126)
    return np.exp2(np.floor(np.log2(a)) - 8)


def store(y, bf16):
    """the value a kernel leaves in memory: bf16 storage rounds to nearest even"""
    return bf16_round(y) if bf16 else np.asarray(y, np.float64)


def sigmoid(v):
    return 1.0 / (1.0 + np.exp(-np.asarray(v, np.float64)))


def swish(v):
    return v * sigmoid(v)


def swish_grad(v):
    s = sigmoid(v)
    return s * (1.0 + v * (1.0 - s))


def act(v, a):
    return v if a == 0 else (np.maximum(v, 0.0) if a == 1 else swish(v))


# ---- depthwise convolution -------------------------------------------------------------------------------------------------------
def _frame(N, Hi, Wi, Ho, Wo, C, K, s, pad_t, pad_l):
    return np.zeros((N, max((Ho - 1) * s + K, pad_t + Hi), max((Wo - 1) * s + K, pad_l + Wi), C), np.float64)


def dw_fwd(x, w, K, s, pad_t, pad_l):
    """x [N][Hi][Wi][C], w [K*K][C] -> y [N][Ho][Wo][C], Ho = ceil(Hi / s)"""
    x, w = np.asarray(x, np.float64), np.asarray(w, np.float64)
    N, Hi, Wi, C = x.shape
    Ho, Wo = out_size(Hi, s), out_size(Wi, s)
    xp = _frame(N, Hi, Wi, Ho, Wo, C, K, s, pad_t, pad_l)
    xp[:, pad_t:pad_t + Hi, pad_l:pad_l + Wi] = x
    y = np.zeros((N, Ho, Wo, C), np.float64)
    for kh in range(K):
        for kw in range(K):
            y += xp[:, kh:kh + (Ho - 1) * s + 1:s, kw:kw + (Wo - 1) * s + 1:s] * w[kh * K + kw]
    return y


def dw_dgrad(dy, w, K, s, pad_t, pad_l, Hi, Wi):
    """dy [N][Ho][Wo][C] -> dx [N][Hi][Wi][C]"""
    dy, w = np.asarray(dy, np.float64), np.asarray(w, np.float64)
    N, Ho, Wo, C = dy.shape
    dxp = _frame(N, Hi, Wi, Ho, Wo, C, K, s, pad_t, pad_l)
    for kh in range(K):
        for kw in range(K):
            dxp[:, kh:kh + (Ho - 1) * s + 1:s, kw:kw + (Wo - 1) * s + 1:s] += dy * w[kh * K + kw]
    return np.ascontiguousarray(dxp[:, pad_t:pad_t + Hi, pad_l:pad_l + Wi])


def dw_wgrad(dy, x, K, s, pad_t, pad_l):
    """-> dw [K*K][C]"""
    dy, x = np.asarray(dy, np.float64), np.asarray(x, np.float64)
    N, Hi, Wi, C = x.shape
    Ho, Wo = dy.shape[1:3]
    xp = _frame(N, Hi, Wi, Ho, Wo, C, K, s, pad_t, pad_l)
    xp[:, pad_t:pad_t + Hi, pad_l:pad_l + Wi] = x
    dw = np.zeros((K * K, C), np.float64)
    for kh in range(K):
        for kw in range(K):
            dw[kh * K + kw] = (dy * xp[:, kh:kh + (Ho - 1) * s + 1:s, kw:kw + (Wo - 1) * s + 1:s]).sum((0, 1, 2))
    return dw


def group_rows(t, groups):
    """t [N][H][W][C] -> [groups][rows][C] with the images split into `groups` equal runs"""
    N, C = t.shape[0], t.shape[-1]
    assert N % groups == 0
    return np.asarray(t, np.float64).reshape(groups, -1, C)


def bn_stats(y, groups):
    """(sum, sum of squares) per group and channel of the STORED y: [groups][2][C]"""
    g = group_rows(y, groups)
    return np.stack([g.sum(1), (g * g).sum(1)], 1)


def bn0_bwd_sums(dx, ye, mean, istd, scale, shift, groups):
    """S1 = sum dx swish'(v), S2 = sum dx swish'(v) xhat (kernels.h: k_chan_reduce mode 1) per group: [groups][2][C];
    mean .. shift [groups][C]"""
    d, y = group_rows(dx, groups), group_rows(ye, groups)
    m, i, sc, sh = (np.asarray(a, np.float64)[:, None, :] for a in (mean, istd, scale, shift))
    dyh = d * swish_grad(y * sc + sh)
    return np.stack([dyh.sum(1), (dyh * ((y - m) * i)).sum(1)], 1)


def pool_sums(y):
    """per-image channel sums [N][C] of y [N][...][C]"""
    y = np.asarray(y, np.float64)
    return y.reshape(y.shape[0], -1, y.shape[-1]).sum(1)


# ---- squeeze-excite ------------------------------------------------------------------------------------------------------------
def per_image(v, ipg, N):
    """[groups][C] -> [N][1][C], image i in group i // ipg"""
    return np.repeat(np.asarray(v, np.float64), ipg, axis=0)[:N, None, :]


def se_input(a, scale=None, shift=None, ipg=1):
    """A = a, or swish(a scale + shift) (the post-BN activation that is never materialised); a [N][HW][C]"""
    a = np.asarray(a, np.float64)
    if scale is None:
        return a
    return swish(a * per_image(scale, ipg, a.shape[0]) + per_image(shift, ipg, a.shape[0]))


def se_fwd(A, W1, b1, W2t, b2, pooled=None):
    """A [N][HW][C] -> sq [N][C], rpre [N][Cs], gate [N][C]; pooled [N][C] = the per-image sums when they come from elsewhere"""
    A = np.asarray(A, np.float64)
    W1, b1, W2t, b2 = (np.asarray(t, np.float64) for t in (W1, b1, W2t, b2))
    sq = (A.sum(1) if pooled is None else np.asarray(pooled, np.float64)) / A.shape[1]
    rpre = sq @ W1.T + b1
    gate = sigmoid(swish(rpre) @ W2t + b2)
    return sq, rpre, gate


def se_scale(A, gate):
    return np.asarray(A, np.float64) * np.asarray(gate, np.float64)[:, None, :]


def se_bwd_bn1(dout, y, scale, shift, mean, istd, ipg, gate, rpre, W1, W2t, pool5=None):
    """dout, y [N][HW][C]; -> pool5 [N][5][C] = per-image sums of (dout A, dout sg, dout sg xh, sg, sg xh) with v = y scale + shift,
    A = swish(v), sg = swish'(v), xh = (y - mean) istd;  dgp = R gate (1 - gate) [N][C], drp = (W2 dgp) swish'(rpre) [N][Cs],
    ds = W1^T drp [N][C];  bn [groups][2][C] = (S1, S2), S1 = sum_img gate P1 + ds / HW Q1, S2 = sum_img gate P2 + ds / HW Q2.
    pool5 given: the sums come from elsewhere (dout may be None)."""
    y = np.asarray(y, np.float64)
    N, HW, C = y.shape
    gate, rpre, W1, W2t = (np.asarray(t, np.float64) for t in (gate, rpre, W1, W2t))
    if pool5 is None:
        d = np.asarray(dout, np.float64)
        v = y * per_image(scale, ipg, N) + per_image(shift, ipg, N)
        xh = (y - per_image(mean, ipg, N)) * per_image(istd, ipg, N)
        A, sg = swish(v), swish_grad(v)
        pool5 = np.stack([(d * A).sum(1), (d * sg).sum(1), (d * sg * xh).sum(1), sg.sum(1), (sg * xh).sum(1)], 1)
    pool5 = np.asarray(pool5, np.float64)
    dgp = pool5[:, 0] * gate * (1.0 - gate)
    drp = (dgp @ W2t.T) * swish_grad(rpre)
    ds = drp @ W1
    s1 = gate * pool5[:, 1] + ds / HW * pool5[:, 3]
    s2 = gate * pool5[:, 2] + ds / HW * pool5[:, 4]
    bn = np.stack([s1.reshape(N // ipg, ipg, C).sum(1), s2.reshape(N // ipg, ipg, C).sum(1)], 1)
    return pool5, dgp, drp, ds, bn


def se_range_offsets(C, Cs):
    """offsets of (dW1, db1, dW2, db2) and the length of the contiguous gradient range [dW1 [Cs][C] | db1 padded to a multiple of 4 |
    dW2 transposed [Cs][C] | db2 [C]]"""
    o_b1 = Cs * C
    o_w2 = o_b1 + (Cs + 3) // 4 * 4
    o_b2 = o_w2 + Cs * C
    return o_b1, o_w2, o_b2, o_b2 + C


def se_wgrad(dgp, drp, rpre, sq):
    """-> the gradient range (pad slots after db1 are 0)"""
    dgp, drp, rpre, sq = (np.asarray(t, np.float64) for t in (dgp, drp, rpre, sq))
    C, Cs = dgp.shape[1], drp.shape[1]
    o_b1, o_w2, o_b2, n = se_range_offsets(C, Cs)
    out = np.zeros(n, np.float64)
    out[:o_b1] = (drp.T @ sq).reshape(-1)                   # dW1[j][c] = sum_img drp[img][j] sq[img][c]
    out[o_b1:o_b1 + Cs] = drp.sum(0)
    out[o_w2:o_b2] = (swish(rpre).T @ dgp).reshape(-1)       # dW2^T[j][c] = sum_img swish(rpre[img][j]) dgp[img][c]
    out[o_b2:] = dgp.sum(0)
    return out


# ---- BN + activation passes --------------------------------------------------------------------------------------------------------
# y, a, dz, res [groups][pix][C]; per-channel vectors [groups][C]; an image is HW consecutive pixels of a group; per-image operands
# rowscale [groups][pix / HW], gate / dsv [groups][pix / HW][C]
def _per_pixel(v, HW):
    """per-image operand -> per pixel: [groups][imgs] -> [groups][pix][1], [groups][imgs][C] -> [groups][pix][C]"""
    v = np.asarray(v, np.float64)
    return np.repeat(v, HW, axis=1)[..., None] if v.ndim == 2 else np.repeat(v, HW, axis=1)


def bnact_apply(y, scale, shift, HW, a, res=None, rowscale=None):
    """out = act(y scale + shift) * rowscale[img] + res   (k_bnact_apply)"""
    y, sc, sh = np.asarray(y, np.float64), np.asarray(scale, np.float64)[:, None, :], np.asarray(shift, np.float64)[:, None, :]
    out = act(y * sc + sh, a)
    if rowscale is not None:
        out = out * _per_pixel(rowscale, HW)
    return out if res is None else out + np.asarray(res, np.float64)


def bnact_dyh(d, y, HW, a, scale=None, shift=None, rowscale=None, gate=None, dsv=None):
    """the gradient reaching v = y scale + shift: d (with gate: d gate[img] + dsv[img] / HW, the squeeze-excite backward folded in)
    times act'(v) (act 0: 1, act 2: swish') times rowscale[img]"""
    d, y = np.asarray(d, np.float64), np.asarray(y, np.float64)
    if gate is not None:
        d = d * _per_pixel(gate, HW) + _per_pixel(dsv, HW) / HW
    if a == 2:
        d = d * swish_grad(y * np.asarray(scale, np.float64)[:, None, :] + np.asarray(shift, np.float64)[:, None, :])
    else:
        assert a == 0
    return d if rowscale is None else d * _per_pixel(rowscale, HW)


def chan_reduce(y, mode, HW=1, a=0, d=None, mean=None, istd=None, **kw):
    """[groups][2][C].  mode 0: (sum y, sum y^2); mode 1: (sum dyh, sum dyh xhat), xhat = (y - mean) istd   (k_chan_reduce)"""
    y = np.asarray(y, np.float64)
    if mode == 0:
        return np.stack([y.sum(1), (y * y).sum(1)], 1)
    dyh = bnact_dyh(d, y, HW, a, **kw)
    xh = (y - np.asarray(mean, np.float64)[:, None, :]) * np.asarray(istd, np.float64)[:, None, :]
    return np.stack([dyh.sum(1), (dyh * xh).sum(1)], 1)


def bnact_bwd_apply(dz, y, ca, cb, cc, HW, a, **kw):
    """dy = ca dyh + cb y + cc   (k_bnact_bwd_apply)"""
    ca, cb, cc = (np.asarray(t, np.float64)[:, None, :] for t in (ca, cb, cc))
    return ca * bnact_dyh(dz, y, HW, a, **kw) + cb * np.asarray(y, np.float64) + cc


def bn_bwd_coefficients(sums, gamma, mean, istd, n):
    """(ca, cb, cc) [groups][C] of the train-mode BatchNorm backward from the mode-1 sums (S1, S2) over n pixels per group:
    dy = gamma istd (dyh - S1 / n - xhat S2 / n)"""
    sums, gamma, mean, istd = (np.asarray(t, np.float64) for t in (sums, gamma, mean, istd))
    ca = gamma * istd
    cb = -ca * istd * sums[:, 1] / n
    return ca, cb, -ca * sums[:, 0] / n - cb * mean
