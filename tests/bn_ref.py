"""Plain float64 restatements of the kernels between ResNet-18's conv GEMMs (fedmlp_amd/csrc/elementwise.hip BatchNorm and stem
max-pool parts, planes_ew.hip), written for reading: the yardstick of tests/test_bn_kernels_gpu.py, itself pinned against torch
float64 autograd by tests/test_bn_ref_cpu.py.  Activations are NHWC; `groups` are the views of one forward (BatchNorm statistics
are per view).  Inputs are the kernels' fp32 operands widened to float64; nothing here rounds to fp32 except the plane split,
which is defined on fp32 values."""
import numpy as np

from tests.test_split3_cpu import bf16_rne, split3

U = 2.0 ** -24          # fp32 unit roundoff


def f64(a):
    return np.asarray(a, dtype=np.float64)


# ---- bf16 planes: P[C/32][3][pixels][32] ------------------------------------------------------------------------------------
def plane_word(c, p, P, plane):
    """index (in 16-bit words) of channel c of pixel p in plane `plane` (0 h, 1 m, 2 l) of a planes tensor over P pixels: the byte
    offset stated in planes_ew.hip -- 64 bytes per pixel and 32-channel block; an 8-channel chunk g = (c % 16) / 4 holds channels
    4g .. 4g+3 then 16+4g .. 16+4g+3 of the block -- halved"""
    c, p = np.asarray(c, np.int64), np.asarray(p, np.int64)
    byte = (((c >> 5) * 3 + plane) * P + p) * 64 + ((c & 15) >> 2) * 16 + ((c >> 4) & 1) * 8 + (c & 3) * 2
    return byte // 2


def planes_of(x):
    """the three planes of fp32 x: h = bf16_rne(x), m = bf16_rne(x - h), l = x - h - m (all fp32 arrays holding bf16 values)"""
    h, _, m, l = split3(np.asarray(x, np.float32))
    return h, m, l


def encode_planes(x):
    """fp32 [P][C] -> uint16 words [3 * P * C] in the kernels' layout"""
    x = np.asarray(x, np.float32)
    P, C = x.shape
    assert C % 32 == 0
    words = np.zeros(3 * P * C, np.uint16)
    pp, cc = np.meshgrid(np.arange(P), np.arange(C), indexing="ij")
    for plane, v in enumerate(planes_of(x)):
        assert np.array_equal(bf16_rne(v), v)
        words[plane_word(cc, pp, P, plane)] = (v.view(np.uint32) >> 16).astype(np.uint16)
    return words


def decode_planes(words, P, C):
    """uint16 words -> (h, m, l) fp32 [P][C]"""
    words = np.asarray(words).view(np.uint16)
    pp, cc = np.meshgrid(np.arange(P), np.arange(C), indexing="ij")
    return tuple((words[plane_word(cc, pp, P, plane)].astype(np.uint32) << 16).view(np.float32) for plane in range(3))


def planes_sum(h, m, l):
    """x back from its planes the way the kernels re-form it: (h + m) + l in fp32 (both additions are exact)"""
    return ((h + m).astype(np.float32) + l).astype(np.float32)


def same_floats(a, b):
    """bit equality of two fp32 arrays, a zero equal to a zero of either sign.  The planes keep the sign of -0 in h only (word
    0x8000, m = l = +0), and IEEE (-0) + (+0) = +0: a -0 reads back from its planes as +0.  Every other value is bit-exact."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and bool(((a.view(np.uint32) == b.view(np.uint32)) | ((a == 0) & (b == 0))).all())


# ---- BatchNorm forward ------------------------------------------------------------------------------------------------------
def tile_stats(x, tiles):
    """per-group per-tile (sum, sumsq) [groups][tiles][2][C] of x [groups][pix][C], pixels dealt to tiles in contiguous runs --
    the partials a conv epilogue leaves (float64; a test rounds them to fp32 to make the kernel's input)"""
    x = f64(x)
    G, pix, C = x.shape
    st = np.zeros((G, tiles, 2, C))
    for t, idx in enumerate(np.array_split(np.arange(pix), tiles)):
        st[:, t, 0] = x[:, idx].sum(1)
        st[:, t, 1] = (x[:, idx] ** 2).sum(1)
    return st


def bn_finalize(stats, count, gamma, beta, eps, momentum=0.1, run_mean=None, run_var=None, skip=False):
    """stats [groups][tiles][2][C] -> dict(mean, istd, scale, shift [groups][C]; run_mean, run_var [C]): biased variance
    (clamped at 0) for the normalisation; the running statistics move once per group, in group order, by `momentum` towards the
    mean and the UNBIASED variance (count > 1), like consecutive train-mode forwards; not at all when skip or run_mean is None"""
    stats, gamma, beta = f64(stats), f64(gamma), f64(beta)
    s = stats.sum(1)                                   # [groups][2][C]
    mean = s[:, 0] / count
    var = np.maximum(s[:, 1] / count - mean * mean, 0.0)
    istd = 1.0 / np.sqrt(var + float(eps))
    scale = gamma[None] * istd
    out = {"mean": mean, "var": var, "istd": istd, "scale": scale, "shift": beta[None] - mean * scale}
    if run_mean is not None:
        rm, rv = f64(run_mean).copy(), f64(run_var).copy()
        if not skip:
            for g in range(stats.shape[0]):
                unb = var[g] * count / (count - 1.0) if count > 1 else var[g]
                rm = (1.0 - momentum) * rm + momentum * mean[g]
                rv = (1.0 - momentum) * rv + momentum * unb
        out["run_mean"], out["run_var"] = rm, rv
    return out


def bn_frozen(groups, gamma, beta, run_mean, run_var, eps):
    """frozen statistics: every group normalises with the running ones"""
    gamma, beta, rm, rv = f64(gamma), f64(beta), f64(run_mean), f64(run_var)
    istd = 1.0 / np.sqrt(rv + float(eps))
    one = lambda v: np.repeat(v[None], groups, 0)
    return {"mean": one(rm), "istd": one(istd), "scale": one(gamma * istd), "shift": one(beta - rm * gamma * istd)}


def bn_apply(y, scale, shift, res=None, y2=None, scale2=None, shift2=None, relu=True):
    """y [groups][pix][C]: out = [relu](y * scale + shift [+ res] [+ y2 * scale2 + shift2]) and abs = the sum of the terms'
    magnitudes (what an fp32 error bound scales with)"""
    y, scale, shift = f64(y), f64(scale)[:, None], f64(shift)[:, None]
    v, a = y * scale + shift, np.abs(y * scale) + np.abs(shift)
    if res is not None:
        v, a = v + f64(res), a + np.abs(f64(res))
    if y2 is not None:
        t = f64(y2) * f64(scale2)[:, None]
        v, a = v + t + f64(shift2)[:, None], a + np.abs(t) + np.abs(f64(shift2)[:, None])
    pre = v
    return (np.maximum(v, 0.0) if relu else v), a, pre


# ---- stem max-pool 3x3 / stride 2 / pad 1 -----------------------------------------------------------------------------------
def pool_choice(a):
    """a [imgs][H][W][C] -> (pooled [imgs][H/2][W/2][C], code uint8, margin): code = kh * 3 + kw of the FIRST inside window
    position, in (kh, kw) row-major order, whose value is the window's maximum (a later one must be strictly greater to win);
    margin = the gap between the two largest inside values (0 at a tie)"""
    a = f64(a)
    N, H, W, C = a.shape
    Hp, Wp = H // 2, W // 2
    pad = np.full((N, H + 2, W + 2, C), -np.inf)
    pad[:, 1:-1, 1:-1] = a
    best = np.full((N, Hp, Wp, C), -np.inf)
    second = np.full((N, Hp, Wp, C), -np.inf)
    code = np.zeros((N, Hp, Wp, C), np.uint8)
    for kh in range(3):
        for kw in range(3):
            v = pad[:, kh:kh + H:2, kw:kw + W:2]                     # window position (kh, kw) of every pooled element
            win = v > best                                           # strict: -inf (outside) never wins, a tie keeps the first
            second = np.where(win, best, np.maximum(second, v))
            code = np.where(win, kh * 3 + kw, code).astype(np.uint8)
            best = np.where(win, v, best)
    return best, code, best - second


def stem_pool(y, scale=None, shift=None, ipg=None):
    """y [imgs][H][W][C]; scale / shift [groups][C] (group = imgs // ipg) or None = plain max-pool.  Returns pooled, code, margin and
    the dense pre-activation"""
    y = f64(y)
    if scale is None:
        return pool_choice(y) + (y,)
    g = np.arange(y.shape[0]) // ipg
    pre = y * f64(scale)[g][:, None, None] + f64(shift)[g][:, None, None]
    return pool_choice(np.maximum(pre, 0.0)) + (pre,)


def pool_route(dp, pooled, code, H, W):
    """dense gradient of relu + max-pool: every window sends its gradient to its argmax where pooled > 0"""
    dp, pooled = f64(dp), f64(pooled)
    N, Hp, Wp, C = dp.shape
    dense = np.zeros((N, H + 2, W + 2, C))
    g = np.where(pooled > 0, dp, 0.0)
    for kh in range(3):
        for kw in range(3):
            dense[:, kh:kh + H:2, kw:kw + W:2] += np.where(code == kh * 3 + kw, g, 0.0)
    return dense[:, 1:-1, 1:-1]


def gather_argmax(y, code):
    """y [imgs][H][W][C] at every pooled element's argmax"""
    y = f64(y)
    N, H, W, C = y.shape
    n, oh, ow, c = np.meshgrid(np.arange(N), np.arange(H // 2), np.arange(W // 2), np.arange(C), indexing="ij")
    return y[n, 2 * oh - 1 + code // 3, 2 * ow - 1 + code % 3, c]


# ---- BatchNorm backward -----------------------------------------------------------------------------------------------------
def bn_bwd_sums(dyh, y, mean, istd):
    """dyh (the gradient after the ReLU mask), y [groups][pix][C] -> s1 = sum dyh, s2 = sum dyh * xhat, and the sums of the terms'
    magnitudes a1, a2; [groups][C] each"""
    dyh, y = f64(dyh), f64(y)
    xh = (y - f64(mean)[:, None]) * f64(istd)[:, None]
    return dyh.sum(1), (dyh * xh).sum(1), np.abs(dyh).sum(1), np.abs(dyh * xh).sum(1)


def bn_bwd_coeffs(s1, s2, count, gamma, mean, istd, frozen=False):
    """dy = ca * dyh + cb * y + cc:  ca = gamma istd, cb = -ca istd s2 / count, cc = -cb mean - ca s1 / count (frozen statistics:
    cb = cc = 0); dgamma = sum over groups of s2, dbeta = of s1"""
    s1, s2, mean, istd = f64(s1), f64(s2), f64(mean), f64(istd)
    ca = f64(gamma)[None] * istd
    cb = np.zeros_like(ca) if frozen else -ca * istd * s2 / count
    cc = np.zeros_like(ca) if frozen else -cb * mean - ca * s1 / count
    return {"ca": ca, "cb": cb, "cc": cc, "dgamma": s2.sum(0), "dbeta": s1.sum(0)}


def bn_bwd_apply(dyh, y, ca, cb, cc):
    """-> dy and the sum of the three terms' magnitudes"""
    dyh, y, ca, cb, cc = f64(dyh), f64(y), f64(ca)[:, None], f64(cb)[:, None], f64(cc)[:, None]
    return ca * dyh + cb * y + cc, np.abs(ca * dyh) + np.abs(cb * y) + np.abs(cc)
